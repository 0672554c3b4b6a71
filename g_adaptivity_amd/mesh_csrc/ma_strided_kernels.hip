// ma_strided_kernels.hip - batched Monge-Ampere target meshes up to 81 x 81 with an fp64 potential (route='strided';
// include/gadapt_mesh.h has the arithmetic, ma_kernels.hip the one-node-per-lane route this one is derived from).
//
// One workgroup per mesh, T = min(nodes rounded up to whole waves, 1024) lanes, K = ceil(nodes / T) <= 7 nodes per lane: lane t
// owns nodes t + k T, the ownership of mmpde5_strided_kernel.  The whole pseudo-time relaxation runs inside the launch.
//
// phi lives in ONE fp64 image in LDS and nowhere else: a lane reads its own phi from the image as it reads its neighbours',
// so no slot state but the K residuals r (fp32, registers) has to survive from the evaluation to the update.  Two barriers a
// step.  Between the first and the second the image is only read: a lane walks its slots in a real loop (not unrolled: one copy
// of the inlined expf / powf / logf), forms the five stencil expressions in fp64, rounds each to fp32 once, and does the rest in
// the lane route's fp32; its partial sums go through the DPP wave reductions to LDS.  After the second barrier every lane
// combines the wave partials in increasing wave order, so all lanes hold the same bits of rbar, res and lmin, take the same exit
// or the same update, and add their increments to their own nodes of the image.  The image is written only after the second
// barrier and next read after the following first one; the partials are written between the barriers and read after the second.
// Nothing a lane computed by itself decides an exit.
//
// r[k] is written with a chain of selects under the loop counter and read in an unrolled loop: constant register indices, no
// scratch.  The node's row and column come from a product with 1 / N (node_row below), not from an integer division per slot
// and step.  x and y are not carried: after the exit the image still holds the last evaluated phi, and the epilogue forms them
// again with the same operations.
//
// LDS: 512 bytes of partials and Gaussian constants, then 8 bytes per node of the launch's largest mesh: 52 488 + 512 = 53 000
// bytes at 81 x 81, below the 64 KB that need no raised limit.
//
// A mesh's T, K and reduction order follow from its own node count, so its bits do not depend on the batch; lanes and waves
// beyond a mesh's own only keep the barriers company.  expf / logf / powf / sqrtf are the accurate ones; no FMA contraction
// (Makefile and the pragma below), as in ma_kernels.hip.
//
// ma_strided_kernel: 70 VGPRs, no AGPRs, 95 SGPRs, no scratch, no spills (hipcc -Rpass-analysis=kernel-resource-usage, gfx950),
// one instance for every K; times and the parity table in docs/measurements.md.
//
// ma_m2n_strided_kernel is the same route with the reference's M2N 'fast' monitor, m = reg + beta F / Fmax with Fmax the maximum
// of F over the mesh's nodes at this step.  Three barriers a step:
//   first -> second   the image is complete and only read: the slot walk (a real loop, one copy of the inlined expf) forms
//                     det, lambda and F of each slot.  F[k] and det[k] (det itself, not its logarithm: r = logf(m det) stays
//                     the header's operation) replace r[k] as the per-slot state across the second barrier, written with the
//                     same select chain; a lane folds min lambda and, from -inf, max F over its slots in increasing k.  The
//                     wave maxima of F go to row 4 of the partials.
//   second -> third   every lane combines row 4 in increasing wave order, then a second walk over its slots (again a real
//                     loop, one copy of the inlined logf: F[k] and det[k] are read and r[k] written through select chains;
//                     the walk unrolled seven times with a branch per slot spilled 16 SGPRs) forms m and r[k] and
//                     accumulates sum w r, max r and min r; with the min lambda folded before, they go through the wave
//                     reductions to rows 0..3.
//   after the third   the combine, the exits and the update of ma_strided_kernel; the image is written.
// Row 4 is written between the first and the second barrier and read between the second and the third; rows 0..3 are written
// between the second and the third and read after the third (a row shared by Fmax and the sum of w r would let wave 0 overwrite
// a maximum another wave still reads).  The image is written only after the third barrier and next read after the following
// first one.  The choice between beta F / Fmax and 0 is made on the Fmax read from LDS.  LDS: a head of 592 bytes (five rows of
// partials, the Gaussians' constants, Cxy in a 16-byte slot) and the image: 53 080 bytes at 81 x 81.
// ma_m2n_strided_kernel: 80 VGPRs, no AGPRs, 101 SGPRs, no scratch, no spills (the same report), one instance for every K.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "gadapt_mesh.h"
#include "mesh_common.h"

#pragma clang fp contract(off)

using namespace gadapt_mesh_shared;                      // g_err, mesh_fail, dpp_move, wave_sum, wave_max, wave_min

namespace {

constexpr int MAX_SIDE = 81;
constexpr int MAX_NODES = MAX_SIDE * MAX_SIDE;
constexpr int MAX_THREADS = 1024;
constexpr int MAX_WAVES = MAX_THREADS / 64;
constexpr int MAX_K = (MAX_NODES + MAX_THREADS - 1) / MAX_THREADS;
constexpr int MAX_GAUSS = 8;                             // gadapt_ma_max_gauss(): both routes take the same Gaussians
constexpr int GAUSS_CONSTS = 8;                          // c0, c1, 1/q0, 1/q1, A0, B0, A1, B1
static_assert(MAX_K == 7, "ma_strided_kernel keeps seven residuals per lane");
static_assert(MAX_THREADS == GADAPT_MMPDE5_MAX_NODES, "the ownership of mmpde5_strided_kernel");

// red[4][MAX_WAVES] and the Gaussians' constants (fp32), then the fp64 image of phi
constexpr int LDS_HEAD_BYTES = 4 * (4 * MAX_WAVES + MAX_GAUSS * GAUSS_CONSTS);
static_assert(LDS_HEAD_BYTES % 16 == 0, "the image is read with 8-byte loads");
__host__ __device__ inline int64_t strided_lds_bytes(int nodes) { return LDS_HEAD_BYTES + 8 * (int64_t)nodes; }

// ma_m2n_strided_kernel: red[5][MAX_WAVES], the Gaussians' constants, Cxy in a 16-byte slot of its own, then the image
constexpr int M2N_CXY = 5 * MAX_WAVES + MAX_GAUSS * GAUSS_CONSTS;
constexpr int M2N_LDS_HEAD_BYTES = 4 * (M2N_CXY + 4);
static_assert(M2N_LDS_HEAD_BYTES % 16 == 0 && M2N_LDS_HEAD_BYTES <= 592, "the image is read with 8-byte loads");
__host__ __device__ inline int64_t m2n_strided_lds_bytes(int nodes) { return M2N_LDS_HEAD_BYTES + 8 * (int64_t)nodes; }

__host__ __device__ inline int strided_threads(int nodes) {
    const int t = (nodes + 63) & ~63;
    return t < MAX_THREADS ? t : MAX_THREADS;
}

// floor(c / N) for 0 <= c < N^2, 3 <= N <= 81: (c + 0.5) is exact, rN = 1 / N and the product are each within 2^-24 relative,
// so the product is within 81 * 2^-23 < 1e-5 of (c + 0.5) / N, which is at least 0.5 / 81 > 6e-3 away from every integer.
__device__ inline int node_row(int c, float rN) { return (int)(((float)c + 0.5f) * rN); }

struct Stencil {
    int c, i, j, row, rowE, rowW, jN, jS;
};

// even reflection: the neighbour beyond an edge is the one inside it
__device__ inline Stencil stencil_of(int c, int N, float rN) {
    Stencil s;
    const int i = node_row(c, rN);
    s.c = c, s.i = i, s.j = c - i * N, s.row = i * N;
    s.rowE = (i == N - 1 ? N - 2 : i + 1) * N, s.rowW = (i == 0 ? 1 : i - 1) * N;
    s.jN = s.j == N - 1 ? N - 2 : s.j + 1, s.jS = s.j == 0 ? 1 : s.j - 1;
    return s;
}

// x = xi + (float)((pE - pW) (n1 / 2)), y likewise: the evaluation and the epilogue share these operations
__device__ inline void moved_node(const Stencil& s, double pE, double pW, double pN, double pS, float n1, double inv2h, float& x,
                                  float& y) {
    x = (float)s.i / n1 + (float)((pE - pW) * inv2h);
    y = (float)s.j / n1 + (float)((pN - pS) * inv2h);
}

__global__ __launch_bounds__(MAX_THREADS) void ma_strided_kernel(const int32_t* __restrict__ desc, const float* __restrict__ gauss,
                                                                const float* __restrict__ mon, double cfl, float tol, int tol_zero,
                                                                int max_steps, float* __restrict__ xo, float* __restrict__ yo,
                                                                int32_t* __restrict__ steps_out, float* __restrict__ res_out,
                                                                int32_t* __restrict__ status_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int b = blockIdx.x;
    const int32_t* d = desc + GADAPT_MA_DESC * b;
    const int N = d[GADAPT_MA_D_N], noff = d[GADAPT_MA_D_NODE_OFF], goff = d[GADAPT_MA_D_GAUSS_OFF], ng = d[GADAPT_MA_D_GAUSS_N];
    const int nodes = N * N, T = strided_threads(nodes), nw = T >> 6, K = (nodes + T - 1) / T;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* red = reinterpret_cast<float*>(lds);
    float* gc = red + 4 * MAX_WAVES;
    double* img = reinterpret_cast<double*>(lds + LDS_HEAD_BYTES);

    const bool mine = tid < T;                           // a launch has the threads of its largest mesh
    const float n1 = (float)(N - 1), rN = 1.0f / (float)N;
    const double n1d = (double)(N - 1);
    const double inv2h = 0.5 * n1d, invh2 = n1d * n1d, inv4h2 = 0.25 * invh2;   // exact
    const float invh2f = n1 * n1;                                               // exact: n1 <= 80
    const float dt = (float)(cfl / invh2);
    const float reg = mon[2 * b], power = mon[2 * b + 1];

    if (tid < ng) {                                      // ng <= 8 <= the threads of any mesh
        const float* g = gauss + 4 * (int64_t)(goff + tid);
        const float q0 = g[2] * g[2], q1 = g[3] * g[3];
        float* o = gc + GAUSS_CONSTS * tid;
        o[0] = g[0], o[1] = g[1], o[2] = 1.0f / q0, o[3] = 1.0f / q1;
        o[4] = 4.0f / (q0 * q0), o[5] = 2.0f / q0, o[6] = 4.0f / (q1 * q1), o[7] = 2.0f / q1;
    }
    for (int k = 0; k < K; ++k) {
        const int idx = tid + k * T;
        if (mine && idx < nodes) img[idx] = 0.0;
    }
    float r[MAX_K];
#pragma unroll
    for (int q = 0; q < MAX_K; ++q) r[q] = 0.0f;
    float res = 0.0f;
    int steps = 0, status;

    for (;;) {
        __syncthreads();                                 // the image is complete (and, the first time, the constants)
        float a_wr = 0.0f, a_mx = -INFINITY, a_mn = INFINITY, a_lm = INFINITY;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const int idx = tid + k * T;
            const bool own = mine && idx < nodes;
            const Stencil s = stencil_of(own ? idx : 0, N, rN);
            const float wgt = ((s.i == 0 || s.i == N - 1) ? 0.5f : 1.0f) * ((s.j == 0 || s.j == N - 1) ? 0.5f : 1.0f);
            const double p0 = img[s.c];
            const double pE = img[s.rowE + s.j], pW = img[s.rowW + s.j], pN = img[s.row + s.jN], pS = img[s.row + s.jS];
            float x, y;
            moved_node(s, pE, pW, pN, pS, n1, inv2h, x, y);
            const double pEN = img[s.rowE + s.jN], pES = img[s.rowE + s.jS], pWN = img[s.rowW + s.jN], pWS = img[s.rowW + s.jS];
            const float A = (float)(1.0 + ((pE - 2.0 * p0) + pW) * invh2);
            const float B = (float)(1.0 + ((pN - 2.0 * p0) + pS) * invh2);
            const float Cc = (float)((((pEN - pES) - pWN) + pWS) * inv4h2);
            const float det = A * B - Cc * Cc;
            const float lam = 0.5f * ((A + B) - sqrtf((A - B) * (A - B) + 4.0f * (Cc * Cc)));
            float uxx = 0.0f, uyy = 0.0f;
#pragma unroll 1
            for (int g = 0; g < ng; ++g) {
                const float4 g0 = *reinterpret_cast<const float4*>(gc + GAUSS_CONSTS * g);
                const float4 g1 = *reinterpret_cast<const float4*>(gc + GAUSS_CONSTS * g + 4);
                const float dx = x - g0.x, dy = y - g0.y;
                const float dx2 = dx * dx, dy2 = dy * dy;
                const float e = expf(-(dx2 * g0.z) - dy2 * g0.w);
                uxx = uxx + (g1.x * dx2 - g1.y) * e;
                uyy = uyy + (g1.z * dy2 - g1.w) * e;
            }
            const float m = powf(reg + sqrtf(uxx * uxx + uyy * uyy), power);
            const float rv = logf(m * det);
            // a lane's own slots in increasing k; a slot without a node gives 0, -inf, +inf, +inf
            a_wr = a_wr + (own ? wgt * rv : 0.0f);
            a_mx = fmaxf(a_mx, own ? rv : -INFINITY);
            a_mn = fminf(a_mn, own ? rv : INFINITY);
            a_lm = fminf(a_lm, own ? lam : INFINITY);
#pragma unroll
            for (int q = 0; q < MAX_K; ++q) r[q] = q == k ? rv : r[q];
        }
        const float s_wr = wave_sum(a_wr);
        const float s_mx = wave_max(a_mx);
        const float s_mn = wave_min(a_mn);
        const float s_lm = wave_min(a_lm);
        if (lane == 0 && wave < nw) {
            red[wave] = s_wr, red[MAX_WAVES + wave] = s_mx, red[2 * MAX_WAVES + wave] = s_mn, red[3 * MAX_WAVES + wave] = s_lm;
        }
        __syncthreads();
        float sum = red[0], mx = red[MAX_WAVES], mn = red[2 * MAX_WAVES], lmin = red[3 * MAX_WAVES];
        for (int w = 1; w < nw; ++w) {
            sum = sum + red[w];
            mx = fmaxf(mx, red[MAX_WAVES + w]);
            mn = fminf(mn, red[2 * MAX_WAVES + w]);
            lmin = fminf(lmin, red[3 * MAX_WAVES + w]);
        }
        const float rbar = sum / invh2f;                 // the weights add up to (N - 1)^2
        res = fmaxf(mx - rbar, rbar - mn);
        // every value below was read from LDS by all lanes alike; written so that a NaN ends the loop
        if (!(lmin > 0.0f) || !(res - res == 0.0f)) { status = GADAPT_MA_NONCONVEX; break; }
        if (!tol_zero && res <= tol) { status = GADAPT_MA_CONVERGED; break; }
        if (steps >= max_steps) { status = GADAPT_MA_CAP; break; }
        const float dtl = dt * fminf(1.0f, lmin);
#pragma unroll
        for (int q = 0; q < MAX_K; ++q) {                // own nodes only: nobody reads them before the next barrier
            const int idx = tid + q * T;
            if (q < K && mine && idx < nodes) img[idx] = img[idx] + (double)(dtl * (r[q] - rbar));
        }
        ++steps;
    }

    // the image was not written after the last evaluation: x and y of that phi, the evaluation's operations again
    for (int k = 0; k < K; ++k) {
        const int idx = tid + k * T;
        if (mine && idx < nodes) {
            const Stencil s = stencil_of(idx, N, rN);
            float x, y;
            moved_node(s, img[s.rowE + s.j], img[s.rowW + s.j], img[s.row + s.jN], img[s.row + s.jS], n1, inv2h, x, y);
            xo[noff + idx] = x;
            yo[noff + idx] = y;
        }
    }
    if (tid == 0) {
        steps_out[b] = steps;
        res_out[b] = res;
        status_out[b] = status;
    }
}

__device__ inline float node_weight(const Stencil& s, int N) {
    return ((s.i == 0 || s.i == N - 1) ? 0.5f : 1.0f) * ((s.j == 0 || s.j == N - 1) ? 0.5f : 1.0f);
}

// The iteration of ma_strided_kernel with the M2N 'fast' monitor (include/gadapt_mesh.h): mon[b] = (mon_reg, beta), no powf.
__global__ __launch_bounds__(MAX_THREADS) void ma_m2n_strided_kernel(const int32_t* __restrict__ desc, const float* __restrict__ gauss,
                                                                    const float* __restrict__ mon, double cfl, float tol, int tol_zero,
                                                                    int max_steps, float* __restrict__ xo, float* __restrict__ yo,
                                                                    int32_t* __restrict__ steps_out, float* __restrict__ res_out,
                                                                    int32_t* __restrict__ status_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int b = blockIdx.x;
    const int32_t* d = desc + GADAPT_MA_DESC * b;
    const int N = d[GADAPT_MA_D_N], noff = d[GADAPT_MA_D_NODE_OFF], goff = d[GADAPT_MA_D_GAUSS_OFF], ng = d[GADAPT_MA_D_GAUSS_N];
    const int nodes = N * N, T = strided_threads(nodes), nw = T >> 6, K = (nodes + T - 1) / T;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* red = reinterpret_cast<float*>(lds);
    float* gc = red + 5 * MAX_WAVES;
    double* img = reinterpret_cast<double*>(lds + M2N_LDS_HEAD_BYTES);

    const bool mine = tid < T;                           // a launch has the threads of its largest mesh
    const float n1 = (float)(N - 1), rN = 1.0f / (float)N;
    const double n1d = (double)(N - 1);
    const double inv2h = 0.5 * n1d, invh2 = n1d * n1d, inv4h2 = 0.25 * invh2;   // exact
    const float invh2f = n1 * n1;                                               // exact: n1 <= 80
    const float dt = (float)(cfl / invh2);
    const float reg = mon[2 * b], beta = mon[2 * b + 1];

    if (tid < ng) {                                      // ng <= 8 <= the threads of any mesh
        const float* g = gauss + 4 * (int64_t)(goff + tid);
        const float q0 = g[2] * g[2], q1 = g[3] * g[3];
        float* o = gc + GAUSS_CONSTS * tid;
        o[0] = g[0], o[1] = g[1], o[2] = 1.0f / q0, o[3] = 1.0f / q1;
        o[4] = 4.0f / (q0 * q0), o[5] = 2.0f / q0, o[6] = 4.0f / (q1 * q1), o[7] = 2.0f / q1;
        if (tid == ng - 1) red[M2N_CXY] = (16.0f * o[2]) * o[3];   // u_xy is the LAST Gaussian's only, as in the reference
    }
    if (tid == 0 && ng == 0) red[M2N_CXY] = 0.0f;       // read below whatever ng is: never an unwritten word
    for (int k = 0; k < K; ++k) {
        const int idx = tid + k * T;
        if (mine && idx < nodes) img[idx] = 0.0;
    }
    float Fs[MAX_K], dets[MAX_K], r[MAX_K];
#pragma unroll
    for (int q = 0; q < MAX_K; ++q) Fs[q] = 0.0f, dets[q] = 1.0f, r[q] = 0.0f;
    float res = 0.0f;
    int steps = 0, status;

    for (;;) {
        __syncthreads();                                 // the image is complete (and, the first time, the constants)
        const float cxy = red[M2N_CXY];
        float a_f = -INFINITY, a_lm = INFINITY;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const int idx = tid + k * T;
            const bool own = mine && idx < nodes;
            const Stencil s = stencil_of(own ? idx : 0, N, rN);
            const double p0 = img[s.c];
            const double pE = img[s.rowE + s.j], pW = img[s.rowW + s.j], pN = img[s.row + s.jN], pS = img[s.row + s.jS];
            float x, y;
            moved_node(s, pE, pW, pN, pS, n1, inv2h, x, y);
            const double pEN = img[s.rowE + s.jN], pES = img[s.rowE + s.jS], pWN = img[s.rowW + s.jN], pWS = img[s.rowW + s.jS];
            const float A = (float)(1.0 + ((pE - 2.0 * p0) + pW) * invh2);
            const float B = (float)(1.0 + ((pN - 2.0 * p0) + pS) * invh2);
            const float Cc = (float)((((pEN - pES) - pWN) + pWS) * inv4h2);
            const float det = A * B - Cc * Cc;
            const float lam = 0.5f * ((A + B) - sqrtf((A - B) * (A - B) + 4.0f * (Cc * Cc)));
            float uxx = 0.0f, uyy = 0.0f, dxl = 0.0f, dyl = 0.0f, gl = 0.0f;
#pragma unroll 1
            for (int g = 0; g < ng; ++g) {
                const float4 g0 = *reinterpret_cast<const float4*>(gc + GAUSS_CONSTS * g);
                const float4 g1 = *reinterpret_cast<const float4*>(gc + GAUSS_CONSTS * g + 4);
                const float dx = x - g0.x, dy = y - g0.y;
                const float dx2 = dx * dx, dy2 = dy * dy;
                const float e = expf(-(dx2 * g0.z) - dy2 * g0.w);
                uxx = uxx + (g1.x * dx2 - g1.y) * e;
                uyy = uyy + (g1.z * dy2 - g1.w) * e;
                dxl = dx, dyl = dy, gl = e;              // what is left after the loop is the last Gaussian's
            }
            const float uxy = (cxy * (dxl * dyl)) * gl;
            const float Fn = sqrtf((uxx * uxx + 2.0f * (uxy * uxy)) + uyy * uyy);
            // a lane's own slots in increasing k; a slot without a node gives -inf, +inf
            a_f = fmaxf(a_f, own ? Fn : -INFINITY);
            a_lm = fminf(a_lm, own ? lam : INFINITY);
#pragma unroll
            for (int q = 0; q < MAX_K; ++q) Fs[q] = q == k ? Fn : Fs[q], dets[q] = q == k ? det : dets[q];
        }
        const float s_f = wave_max(a_f);
        if (lane == 0 && wave < nw) red[4 * MAX_WAVES + wave] = s_f;
        __syncthreads();                                 // the wave maxima of F are complete
        float fmx = red[4 * MAX_WAVES];
        for (int w = 1; w < nw; ++w) fmx = fmaxf(fmx, red[4 * MAX_WAVES + w]);
        // fmx was read from LDS by all lanes alike: a constant monitor is a decision of the whole mesh
        const bool flat = !(fmx > 0.0f);
        float a_wr = 0.0f, a_mx = -INFINITY, a_mn = INFINITY;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {                    // one copy of the inlined logf; the slot's F and det by select chains
            const int idx = tid + k * T;
            const bool own = mine && idx < nodes;
            const float wgt = node_weight(stencil_of(own ? idx : 0, N, rN), N);
            float Fk = Fs[0], detk = dets[0];
#pragma unroll
            for (int q = 1; q < MAX_K; ++q) Fk = q == k ? Fs[q] : Fk, detk = q == k ? dets[q] : detk;
            const float m = reg + (flat ? 0.0f : beta * (Fk / fmx));
            const float rv = logf(m * detk);
            a_wr = a_wr + (own ? wgt * rv : 0.0f);
            a_mx = fmaxf(a_mx, own ? rv : -INFINITY);
            a_mn = fminf(a_mn, own ? rv : INFINITY);
#pragma unroll
            for (int q = 0; q < MAX_K; ++q) r[q] = q == k ? rv : r[q];
        }
        const float s_wr = wave_sum(a_wr);
        const float s_mx = wave_max(a_mx);
        const float s_mn = wave_min(a_mn);
        const float s_lm = wave_min(a_lm);
        if (lane == 0 && wave < nw) {
            red[wave] = s_wr, red[MAX_WAVES + wave] = s_mx, red[2 * MAX_WAVES + wave] = s_mn, red[3 * MAX_WAVES + wave] = s_lm;
        }
        __syncthreads();
        float sum = red[0], mx = red[MAX_WAVES], mn = red[2 * MAX_WAVES], lmin = red[3 * MAX_WAVES];
        for (int w = 1; w < nw; ++w) {
            sum = sum + red[w];
            mx = fmaxf(mx, red[MAX_WAVES + w]);
            mn = fminf(mn, red[2 * MAX_WAVES + w]);
            lmin = fminf(lmin, red[3 * MAX_WAVES + w]);
        }
        const float rbar = sum / invh2f;                 // the weights add up to (N - 1)^2
        res = fmaxf(mx - rbar, rbar - mn);
        // every value below was read from LDS by all lanes alike; written so that a NaN ends the loop
        if (!(lmin > 0.0f) || !(res - res == 0.0f)) { status = GADAPT_MA_NONCONVEX; break; }
        if (!tol_zero && res <= tol) { status = GADAPT_MA_CONVERGED; break; }
        if (steps >= max_steps) { status = GADAPT_MA_CAP; break; }
        const float dtl = dt * fminf(1.0f, lmin);
#pragma unroll
        for (int q = 0; q < MAX_K; ++q) {                // own nodes only: nobody reads them before the next barrier
            const int idx = tid + q * T;
            if (q < K && mine && idx < nodes) img[idx] = img[idx] + (double)(dtl * (r[q] - rbar));
        }
        ++steps;
    }

    // the image was not written after the last evaluation: x and y of that phi, the evaluation's operations again
    for (int k = 0; k < K; ++k) {
        const int idx = tid + k * T;
        if (mine && idx < nodes) {
            const Stencil s = stencil_of(idx, N, rN);
            float x, y;
            moved_node(s, img[s.rowE + s.j], img[s.rowW + s.j], img[s.row + s.jN], img[s.row + s.jS], n1, inv2h, x, y);
            xo[noff + idx] = x;
            yo[noff + idx] = y;
        }
    }
    if (tid == 0) {
        steps_out[b] = steps;
        res_out[b] = res;
        status_out[b] = status;
    }
}

// The host side of both entry points: everything is checked on desc_host before the one launch.
int strided_launch(const char* who, bool m2n, int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* gauss,
                   const float* mon, double cfl, double tol, int max_steps, float* x, float* y, int32_t* steps, float* residual,
                   int32_t* status, void* stream) {
    char msg[240];
    if (n_mesh < 1 || !desc_host || !desc || !mon || !x || !y || !steps || !residual || !status) {
        snprintf(msg, sizeof msg, "%s: empty batch or null pointer", who);
        return mesh_fail(GADAPT_MESH_E_BADARG, msg);
    }
    if (!(cfl > 0.0) || !(tol >= 0.0) || !isfinite(cfl) || !isfinite(tol)) {
        snprintf(msg, sizeof msg, "%s: need cfl > 0 and tol >= 0, both finite", who);
        return mesh_fail(GADAPT_MESH_E_BADARG, msg);
    }
    if (max_steps < 0 || max_steps > GADAPT_MMPDE5_MAX_STEPS) {
        snprintf(msg, sizeof msg, "%s: max_steps %d; 0..%d supported (the loop must end)", who, max_steps, GADAPT_MMPDE5_MAX_STEPS);
        return mesh_fail(GADAPT_MESH_E_SIZE, msg);
    }
    int threads = 64, most = 0;
    for (int b = 0; b < n_mesh; ++b) {
        const int32_t* d = desc_host + GADAPT_MA_DESC * b;
        const int N = d[GADAPT_MA_D_N], ng = d[GADAPT_MA_D_GAUSS_N];
        if (N < 3 || d[GADAPT_MA_D_NODE_OFF] < 0 || d[GADAPT_MA_D_GAUSS_OFF] < 0 || ng < 0 || (ng > 0 && !gauss)) {
            snprintf(msg, sizeof msg, "%s: mesh %d: N %d, offsets %d / %d, %d Gaussians", who, b, N, d[GADAPT_MA_D_NODE_OFF],
                     d[GADAPT_MA_D_GAUSS_OFF], ng);
            return mesh_fail(GADAPT_MESH_E_BADARG, msg);
        }
        if (N > MAX_SIDE || ng > MAX_GAUSS) {
            snprintf(msg, sizeof msg, "%s: mesh %d: N = %d with %d Gaussians; N <= %d a side (one workgroup holds a mesh) and at most "
                     "%d Gaussians", who, b, N, ng, MAX_SIDE, MAX_GAUSS);
            return mesh_fail(GADAPT_MESH_E_SIZE, msg);
        }
        if ((int64_t)d[GADAPT_MA_D_NODE_OFF] + N * N > INT32_MAX) {
            snprintf(msg, sizeof msg, "%s: more than 2^31 nodes in one batch", who);
            return mesh_fail(GADAPT_MESH_E_SIZE, msg);
        }
        const int t = strided_threads(N * N);
        threads = t > threads ? t : threads;
        most = N * N > most ? N * N : most;
    }
    const float tol_f = (float)tol;
    if (m2n)
        ma_m2n_strided_kernel<<<n_mesh, threads, (size_t)m2n_strided_lds_bytes(most), (hipStream_t)stream>>>(
            desc, gauss, mon, cfl, tol_f, tol_f == 0.0f, max_steps, x, y, steps, residual, status);
    else
        ma_strided_kernel<<<n_mesh, threads, (size_t)strided_lds_bytes(most), (hipStream_t)stream>>>(
            desc, gauss, mon, cfl, tol_f, tol_f == 0.0f, max_steps, x, y, steps, residual, status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mesh_fail(GADAPT_MESH_E_LAUNCH, hipGetErrorString(e));
    return GADAPT_MESH_OK;
}

}  // namespace

extern "C" int gadapt_ma_strided_max_side(void) { return MAX_SIDE; }

extern "C" int64_t gadapt_ma_strided_lds_bytes(int nodes) {
    if (nodes < 9 || nodes > MAX_NODES) return mesh_fail(GADAPT_MESH_E_SIZE, "gadapt_ma_strided_lds_bytes: 9..6561 nodes");
    return strided_lds_bytes(nodes);
}

extern "C" int64_t gadapt_ma_m2n_strided_lds_bytes(int nodes) {
    if (nodes < 9 || nodes > MAX_NODES) return mesh_fail(GADAPT_MESH_E_SIZE, "gadapt_ma_m2n_strided_lds_bytes: 9..6561 nodes");
    return m2n_strided_lds_bytes(nodes);
}

extern "C" int gadapt_ma_batch_strided(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* gauss,
                                       const float* mon, double cfl, double tol, int max_steps, float* x, float* y, int32_t* steps,
                                       float* residual, int32_t* status, void* stream) {
    return strided_launch("gadapt_ma_batch_strided", false, n_mesh, desc_host, desc, gauss, mon, cfl, tol, max_steps, x, y, steps,
                          residual, status, stream);
}

extern "C" int gadapt_ma_m2n_batch_strided(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* gauss,
                                           const float* mon, double cfl, double tol, int max_steps, float* x, float* y,
                                           int32_t* steps, float* residual, int32_t* status, void* stream) {
    return strided_launch("gadapt_ma_m2n_batch_strided", true, n_mesh, desc_host, desc, gauss, mon, cfl, tol, max_steps, x, y, steps,
                          residual, status, stream);
}
