// ma_kernels.hip - batched Monge-Ampere target meshes, 2-D up to 32 x 32 (include/gadapt_mesh.h has the iteration).
//
// One workgroup per mesh, one lane per node, the whole pseudo-time relaxation inside the launch.  Unlike MMPDE5 the monitor is
// evaluated at the moving coordinates, so every step computes it from the mesh's Gaussians (at most 8; eight derived
// constants each, written to LDS once before the loop and read back as broadcasts).  A lane keeps its own phi in a register;
// the neighbours' come from two LDS images that alternate.
//
// Two barriers a step.  After the first the image is complete: every lane computes r and lambda of its node, and four wave
// reductions on DPP (sum of w r, max r, min r, min lambda; lanes without a node give 0, -inf, +inf, +inf) go to LDS.  After the
// second every lane combines the wave partials in increasing wave order, so all lanes hold the same bits of rbar, res and
// lmin, take the same exit or the same update, and write the next image.  Nothing a lane computed by itself decides an exit.
// One set of partials is enough: it is written between the barriers and read after the second, and the next write comes
// after the next first barrier.
//
// A mesh's thread count follows from its own node count, so its arithmetic and the order of its reduction do not depend on
// the batch; waves beyond a mesh's own only keep the barriers company.
//
// expf / logf / powf / sqrtf are the accurate ones; no FMA contraction (Makefile and the pragma below), as in
// mmpde5_kernels.hip: the parity bars are stated against plain fp32 arithmetic.
//
// ma_kernel: 126 VGPRs, no AGPRs, 83 SGPRs, no scratch, no spills (hipcc -Rpass-analysis=kernel-resource-usage, gfx950).
// 1024 lanes = 4 waves per SIMD allow 128 registers, and the compiler takes what the launch bounds allow: it unrolls the
// loop over the Gaussians around the inlined expf.  The state that has to live across the loop is about 20 registers.
//
// ma_m2n_kernel is the same iteration with the reference's M2N 'fast' monitor, m = reg + beta F / Fmax with Fmax the maximum of
// F over the mesh's nodes AT THIS STEP, so no residual can be formed before a workgroup-wide maximum.  Three barriers a step:
//   first -> second   the image is complete and only read: every lane forms x, y, det, lambda and F of its node (they live in
//                     registers across the second barrier, with phi); the wave maxima of F go to row 4 of the partials.
//   second -> third   every lane combines row 4 in increasing wave order (the same bits of Fmax in all lanes), forms m and r,
//                     and the four wave reductions of ma_kernel go to rows 0..3.
//   after the third   the combine, the exits and the update of ma_kernel; the next image is written.
// Row 4 is written between the first and the second barrier and read between the second and the third; rows 0..3 are written
// between the second and the third and read after the third; the next write of either comes after the next first (second)
// barrier.  Fmax has a row of its own: in row 0 wave 0 could write its sum of w r after the second barrier while another wave
// still reads that word as a maximum of F.  The image that is written after the third barrier was last read before the second.
// The choice between beta F / Fmax and 0 (no Gaussians, or F = 0 at every node) is made on the Fmax read from LDS.
// ma_m2n_kernel: 124 VGPRs, no AGPRs, 90 SGPRs, no scratch, no spills (the same report).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "gadapt_mesh.h"
#include "mesh_common.h"

#pragma clang fp contract(off)

using namespace gadapt_mesh_shared;                      // g_err, mesh_fail, dpp_move, wave_sum, wave_max, wave_min

namespace {

constexpr int MAX_SIDE = 32;
constexpr int MAX_NODES = MAX_SIDE * MAX_SIDE;
constexpr int MAX_WAVES = MAX_NODES / 64;
constexpr int MAX_GAUSS = 8;
constexpr int GAUSS_CONSTS = 8;                          // c0, c1, 1/q0, 1/q1, A0, B0, A1, B1
static_assert(MAX_NODES == GADAPT_MMPDE5_MAX_NODES, "one lane per node, one workgroup per mesh");

__host__ __device__ inline int ma_threads(int nodes) { return (nodes + 63) & ~63; }

// red[4][MAX_WAVES], the Gaussians' constants, then the two images of phi, each MAX of the batch's nodes long
constexpr int LDS_HEAD = 4 * MAX_WAVES + MAX_GAUSS * GAUSS_CONSTS;
__host__ __device__ inline int64_t ma_lds_floats(int nodes) { return LDS_HEAD + 2 * (int64_t)nodes; }

// ma_m2n_kernel: red[5][MAX_WAVES], the Gaussians' constants, Cxy in a 16-byte slot of its own, then the two images
constexpr int M2N_CXY = 5 * MAX_WAVES + MAX_GAUSS * GAUSS_CONSTS;
constexpr int M2N_LDS_HEAD = M2N_CXY + 4;
__host__ __device__ inline int64_t ma_m2n_lds_floats(int nodes) { return M2N_LDS_HEAD + 2 * (int64_t)nodes; }

__global__ __launch_bounds__(MAX_NODES) void ma_kernel(const int32_t* __restrict__ desc, const float* __restrict__ gauss,
                                                      const float* __restrict__ mon, double cfl, float tol, int tol_zero,
                                                      int max_steps, float* __restrict__ xo, float* __restrict__ yo,
                                                      int32_t* __restrict__ steps_out, float* __restrict__ res_out,
                                                      int32_t* __restrict__ status_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x;
    const int32_t* d = desc + GADAPT_MA_DESC * b;
    const int N = d[GADAPT_MA_D_N], noff = d[GADAPT_MA_D_NODE_OFF], goff = d[GADAPT_MA_D_GAUSS_OFF], ng = d[GADAPT_MA_D_GAUSS_N];
    const int nodes = N * N, nw = ma_threads(nodes) >> 6;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* red = lds;
    float* gc = lds + 4 * MAX_WAVES;
    float* img[2] = {lds + LDS_HEAD, lds + LDS_HEAD + nodes};

    const bool own = tid < nodes;
    const int c = own ? tid : 0;
    const int i = c / N, j = c - i * N;
    // even reflection: the neighbour beyond an edge is the one inside it
    const int rowE = (i == N - 1 ? N - 2 : i + 1) * N, rowW = (i == 0 ? 1 : i - 1) * N;
    const int jN = j == N - 1 ? N - 2 : j + 1, jS = j == 0 ? 1 : j - 1;
    const float n1 = (float)(N - 1);
    const float xi = (float)i / n1, xj = (float)j / n1;
    const float inv2h = 0.5f * n1, invh2 = n1 * n1, inv4h2 = 0.25f * invh2;   // exact: n1 <= 31
    const float wgt = ((i == 0 || i == N - 1) ? 0.5f : 1.0f) * ((j == 0 || j == N - 1) ? 0.5f : 1.0f);
    const float dt = (float)(cfl / ((double)(N - 1) * (double)(N - 1)));
    const float reg = mon[2 * b], power = mon[2 * b + 1];

    if (tid < ng) {                                      // ng <= 8 <= the threads of any mesh
        const float* g = gauss + 4 * (int64_t)(goff + tid);
        const float q0 = g[2] * g[2], q1 = g[3] * g[3];
        float* o = gc + GAUSS_CONSTS * tid;
        o[0] = g[0], o[1] = g[1], o[2] = 1.0f / q0, o[3] = 1.0f / q1;
        o[4] = 4.0f / (q0 * q0), o[5] = 2.0f / q0, o[6] = 4.0f / (q1 * q1), o[7] = 2.0f / q1;
    }
    float phi = 0.0f, x = xi, y = xj, res = 0.0f;
    if (own) img[0][c] = phi;
    int steps = 0, cur = 0, status;

    for (;;) {
        __syncthreads();                                 // image `cur` is complete (and, the first time, the constants)
        const float* p = img[cur];
        const float pE = p[rowE + j], pW = p[rowW + j], pN = p[i * N + jN], pS = p[i * N + jS];
        const float pEN = p[rowE + jN], pES = p[rowE + jS], pWN = p[rowW + jN], pWS = p[rowW + jS];
        x = xi + (pE - pW) * inv2h;
        y = xj + (pN - pS) * inv2h;
        const float A = 1.0f + ((pE - 2.0f * phi) + pW) * invh2;
        const float B = 1.0f + ((pN - 2.0f * phi) + pS) * invh2;
        const float Cc = (((pEN - pES) - pWN) + pWS) * inv4h2;
        const float det = A * B - Cc * Cc;
        const float lam = 0.5f * ((A + B) - sqrtf((A - B) * (A - B) + 4.0f * (Cc * Cc)));
        float uxx = 0.0f, uyy = 0.0f;
        for (int k = 0; k < ng; ++k) {
            const float4 g0 = *reinterpret_cast<const float4*>(gc + GAUSS_CONSTS * k);
            const float4 g1 = *reinterpret_cast<const float4*>(gc + GAUSS_CONSTS * k + 4);
            const float dx = x - g0.x, dy = y - g0.y;
            const float dx2 = dx * dx, dy2 = dy * dy;
            const float g = expf(-(dx2 * g0.z) - dy2 * g0.w);
            uxx = uxx + (g1.x * dx2 - g1.y) * g;
            uyy = uyy + (g1.z * dy2 - g1.w) * g;
        }
        const float m = powf(reg + sqrtf(uxx * uxx + uyy * uyy), power);
        const float r = logf(m * det);

        const float s_wr = wave_sum(own ? wgt * r : 0.0f);
        const float s_mx = wave_max(own ? r : -INFINITY);
        const float s_mn = wave_min(own ? r : INFINITY);
        const float s_lm = wave_min(own ? lam : INFINITY);
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
        const float rbar = sum / invh2;                  // the weights add up to (N - 1)^2
        res = fmaxf(mx - rbar, rbar - mn);
        // every value below was read from LDS by all lanes alike; written so that a NaN ends the loop
        if (!(lmin > 0.0f) || !(res - res == 0.0f)) { status = GADAPT_MA_NONCONVEX; break; }
        if (!tol_zero && res <= tol) { status = GADAPT_MA_CONVERGED; break; }
        if (steps >= max_steps) { status = GADAPT_MA_CAP; break; }
        phi = phi + (dt * fminf(1.0f, lmin)) * (r - rbar);
        ++steps;
        cur ^= 1;
        if (own) img[cur][c] = phi;                      // this image was last read before the barrier above
    }

    if (own) {
        xo[noff + c] = x;
        yo[noff + c] = y;
    }
    if (tid == 0) {
        steps_out[b] = steps;
        res_out[b] = res;
        status_out[b] = status;
    }
}

// The iteration of ma_kernel with the M2N 'fast' monitor (include/gadapt_mesh.h): mon[b] = (mon_reg, beta), no powf.
__global__ __launch_bounds__(MAX_NODES) void ma_m2n_kernel(const int32_t* __restrict__ desc, const float* __restrict__ gauss,
                                                          const float* __restrict__ mon, double cfl, float tol, int tol_zero,
                                                          int max_steps, float* __restrict__ xo, float* __restrict__ yo,
                                                          int32_t* __restrict__ steps_out, float* __restrict__ res_out,
                                                          int32_t* __restrict__ status_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x;
    const int32_t* d = desc + GADAPT_MA_DESC * b;
    const int N = d[GADAPT_MA_D_N], noff = d[GADAPT_MA_D_NODE_OFF], goff = d[GADAPT_MA_D_GAUSS_OFF], ng = d[GADAPT_MA_D_GAUSS_N];
    const int nodes = N * N, nw = ma_threads(nodes) >> 6;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* red = lds;
    float* gc = lds + 5 * MAX_WAVES;
    float* img[2] = {lds + M2N_LDS_HEAD, lds + M2N_LDS_HEAD + nodes};

    const bool own = tid < nodes;
    const int c = own ? tid : 0;
    const int i = c / N, j = c - i * N;
    // even reflection: the neighbour beyond an edge is the one inside it
    const int rowE = (i == N - 1 ? N - 2 : i + 1) * N, rowW = (i == 0 ? 1 : i - 1) * N;
    const int jN = j == N - 1 ? N - 2 : j + 1, jS = j == 0 ? 1 : j - 1;
    const float n1 = (float)(N - 1);
    const float xi = (float)i / n1, xj = (float)j / n1;
    const float inv2h = 0.5f * n1, invh2 = n1 * n1, inv4h2 = 0.25f * invh2;   // exact: n1 <= 31
    const float wgt = ((i == 0 || i == N - 1) ? 0.5f : 1.0f) * ((j == 0 || j == N - 1) ? 0.5f : 1.0f);
    const float dt = (float)(cfl / ((double)(N - 1) * (double)(N - 1)));
    const float reg = mon[2 * b], beta = mon[2 * b + 1];

    if (tid < ng) {                                      // ng <= 8 <= the threads of any mesh
        const float* g = gauss + 4 * (int64_t)(goff + tid);
        const float q0 = g[2] * g[2], q1 = g[3] * g[3];
        float* o = gc + GAUSS_CONSTS * tid;
        o[0] = g[0], o[1] = g[1], o[2] = 1.0f / q0, o[3] = 1.0f / q1;
        o[4] = 4.0f / (q0 * q0), o[5] = 2.0f / q0, o[6] = 4.0f / (q1 * q1), o[7] = 2.0f / q1;
        if (tid == ng - 1) lds[M2N_CXY] = (16.0f * o[2]) * o[3];   // u_xy is the LAST Gaussian's only, as in the reference
    }
    if (tid == 0 && ng == 0) lds[M2N_CXY] = 0.0f;       // read below whatever ng is: never an unwritten word
    float phi = 0.0f, x = xi, y = xj, res = 0.0f;
    if (own) img[0][c] = phi;
    int steps = 0, cur = 0, status;

    for (;;) {
        __syncthreads();                                 // image `cur` is complete (and, the first time, the constants)
        const float* p = img[cur];
        const float pE = p[rowE + j], pW = p[rowW + j], pN = p[i * N + jN], pS = p[i * N + jS];
        const float pEN = p[rowE + jN], pES = p[rowE + jS], pWN = p[rowW + jN], pWS = p[rowW + jS];
        x = xi + (pE - pW) * inv2h;
        y = xj + (pN - pS) * inv2h;
        const float A = 1.0f + ((pE - 2.0f * phi) + pW) * invh2;
        const float B = 1.0f + ((pN - 2.0f * phi) + pS) * invh2;
        const float Cc = (((pEN - pES) - pWN) + pWS) * inv4h2;
        const float det = A * B - Cc * Cc;
        const float lam = 0.5f * ((A + B) - sqrtf((A - B) * (A - B) + 4.0f * (Cc * Cc)));
        float uxx = 0.0f, uyy = 0.0f, dxl = 0.0f, dyl = 0.0f, gl = 0.0f;
        for (int k = 0; k < ng; ++k) {
            const float4 g0 = *reinterpret_cast<const float4*>(gc + GAUSS_CONSTS * k);
            const float4 g1 = *reinterpret_cast<const float4*>(gc + GAUSS_CONSTS * k + 4);
            const float dx = x - g0.x, dy = y - g0.y;
            const float dx2 = dx * dx, dy2 = dy * dy;
            const float g = expf(-(dx2 * g0.z) - dy2 * g0.w);
            uxx = uxx + (g1.x * dx2 - g1.y) * g;
            uyy = uyy + (g1.z * dy2 - g1.w) * g;
            dxl = dx, dyl = dy, gl = g;                  // what is left after the loop is the last Gaussian's
        }
        const float uxy = (lds[M2N_CXY] * (dxl * dyl)) * gl;
        const float Fn = sqrtf((uxx * uxx + 2.0f * (uxy * uxy)) + uyy * uyy);

        const float s_f = wave_max(own ? Fn : -INFINITY);
        if (lane == 0 && wave < nw) red[4 * MAX_WAVES + wave] = s_f;
        __syncthreads();                                 // the wave maxima of F are complete
        float fmx = red[4 * MAX_WAVES];
        for (int w = 1; w < nw; ++w) fmx = fmaxf(fmx, red[4 * MAX_WAVES + w]);
        // fmx was read from LDS by all lanes alike: a constant monitor is a decision of the whole mesh
        const float m = reg + (fmx > 0.0f ? beta * (Fn / fmx) : 0.0f);
        const float r = logf(m * det);

        const float s_wr = wave_sum(own ? wgt * r : 0.0f);
        const float s_mx = wave_max(own ? r : -INFINITY);
        const float s_mn = wave_min(own ? r : INFINITY);
        const float s_lm = wave_min(own ? lam : INFINITY);
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
        const float rbar = sum / invh2;                  // the weights add up to (N - 1)^2
        res = fmaxf(mx - rbar, rbar - mn);
        // every value below was read from LDS by all lanes alike; written so that a NaN ends the loop
        if (!(lmin > 0.0f) || !(res - res == 0.0f)) { status = GADAPT_MA_NONCONVEX; break; }
        if (!tol_zero && res <= tol) { status = GADAPT_MA_CONVERGED; break; }
        if (steps >= max_steps) { status = GADAPT_MA_CAP; break; }
        phi = phi + (dt * fminf(1.0f, lmin)) * (r - rbar);
        ++steps;
        cur ^= 1;
        if (own) img[cur][c] = phi;                      // this image was last read before the second barrier above
    }

    if (own) {
        xo[noff + c] = x;
        yo[noff + c] = y;
    }
    if (tid == 0) {
        steps_out[b] = steps;
        res_out[b] = res;
        status_out[b] = status;
    }
}

// The host side of both entry points: everything is checked on desc_host before the one launch.
int ma_launch(const char* who, bool m2n, int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* gauss, const float* mon,
              double cfl, double tol, int max_steps, float* x, float* y, int32_t* steps, float* residual, int32_t* status, void* stream) {
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
            snprintf(msg, sizeof msg, "%s: mesh %d: N = %d with %d Gaussians; N <= %d a side (one workgroup holds a mesh) "
                     "and at most %d Gaussians", who, b, N, ng, MAX_SIDE, MAX_GAUSS);
            return mesh_fail(GADAPT_MESH_E_SIZE, msg);
        }
        if ((int64_t)d[GADAPT_MA_D_NODE_OFF] + N * N > INT32_MAX) {
            snprintf(msg, sizeof msg, "%s: more than 2^31 nodes in one batch", who);
            return mesh_fail(GADAPT_MESH_E_SIZE, msg);
        }
        const int t = ma_threads(N * N);
        threads = t > threads ? t : threads;
        most = N * N > most ? N * N : most;
    }
    const float tol_f = (float)tol;
    if (m2n)
        ma_m2n_kernel<<<n_mesh, threads, (size_t)(4 * ma_m2n_lds_floats(most)), (hipStream_t)stream>>>(
            desc, gauss, mon, cfl, tol_f, tol_f == 0.0f, max_steps, x, y, steps, residual, status);
    else
        ma_kernel<<<n_mesh, threads, (size_t)(4 * ma_lds_floats(most)), (hipStream_t)stream>>>(
            desc, gauss, mon, cfl, tol_f, tol_f == 0.0f, max_steps, x, y, steps, residual, status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mesh_fail(GADAPT_MESH_E_LAUNCH, hipGetErrorString(e));
    return GADAPT_MESH_OK;
}

}  // namespace

extern "C" int gadapt_ma_max_side(void) { return MAX_SIDE; }
extern "C" int gadapt_ma_max_gauss(void) { return MAX_GAUSS; }

extern "C" int64_t gadapt_ma_lds_bytes(int nodes) {
    if (nodes < 9 || nodes > MAX_NODES) return mesh_fail(GADAPT_MESH_E_SIZE, "gadapt_ma_lds_bytes: 9..1024 nodes");
    return 4 * ma_lds_floats(nodes);
}

extern "C" int64_t gadapt_ma_m2n_lds_bytes(int nodes) {
    if (nodes < 9 || nodes > MAX_NODES) return mesh_fail(GADAPT_MESH_E_SIZE, "gadapt_ma_m2n_lds_bytes: 9..1024 nodes");
    return 4 * ma_m2n_lds_floats(nodes);
}

extern "C" int gadapt_ma_batch(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* gauss, const float* mon,
                               double cfl, double tol, int max_steps, float* x, float* y, int32_t* steps, float* residual,
                               int32_t* status, void* stream) {
    return ma_launch("gadapt_ma_batch", false, n_mesh, desc_host, desc, gauss, mon, cfl, tol, max_steps, x, y, steps, residual, status,
                     stream);
}

extern "C" int gadapt_ma_m2n_batch(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* gauss, const float* mon,
                                   double cfl, double tol, int max_steps, float* x, float* y, int32_t* steps, float* residual,
                                   int32_t* status, void* stream) {
    return ma_launch("gadapt_ma_m2n_batch", true, n_mesh, desc_host, desc, gauss, mon, cfl, tol, max_steps, x, y, steps, residual,
                     status, stream);
}
