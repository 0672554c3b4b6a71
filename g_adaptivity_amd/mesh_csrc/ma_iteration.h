// ma_iteration.h - the Monge-Ampere iteration of include/gadapt_mesh.h, stated once for the seven kernels that run it:
// ma_kernel, ma_m2n_kernel (ma_kernels.hip), ma_m2n_slow_kernel (ma_m2n_slow_kernels.hip), ma_table_kernel (ma_table_kernels.hip)
// on the lane route, ma_strided_kernel, ma_m2n_strided_kernel (ma_strided_kernels.hip) and ma_table_strided_kernel on the strided
// one.  ma_kernel and ma_m2n_kernel are written on all of it: what is left in their bodies is their monitor and its barrier
// phase.  The other five take from here the strided route's node and stencil definitions and the write-out, and keep the
// bodies they were timed with: restated on these helpers they ran 0.4 to 4 % longer than before, and one of them 0.7 to 1.8 %
// longer with no more than its prologue restated (docs/measurements.md), so for them the hazard arguments below describe the
// same scheme in their own lines.
//
// One workgroup per mesh, the whole pseudo-time relaxation inside the launch.  A mesh's thread count, its slots per lane and the
// order of its reductions follow from its own node count, so its bits do not depend on the batch; lanes and waves beyond a
// mesh's own (a launch has the threads of its largest mesh) only keep the barriers company, and every trip count depends on N
// alone, never on a lane.  Nothing a lane computed by itself decides an exit: every exit-deciding value is read back from LDS by
// all lanes alike (reduce_residual, row_max, relax).
//
// expf / logf / powf / sqrtf are the accurate ones; no FMA contraction (Makefile and the pragma below, which is in force in
// every translation unit from here on), as in mmpde5_kernels.hip: the parity bars are stated against plain fp32 arithmetic, and
// every expression below keeps the operands, the association and the order the recorded bits were made with
// (tests/test_gpu_ma_recorded_bits.py).
#ifndef GADAPT_MA_ITERATION_H
#define GADAPT_MA_ITERATION_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gadapt_mesh.h"
#include "ma_host.h"
#include "mesh_common.h"

#pragma clang fp contract(off)

namespace gadapt_ma {

using namespace gadapt_mesh_shared;                      // dpp_move, wave_sum, wave_max, wave_min

// ---- the Gaussians --------------------------------------------------------------------------------------------------------

// Eight derived constants per Gaussian, written to LDS once before the loop and read back as broadcasts (the first barrier of
// the first update covers them).  ng <= 8 <= the threads of any mesh.  `cxy`, where the monitor has a u_xy, is the LAST
// Gaussian's 16 / (q0 q1), as in the reference; it is read whatever ng is, so without Gaussians it is written as 0: never an
// unwritten word.
__device__ __forceinline__ void gauss_to_lds(const float* __restrict__ gauss, int goff, int ng, int tid, float* gc, float* cxy) {
    if (tid < ng) {
        const float* g = gauss + 4 * (int64_t)(goff + tid);
        const float q0 = g[2] * g[2], q1 = g[3] * g[3];
        float* o = gc + GAUSS_CONSTS * tid;
        o[0] = g[0], o[1] = g[1], o[2] = 1.0f / q0, o[3] = 1.0f / q1;
        o[4] = 4.0f / (q0 * q0), o[5] = 2.0f / q0, o[6] = 4.0f / (q1 * q1), o[7] = 2.0f / q1;
        if (cxy && tid == ng - 1) *cxy = (16.0f * o[2]) * o[3];
    }
    if (cxy && tid == 0 && ng == 0) *cxy = 0.0f;
}

struct GaussTerm {
    float dx, dy, g;                                     // what the M2N monitors keep of the last Gaussian, and u's summand
};

// Gaussian k at (x, y): adds its u_xx and u_yy.  The loop around it is the kernel's: the lane kernels let the compiler unroll it
// around the inlined expf (it takes the registers the launch bounds allow), the strided ones keep one copy (#pragma unroll 1).
__device__ __forceinline__ GaussTerm gauss_term(const float* gc, int k, float x, float y, float& uxx, float& uyy) {
    const float4 g0 = *reinterpret_cast<const float4*>(gc + GAUSS_CONSTS * k);
    const float4 g1 = *reinterpret_cast<const float4*>(gc + GAUSS_CONSTS * k + 4);
    const float dx = x - g0.x, dy = y - g0.y;
    const float dx2 = dx * dx, dy2 = dy * dy;
    const float g = expf(-(dx2 * g0.z) - dy2 * g0.w);
    uxx = uxx + (g1.x * dx2 - g1.y) * g;
    uyy = uyy + (g1.z * dy2 - g1.w) * g;
    return GaussTerm{dx, dy, g};
}

// F of the M2N monitors: u_xy is the last Gaussian's only (all zeros without one)
__device__ __forceinline__ float hessian_norm(float cxy, const GaussTerm& last, float uxx, float uyy) {
    const float uxy = (cxy * (last.dx * last.dy)) * last.g;
    return sqrtf((uxx * uxx + 2.0f * (uxy * uxy)) + uyy * uyy);
}

struct Reduced {
    float rbar, res, lmin;                               // of one update: the same bits in every lane (reduce_residual)
};

// ---- a node ---------------------------------------------------------------------------------------------------------------

struct NodeEval {
    float x, y, det, lam;                                // the moved node, det and the smaller eigenvalue of I + H phi
};

// det and lambda from the three fp32 entries of I + H phi, on both routes
__device__ __forceinline__ void det_lambda(float A, float B, float Cc, NodeEval& e) {
    e.det = A * B - Cc * Cc;
    e.lam = 0.5f * ((A + B) - sqrtf((A - B) * (A - B) + 4.0f * (Cc * Cc)));
}

// The lane route: lane `tid` owns node tid and keeps its phi in a register; the neighbours' come from two LDS images that
// alternate.  A lane without a node reads with node 0's indices and contributes 0, -inf, +inf, +inf.
struct LaneNode {
    bool own;
    int c, i, j, rowE, rowW, jN, jS;
    float xi, xj, inv2h, invh2, inv4h2, wgt, dt;
};

__device__ __forceinline__ LaneNode lane_node(int tid, int N, double cfl) {
    LaneNode n;
    n.own = tid < N * N;
    n.c = n.own ? tid : 0;
    const int i = n.c / N, j = n.c - i * N;
    n.i = i, n.j = j;
    // even reflection: the neighbour beyond an edge is the one inside it
    n.rowE = (i == N - 1 ? N - 2 : i + 1) * N, n.rowW = (i == 0 ? 1 : i - 1) * N;
    n.jN = j == N - 1 ? N - 2 : j + 1, n.jS = j == 0 ? 1 : j - 1;
    const float n1 = (float)(N - 1);
    n.xi = (float)i / n1, n.xj = (float)j / n1;
    n.inv2h = 0.5f * n1, n.invh2 = n1 * n1, n.inv4h2 = 0.25f * n.invh2;      // exact: n1 <= 31
    n.wgt = ((i == 0 || i == N - 1) ? 0.5f : 1.0f) * ((j == 0 || j == N - 1) ? 0.5f : 1.0f);
    n.dt = (float)(cfl / ((double)(N - 1) * (double)(N - 1)));
    return n;
}

// The nine-point stencil on the complete image p (only read between the barrier before and the next one)
__device__ __forceinline__ NodeEval lane_stencil(const LaneNode& n, int N, const float* p, float phi) {
    const int i = n.i, j = n.j;
    const float pE = p[n.rowE + j], pW = p[n.rowW + j], pN = p[i * N + n.jN], pS = p[i * N + n.jS];
    const float pEN = p[n.rowE + n.jN], pES = p[n.rowE + n.jS], pWN = p[n.rowW + n.jN], pWS = p[n.rowW + n.jS];
    NodeEval e;
    e.x = n.xi + (pE - pW) * n.inv2h;
    e.y = n.xj + (pN - pS) * n.inv2h;
    const float A = 1.0f + ((pE - 2.0f * phi) + pW) * n.invh2;
    const float B = 1.0f + ((pN - 2.0f * phi) + pS) * n.invh2;
    const float Cc = (((pEN - pES) - pWN) + pWS) * n.inv4h2;
    det_lambda(A, B, Cc, e);
    return e;
}

// The lane route's update, after the last barrier of the step: the other image was last read before that barrier
__device__ __forceinline__ void lane_update(const LaneNode& n, float* const (&img)[2], int& cur, float& phi, float r, const Reduced& q) {
    phi = phi + (n.dt * fminf(1.0f, q.lmin)) * (r - q.rbar);
    cur ^= 1;
    if (n.own) img[cur][n.c] = phi;
}

// The strided route: T = ma_threads(nodes) lanes, K = ceil(nodes / T) <= 7 nodes per lane, lane t owns nodes t + k T (the
// ownership of mmpde5_strided_kernel).  phi lives in ONE fp64 image in LDS and nowhere else: a lane reads its own phi from the
// image as it reads its neighbours', so no slot state but the kernel's own (K residuals r, fp32, in registers) has to survive
// from the evaluation to the update.  A kernel walks its slots in a real loop (#pragma unroll 1: one copy of the inlined expf /
// powf / logf), writes its per-slot state with a chain of selects under the loop counter and reads it in unrolled loops:
// constant register indices, no scratch.  The image is written only after the last barrier of a step, by the lanes that own
// the nodes, and next read after the following first barrier; x and y are not carried through the loop: after the exit the
// image still holds the last evaluated phi, and the epilogue forms them again with the evaluation's operations (moved_node).
// The three strided kernels share the definitions below.

// floor(c / N) for 0 <= c < N^2, 3 <= N <= 81: (c + 0.5) is exact, rN = 1 / N and the product are each within 2^-24 relative,
// so the product is within 81 * 2^-23 < 1e-5 of (c + 0.5) / N, which is at least 0.5 / 81 > 6e-3 away from every integer.
// No integer division per slot and step.
__device__ __forceinline__ int node_row(int c, float rN) { return (int)(((float)c + 0.5f) * rN); }

struct Stencil {
    int c, i, j, row, rowE, rowW, jN, jS;
};

// even reflection: the neighbour beyond an edge is the one inside it
__device__ __forceinline__ Stencil stencil_of(int c, int N, float rN) {
    Stencil s;
    const int i = node_row(c, rN);
    s.c = c, s.i = i, s.j = c - i * N, s.row = i * N;
    s.rowE = (i == N - 1 ? N - 2 : i + 1) * N, s.rowW = (i == 0 ? 1 : i - 1) * N;
    s.jN = s.j == N - 1 ? N - 2 : s.j + 1, s.jS = s.j == 0 ? 1 : s.j - 1;
    return s;
}

// x = xi + (float)((pE - pW) (n1 / 2)), y likewise: the evaluation and the epilogue share these operations
__device__ __forceinline__ void moved_node(const Stencil& s, double pE, double pW, double pN, double pS, float n1, double inv2h,
                                           float& x, float& y) {
    x = (float)s.i / n1 + (float)((pE - pW) * inv2h);
    y = (float)s.j / n1 + (float)((pN - pS) * inv2h);
}

__device__ __forceinline__ float node_weight(const Stencil& s, int N) {
    return ((s.i == 0 || s.i == N - 1) ? 0.5f : 1.0f) * ((s.j == 0 || s.j == N - 1) ? 0.5f : 1.0f);
}

// ---- the reductions and the exits -----------------------------------------------------------------------------------------

// Four wave reductions on DPP (sum of w r, max r, min r, min lambda) go to rows 0..3 of the partials; ONE BARRIER; every lane
// combines the wave partials in increasing wave order, so all lanes hold the same bits of rbar, res and lmin and take the same
// exit or the same update.  One set of partials is enough: a row is written before this barrier and read after it, and its next
// write comes after the next update's first barrier.  `invh2` = (N - 1)^2 is what the weights add up to.  After a NaN anywhere
// (a failed pivot of the slow kernel makes every r NaN) rbar and both operands of res are NaN.
__device__ __forceinline__ Reduced reduce_residual(float* red, int tid, int nw, float wr, float mx, float mn, float lm, float invh2) {
    const int wave = tid >> 6, lane = tid & 63;
    const float s_wr = wave_sum(wr);
    const float s_mx = wave_max(mx);
    const float s_mn = wave_min(mn);
    const float s_lm = wave_min(lm);
    if (lane == 0 && wave < nw) {
        red[wave] = s_wr, red[ROW + wave] = s_mx, red[2 * ROW + wave] = s_mn, red[3 * ROW + wave] = s_lm;
    }
    __syncthreads();
    float sum = red[0];
    Reduced q;
    mx = red[ROW], mn = red[2 * ROW], q.lmin = red[3 * ROW];
    for (int w = 1; w < nw; ++w) {
        sum = sum + red[w];
        mx = fmaxf(mx, red[ROW + w]);
        mn = fminf(mn, red[2 * ROW + w]);
        q.lmin = fminf(q.lmin, red[3 * ROW + w]);
    }
    q.rbar = sum / invh2;
    q.res = fmaxf(mx - q.rbar, q.rbar - mn);
    return q;
}

// The lane route's contribution: a lane without a node gives 0, -inf, +inf, +inf
__device__ __forceinline__ Reduced reduce_residual(float* red, int tid, int nw, const LaneNode& n, float r, float lam) {
    return reduce_residual(red, tid, nw, n.own ? n.wgt * r : 0.0f, n.own ? r : -INFINITY, n.own ? r : INFINITY,
                           n.own ? lam : INFINITY, n.invh2);
}

// A maximum over the mesh (Fmax, Emax of the M2N monitors) in a row of its own: wave_row_max before a barrier, row_max after
// it, in increasing wave order, so a constant monitor term is a decision of the whole mesh.  The row is written before that
// barrier and read between it and the next; a row shared with the sum of w r would let wave 0 write its sum after the barrier
// while another wave still reads that word as a maximum.
__device__ __forceinline__ void wave_row_max(float* red, int row, int tid, int nw, float v) {
    const int wave = tid >> 6, lane = tid & 63;
    const float s = wave_max(v);
    if (lane == 0 && wave < nw) red[row * ROW + wave] = s;
}

__device__ __forceinline__ float row_max(const float* red, int row, int nw) {
    float m = red[row * ROW];
#pragma clang loop vectorize_width(1)
    for (int w = 1; w < nw; ++w) m = fmaxf(m, red[row * ROW + w]);
    return m;
}

// The loop of every kernel: a barrier after which the image is complete (and, the first time, the Gaussians' constants);
// `evaluate()`, the kernel's own phases, which end with reduce_residual; the three exit tests in their order, on values every
// lane read from LDS alike and written so that a NaN ends the loop; `update(q)`, which writes the next image.  The barrier count
// per update is evaluate's plus this one.
template <class Evaluate, class Update>
__device__ __forceinline__ void relax(float tol, int tol_zero, int max_steps, int& steps, float& res, int& status, Evaluate evaluate,
                                      Update update) {
    steps = 0, res = 0.0f;
    for (;;) {
        __syncthreads();
        const Reduced q = evaluate();
        res = q.res;
        if (!(q.lmin > 0.0f) || !(res - res == 0.0f)) { status = GADAPT_MA_NONCONVEX; break; }
        if (!tol_zero && res <= tol) { status = GADAPT_MA_CONVERGED; break; }
        if (steps >= max_steps) { status = GADAPT_MA_CAP; break; }
        update(q);
        ++steps;
    }
}

__device__ __forceinline__ void write_status(int b, int tid, int steps, float res, int status, int32_t* __restrict__ steps_out,
                                             float* __restrict__ res_out, int32_t* __restrict__ status_out) {
    if (tid == 0) {
        steps_out[b] = steps;
        res_out[b] = res;
        status_out[b] = status;
    }
}

}  // namespace gadapt_ma

#endif
