// ma_kernels.hip - batched Monge-Ampere target meshes, 2-D up to 32 x 32: the lane route with the monitors that are computed
// from the mesh's Gaussians (include/gadapt_mesh.h has the iteration, ma_iteration.h its one statement, ma_host.h the launch).
//
// One workgroup per mesh, one lane per node.  Unlike MMPDE5 the monitor is evaluated at the moving coordinates, so every step
// computes it from the mesh's Gaussians (at most 8).
//
// ma_kernel: two barriers a step.  After the first the image is complete: every lane computes r and lambda of its node; the
// second is reduce_residual's, after which come the exits, the update and the next image.
// 116 VGPRs, no AGPRs, 82 SGPRs, no scratch, no spills (hipcc -Rpass-analysis=kernel-resource-usage, gfx950).  1024 lanes =
// 4 waves per SIMD allow 128 registers, and the compiler takes what the launch bounds allow: it unrolls the loop over the
// Gaussians around the inlined expf.  The state that has to live across the loop is about 20 registers.
//
// ma_m2n_kernel is the same iteration with the reference's M2N 'fast' monitor, m = reg + beta F / Fmax with Fmax the maximum of
// F over the mesh's nodes AT THIS STEP, so no residual can be formed before a workgroup-wide maximum.  Three barriers a step:
//   first -> second   the image is complete and only read: every lane forms x, y, det, lambda and F of its node (they live in
//                     registers across the second barrier, with phi); the wave maxima of F go to row 4 of the partials.
//   second -> third   every lane combines row 4 (the same bits of Fmax in all lanes), forms m and r, and reduce_residual's four
//                     wave reductions go to rows 0..3.
//   after the third   the exits and the update of ma_kernel; the next image is written.
// Row 4 is written between the first and the second barrier and read between the second and the third; the image that is written
// after the third barrier was last read before the second.  The choice between beta F / Fmax and 0 (no Gaussians, or F = 0 at
// every node) is made on the Fmax read from LDS.
// ma_m2n_kernel: 124 VGPRs, no AGPRs, 82 SGPRs, no scratch, no spills (the same report).
#include "ma_iteration.h"                            // and through it ma_host.h, mesh_common.h, gadapt_mesh.h

#pragma clang fp contract(off)

using namespace gadapt_ma;

namespace {

__global__ __launch_bounds__(LANE_MAX_NODES) void ma_kernel(const int32_t* __restrict__ desc, const float* __restrict__ gauss,
                                                      const float* __restrict__ mon, double cfl, float tol, int tol_zero,
                                                      int max_steps, float* __restrict__ xo, float* __restrict__ yo,
                                                      int32_t* __restrict__ steps_out, float* __restrict__ res_out,
                                                      int32_t* __restrict__ status_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x;
    const int32_t* d = desc + GADAPT_MA_DESC * b;
    const int N = d[GADAPT_MA_D_N], noff = d[GADAPT_MA_D_NODE_OFF], goff = d[GADAPT_MA_D_GAUSS_OFF], ng = d[GADAPT_MA_D_GAUSS_N];
    const int nodes = N * N, nw = ma_threads(nodes) >> 6, tid = threadIdx.x;
    float* red = lds;
    float* gc = lds + 4 * ROW;
    float* img[2] = {lds + MA_HEAD, lds + MA_HEAD + nodes};
    const LaneNode nd = lane_node(tid, N, cfl);
    const float reg = mon[2 * b], power = mon[2 * b + 1];

    gauss_to_lds(gauss, goff, ng, tid, gc, nullptr);
    float phi = 0.0f, r, res;
    NodeEval e;
    if (nd.own) img[0][nd.c] = phi;
    int cur = 0, steps, status;

    relax(tol, tol_zero, max_steps, steps, res, status,
          [&]() __attribute__((always_inline)) {
              e = lane_stencil(nd, N, img[cur], phi);
              float uxx = 0.0f, uyy = 0.0f;
              for (int k = 0; k < ng; ++k) gauss_term(gc, k, e.x, e.y, uxx, uyy);
              const float m = powf(reg + sqrtf(uxx * uxx + uyy * uyy), power);
              r = logf(m * e.det);
              return reduce_residual(red, tid, nw, nd, r, e.lam);
          },
          [&](const Reduced& q) __attribute__((always_inline)) { lane_update(nd, img, cur, phi, r, q); });

    if (nd.own) {
        xo[noff + nd.c] = e.x;
        yo[noff + nd.c] = e.y;
    }
    write_status(b, tid, steps, res, status, steps_out, res_out, status_out);
}

// The iteration of ma_kernel with the M2N 'fast' monitor (include/gadapt_mesh.h): mon[b] = (mon_reg, beta), no powf.
__global__ __launch_bounds__(LANE_MAX_NODES) void ma_m2n_kernel(const int32_t* __restrict__ desc, const float* __restrict__ gauss,
                                                          const float* __restrict__ mon, double cfl, float tol, int tol_zero,
                                                          int max_steps, float* __restrict__ xo, float* __restrict__ yo,
                                                          int32_t* __restrict__ steps_out, float* __restrict__ res_out,
                                                          int32_t* __restrict__ status_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x;
    const int32_t* d = desc + GADAPT_MA_DESC * b;
    const int N = d[GADAPT_MA_D_N], noff = d[GADAPT_MA_D_NODE_OFF], goff = d[GADAPT_MA_D_GAUSS_OFF], ng = d[GADAPT_MA_D_GAUSS_N];
    const int nodes = N * N, nw = ma_threads(nodes) >> 6, tid = threadIdx.x;
    float* red = lds;
    float* gc = lds + 5 * ROW;
    float* cxy = gc + MAX_GAUSS * GAUSS_CONSTS;
    float* img[2] = {lds + M2N_HEAD, lds + M2N_HEAD + nodes};
    const LaneNode nd = lane_node(tid, N, cfl);
    const float reg = mon[2 * b], beta = mon[2 * b + 1];

    gauss_to_lds(gauss, goff, ng, tid, gc, cxy);
    float phi = 0.0f, r, res;
    NodeEval e;
    if (nd.own) img[0][nd.c] = phi;
    int cur = 0, steps, status;

    relax(tol, tol_zero, max_steps, steps, res, status,
          [&]() __attribute__((always_inline)) {
              e = lane_stencil(nd, N, img[cur], phi);
              float uxx = 0.0f, uyy = 0.0f;
              GaussTerm last = {0.0f, 0.0f, 0.0f};
              for (int k = 0; k < ng; ++k) last = gauss_term(gc, k, e.x, e.y, uxx, uyy);   // what is left is the last Gaussian's
              const float Fn = hessian_norm(*cxy, last, uxx, uyy);

              wave_row_max(red, 4, tid, nw, nd.own ? Fn : -INFINITY);
              __syncthreads();                           // the wave maxima of F are complete
              const float fmx = row_max(red, 4, nw);
              const float m = reg + (fmx > 0.0f ? beta * (Fn / fmx) : 0.0f);
              r = logf(m * e.det);
              return reduce_residual(red, tid, nw, nd, r, e.lam);
          },
          [&](const Reduced& q) __attribute__((always_inline)) { lane_update(nd, img, cur, phi, r, q); });

    if (nd.own) {
        xo[noff + nd.c] = e.x;
        yo[noff + nd.c] = e.y;
    }
    write_status(b, tid, steps, res, status, steps_out, res_out, status_out);
}

// The host side of both entry points: everything is checked on desc_host before the one launch.
int ma_launch(const char* who, bool m2n, int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* gauss, const float* mon,
              double cfl, double tol, int max_steps, float* x, float* y, int32_t* steps, float* residual, int32_t* status, void* stream) {
    Geometry g;
    const int rc = check_batch(who, LANE_MAX_SIDE, ONE_WORKGROUP, false, n_mesh, desc_host, desc, gauss, mon, cfl, tol, max_steps, x, y,
                               steps, residual, status, &g);
    if (rc != GADAPT_MESH_OK) return rc;
    const float tol_f = (float)tol;
    return launch(m2n ? ma_m2n_kernel : ma_kernel, n_mesh, g.threads, lane_lds_bytes(m2n ? M2N_HEAD : MA_HEAD, g.side * g.side), stream,
                  desc, gauss, mon, cfl, tol_f, (int)(tol_f == 0.0f), max_steps, x, y, steps, residual, status);
}

}  // namespace

extern "C" int gadapt_ma_max_side(void) { return LANE_MAX_SIDE; }
extern "C" int gadapt_ma_max_gauss(void) { return MAX_GAUSS; }

extern "C" int64_t gadapt_ma_lds_bytes(int nodes) {
    if (nodes < 9 || nodes > LANE_MAX_NODES) return mesh_fail(GADAPT_MESH_E_SIZE, "gadapt_ma_lds_bytes: 9..1024 nodes");
    return lane_lds_bytes(MA_HEAD, nodes);
}

extern "C" int64_t gadapt_ma_m2n_lds_bytes(int nodes) {
    if (nodes < 9 || nodes > LANE_MAX_NODES) return mesh_fail(GADAPT_MESH_E_SIZE, "gadapt_ma_m2n_lds_bytes: 9..1024 nodes");
    return lane_lds_bytes(M2N_HEAD, nodes);
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
