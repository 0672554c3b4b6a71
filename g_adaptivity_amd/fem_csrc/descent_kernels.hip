// descent_kernels.hip - gradient descent of the mesh nodes on the FEM error (the reference's backFEM baselines:
// train_step_adjoint, difFEM_2d.py:593-685, and train_step_vec, difFEM_1d.py:241-292), all epochs enqueued by one call.
//
// An epoch is the launches the modular loss already has - fem_launch_modular_forward + fem_launch_backward (fem_host.h) in 2-D,
// fem1d_launch_poisson_forward + the L2 seed below + fem1d_launch_poisson_backward in 1-D - followed by one step launch that
// does what torch.optim.SGD does (x - lr * g, the product rounded before the subtraction), keeps the epoch's loss and mesh
// and watches for tangling.  One workgroup per mesh in the step launches; every reduction runs in a fixed order.
#include <math.h>
#include <stdio.h>
#include "fem_common.h"
#include "fem1d_common.h"
#include "fem_host.h"

#pragma clang fp contract(off)

using fem::V2;
using fem::ld2;

#define DESC_THREADS 256
#define DESC_MAX_WAVES 16                  // a 1024-lane workgroup

// the smaller of a and b; a NaN in either is kept
__device__ inline float min_nan(float a, float b) { return a != a ? a : (b != b ? b : fminf(a, b)); }

// min_nan over the workgroup (a multiple of 64 lanes): by wave with shuffles, then the waves' results in wave order.  Every
// lane returns the result; waves[] (DESC_MAX_WAVES floats of LDS) is free again on return.
__device__ inline float block_min_nan(float v, float* waves) {
    for (int off = 32; off > 0; off >>= 1) v = min_nan(v, __shfl_down(v, off, 64));
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = waves[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = min_nan(m, waves[w]);
    __syncthreads();
    return m;
}

// thread 0 of mesh b's workgroup: this epoch's loss, and the watch.  min_area follows the epochs until the mesh tangles
// (minimum <= 0 or NaN) and keeps the value of that epoch from then on.
__device__ inline void record_epoch(int b, int n_meshes, int epoch, float m, const float* __restrict__ loss,
                                    float* __restrict__ loss_hist, int32_t* __restrict__ first_tangled, float* __restrict__ min_area) {
    loss_hist[(int64_t)epoch * n_meshes + b] = loss[b];
    if (first_tangled[b] < 0) {
        min_area[b] = m;
        if (!(m > 0.0f)) first_tangled[b] = epoch;
    }
}

// ---------------------------------------------------------------------------------------------------- 2-D
// the determinant D of tri_geometry (fem_kernels.hip), term for term: twice the signed area of triangle t
__device__ inline float tri_det(const float* x, const int32_t* __restrict__ cells, int t) {
    const V2 p0 = ld2(x, cells[3 * t]), p1 = ld2(x, cells[3 * t + 1]), p2 = ld2(x, cells[3 * t + 2]);
    return p0.x * (p1.y - p2.y) + p1.x * (p2.y - p0.y) + p2.x * (p0.y - p1.y);
}

// before epoch 0: the orientation of every triangle on the reference mesh (-1, 0, 1; 0 for a degenerate or NaN one, which
// then counts as tangled), and the watch's start values
__global__ void __launch_bounds__(DESC_THREADS) fem_descent_sign_kernel(int n_tris, int n_meshes, const int32_t* __restrict__ cells,
                                                                        const float* __restrict__ x_ref, int8_t* __restrict__ sign,
                                                                        int32_t* __restrict__ first_tangled, float* __restrict__ min_area) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_tris) {
        const float D = tri_det(x_ref, cells, i);
        sign[i] = (int8_t)((D > 0.0f) - (D < 0.0f));
    }
    if (i < n_meshes) {
        first_tangled[i] = -1;
        min_area[i] = INFINITY;
    }
}

// x is read and written by the same workgroup (the new coordinates feed the watch): no __restrict__ on it
__global__ void __launch_bounds__(DESC_THREADS) fem_descent_step_kernel(const int32_t* __restrict__ meta, const int32_t* __restrict__ cells,
                                                                        const int32_t* __restrict__ int_idx, const int8_t* __restrict__ sign,
                                                                        const float* __restrict__ gx, const float* __restrict__ loss,
                                                                        float lr, int epoch, int n_meshes, int n_nodes, float* x,
                                                                        float* __restrict__ loss_hist, float* __restrict__ mesh_hist,
                                                                        int32_t* __restrict__ first_tangled, float* __restrict__ min_area) {
    __shared__ float waves[DESC_MAX_WAVES];
    const int b = blockIdx.x;
    const int32_t* mt = meta + b * GADAPT_FEM_META;
    const int v0 = mt[GADAPT_FEM_M_NODE_OFF], nn = mt[GADAPT_FEM_M_N_NODES];
    const int t0 = mt[GADAPT_FEM_M_TRI_OFF], nt = mt[GADAPT_FEM_M_N_TRIS];
    float* hist = mesh_hist ? mesh_hist + ((int64_t)epoch * n_nodes + v0) * 2 : nullptr;
    for (int i = threadIdx.x; i < nn; i += DESC_THREADS) {
        const int v = v0 + i;
        float a = x[2 * v], c = x[2 * v + 1];
        if (int_idx[v] >= 0) {                                  // boundary nodes stay as they are, bit for bit
            const float pa = lr * gx[2 * v], pc = lr * gx[2 * v + 1];
            a = a - pa;
            c = c - pc;
            x[2 * v] = a;
            x[2 * v + 1] = c;
        }
        if (hist) {
            hist[2 * i] = a;
            hist[2 * i + 1] = c;
        }
    }
    __syncthreads();
    float m = INFINITY;
    for (int i = threadIdx.x; i < nt; i += DESC_THREADS) m = min_nan(m, tri_det(x, cells, t0 + i) * (float)sign[t0 + i]);
    m = block_min_nan(m, waves);
    if (threadIdx.x == 0) record_epoch(b, n_meshes, epoch, m, loss, loss_hist, first_tangled, min_area);
}

// Both 2-D entry points, under the name `who`.  routes: GADAPT_FEM_ROUTE_WAVE_FORWARD and _ADJOINT select the wave-parallel
// form of an epoch's forward and backward launches (fem_host.h), which have the lane kernels' bits; 0 is gadapt_fem_descend.
static int descend_2d(const char* who, int routes, int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                      const int32_t* tri_mesh, const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                      const int32_t* nt_idx, const int32_t* gptr, const float* gpar, float* x, const float* x_ref, const float* lat_x,
                      const float* lat_y, int nlat, int max_lds_bytes, int max_tris, int epochs, float lr, float* rhs, float* coeffs,
                      float* lfac, float* sol, float* loss, float* g_sol, float* gc, float* mu, float* tgrad, float* gx, float* loss_hist,
                      float* mesh_hist, int32_t* first_tangled, float* min_area, int8_t* sign, void* stream) {
    if (B <= 0 || N <= 0 || T <= 0 || epochs < 0 || !meta || !cells || !node_mesh || !tri_mesh || !int_idx || !int_node || !nt_ptr ||
        !nt_idx || !gptr || !gpar || !x || !lat_x || !lat_y || !rhs || !coeffs || !lfac || !sol || !loss || !g_sol || !gc || !mu ||
        !tgrad || !gx || !first_tangled || !min_area || !sign || (epochs > 0 && !loss_hist) || max_tris <= 0)
        return fem_fail_as(GADAPT_FEM_E_BADARG, who, "null pointer or bad size");
    if (nlat < 3 || !(nlat & 1)) return fem_fail_as(GADAPT_FEM_E_BADARG, who, "the Simpson rule needs an odd nlat >= 3");
    if (max_lds_bytes <= 0 || max_lds_bytes > GADAPT_FEM_LDS_BUDGET || gadapt_fem_eval_lds_bytes(max_tris) > GADAPT_FEM_LDS_BUDGET)
        return fem_fail_as(GADAPT_FEM_E_LDS, who, "band factor or triangle bin mask outside the LDS budget");
    // the lattice loss's row sums, as gadapt_fem_modular_forward refuses them in an epoch (and under its name)
    if (epochs > 0 && (int64_t)nlat * 4 > GADAPT_FEM_LDS_BUDGET)
        return fem_fail(GADAPT_FEM_E_LDS, "gadapt_fem_modular_forward: the lattice's row sums exceed the LDS budget");
    const FemBatch b = FEM_BATCH(tri_mesh, max_tris);
    const FemScratch sc{rhs, coeffs, lfac};
    const FemAdjoint adj{gc, mu, tgrad, gx};
    const FemPlan P{max_lds_bytes, gadapt_fem_eval_lds_bytes(max_tris), 0};
    hipStream_t s = (hipStream_t)stream;
    const bool wave_forward = routes & GADAPT_FEM_ROUTE_WAVE_FORWARD, wave_adjoint = routes & GADAPT_FEM_ROUTE_WAVE_ADJOINT;
    const int n_init = T > B ? T : B;
    FEM_LAUNCH(fem_descent_sign_kernel, (n_init + DESC_THREADS - 1) / DESC_THREADS, DESC_THREADS, 0, T, B, cells, x_ref ? x_ref : x, sign,
               first_tangled, min_area);
    for (int j = 0; j < epochs; ++j) {
        int rc = fem_launch_modular_forward(Band::lds, b, P, sc, GADAPT_FEM_LOSS_SIMPSON, sol, loss, g_sol, s, wave_forward);
        if (rc || (rc = fem_launch_backward(Band::lds, b, P, sc, nullptr, g_sol, adj, s, wave_adjoint))) return rc;
        FEM_LAUNCH(fem_descent_step_kernel, B, DESC_THREADS, 0, meta, cells, int_idx, sign, gx, loss, lr, j, B, N, x, loss_hist, mesh_hist,
                   first_tangled, min_area);
    }
    return GADAPT_FEM_OK;
}

#define DESCEND_ARGS                                                                                                                       \
    B, N, T, meta, cells, node_mesh, tri_mesh, int_idx, int_node, nt_ptr, nt_idx, gptr, gpar, x, x_ref, lat_x, lat_y, nlat, max_lds_bytes, \
        max_tris, epochs, lr, rhs, coeffs, lfac, sol, loss, g_sol, gc, mu, tgrad, gx, loss_hist, mesh_hist, first_tangled, min_area, sign, stream

extern "C" int gadapt_fem_descend(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                  const int32_t* tri_mesh, const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                                  const int32_t* nt_idx, const int32_t* gptr, const float* gpar, float* x, const float* x_ref,
                                  const float* lat_x, const float* lat_y, int nlat, int max_lds_bytes, int max_tris, int epochs, float lr,
                                  float* rhs, float* coeffs, float* lfac, float* sol, float* loss, float* g_sol, float* gc, float* mu,
                                  float* tgrad, float* gx, float* loss_hist, float* mesh_hist, int32_t* first_tangled, float* min_area,
                                  int8_t* sign, void* stream) {
    return descend_2d("gadapt_fem_descend", 0, DESCEND_ARGS);
}

// routes is checked first: a value with other bits set selects nothing that is built
extern "C" int gadapt_fem_descend_wave(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                       const int32_t* tri_mesh, const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                                       const int32_t* nt_idx, const int32_t* gptr, const float* gpar, float* x, const float* x_ref,
                                       const float* lat_x, const float* lat_y, int nlat, int max_lds_bytes, int max_tris, int epochs,
                                       float lr, float* rhs, float* coeffs, float* lfac, float* sol, float* loss, float* g_sol, float* gc,
                                       float* mu, float* tgrad, float* gx, float* loss_hist, float* mesh_hist, int32_t* first_tangled,
                                       float* min_area, int8_t* sign, int routes, void* stream) {
    if (routes & ~(GADAPT_FEM_ROUTE_WAVE_FORWARD | GADAPT_FEM_ROUTE_WAVE_ADJOINT))
        return fem_fail(GADAPT_FEM_E_BADARG, "gadapt_fem_descend_wave: routes takes bit 0 (wave forward) and bit 1 (wave adjoint) only");
    return descend_2d("gadapt_fem_descend_wave", routes, DESCEND_ARGS);
}
#undef DESCEND_ARGS

// ---------------------------------------------------------------------------------------------------- 1-D
// u_true is f1::gauss, the one the 1-D tail evaluates (fem1d_common.h)
// loss[b] = torch.trapezoid((sol - u_true)^2, pts) = sum_j (e_j+1^2 + e_j^2) (pts_j+1 - pts_j) / 2 (L2norm, difFEM_1d.py:82-83)
// and g_sol = d loss[b] / d sol.  Lane l adds the intervals l, l + 256, ... in that order; the lanes' sums meet in a binary tree.
__global__ void __launch_bounds__(DESC_THREADS) fem1d_l2_seed_kernel(const int32_t* __restrict__ gptr, const float* __restrict__ gpar,
                                                                     int P, const float* __restrict__ pts, const float* __restrict__ sol,
                                                                     float* __restrict__ loss, float* __restrict__ g_sol) {
    __shared__ float part[DESC_THREADS];
    const int b = blockIdx.x;
    const int g0 = gptr[b], g1 = gptr[b + 1];
    const float* s_row = sol + (int64_t)b * P;
    float* g_row = g_sol + (int64_t)b * P;
    float acc = 0.0f;
    for (int j = threadIdx.x; j < P; j += DESC_THREADS) {
        const float p = pts[j];
        const float e = s_row[j] - f1::gauss(p, gpar, g0, g1);
        const float dl = j > 0 ? p - pts[j - 1] : 0.0f, dr = j + 1 < P ? pts[j + 1] - p : 0.0f;
        g_row[j] = 2.0f * e * (0.5f * dl + 0.5f * dr);
        if (j + 1 < P) {
            const float e1 = s_row[j + 1] - f1::gauss(pts[j + 1], gpar, g0, g1);
            acc = acc + (e1 * e1 + e * e) * dr;
        }
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int h = DESC_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[b] = part[0] / 2.0f;
}

__global__ void __launch_bounds__(DESC_THREADS) fem1d_descent_init_kernel(int n_meshes, int32_t* __restrict__ first_tangled,
                                                                          float* __restrict__ min_area) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_meshes) {
        first_tangled[i] = -1;
        min_area[i] = INFINITY;
    }
}

// One lane per node.  all == 0 (mesh_params 'internal'): nodes 1..n-2 move.  all != 0: every node moves, then the mesh is
// rescaled to (x - min) / (max - min) and its ends set to 0 and 1 (difFEM_1d.py:273-279; nothing is sorted there).
// The watch is the smallest x[i+1] - x[i] of the new mesh.
__global__ void __launch_bounds__(GADAPT_FEM1D_MAX_NODES) fem1d_descent_step_kernel(
    const int32_t* __restrict__ node_off, const float* __restrict__ gx, const float* __restrict__ loss, float lr, int all, int epoch,
    int n_meshes, int n_nodes, float* __restrict__ x, float* __restrict__ loss_hist, float* __restrict__ mesh_hist,
    int32_t* __restrict__ first_tangled, float* __restrict__ min_area) {
    extern __shared__ float xs[];                                // the mesh's new nodes (f1::Layout::DESCENT_ROWS)
    __shared__ float waves[DESC_MAX_WAVES];
    const int b = blockIdx.x, i = threadIdx.x;
    const int o = node_off[b], n = node_off[b + 1] - o;
    float v = 0.0f;
    if (i < n) {
        v = x[o + i];
        if (all || (i > 0 && i < n - 1)) {
            const float p = lr * gx[o + i];
            v = v - p;
        }
    }
    if (all) {
        const float lo = block_min_nan(i < n ? v : INFINITY, waves);
        const float hi = -block_min_nan(i < n ? -v : INFINITY, waves);
        if (i < n) {
            v = (v - lo) / (hi - lo);
            if (i == 0) v = 0.0f;
            if (i == n - 1) v = 1.0f;
        }
    }
    if (i < n) {
        xs[i] = v;
        x[o + i] = v;
        if (mesh_hist) mesh_hist[(int64_t)epoch * n_nodes + o + i] = v;
    }
    __syncthreads();
    const float m = block_min_nan(i + 1 < n ? xs[i + 1] - xs[i] : INFINITY, waves);
    if (i == 0) record_epoch(b, n_meshes, epoch, m, loss, loss_hist, first_tangled, min_area);
}

extern "C" int gadapt_fem1d_descend(int n_meshes, int max_nodes, const int32_t* node_off, float* x, const int32_t* gptr, const float* gpar,
                                    int k_load, int k_stiff, int n_pts, const float* pts, int epochs, float lr, int mesh_params, int n_nodes,
                                    float* coeffs, float* sol, int32_t* flags, float* loss, float* g_sol, float* gx, float* loss_hist,
                                    float* mesh_hist, int32_t* first_tangled, float* min_area, void* stream) {
    if (n_meshes <= 0 || epochs < 0 || n_nodes <= 0 || !node_off || !x || !gptr || !gpar || !pts || n_pts < 2 || !coeffs || !sol || !flags ||
        !loss || !g_sol || !gx || !first_tangled || !min_area || (epochs > 0 && !loss_hist) ||
        (mesh_params != GADAPT_FEM1D_DESCEND_INTERNAL && mesh_params != GADAPT_FEM1D_DESCEND_ALL))
        return fem_fail(GADAPT_FEM_E_BADARG, "gadapt_fem1d_descend: null pointer, bad size or unknown mesh_params");
    if (max_nodes < 3 || max_nodes > GADAPT_FEM1D_MAX_NODES)
        return fem_fail(max_nodes > GADAPT_FEM1D_MAX_NODES ? GADAPT_FEM_E_LDS : GADAPT_FEM_E_BADARG,
                        "gadapt_fem1d_descend: 3..GADAPT_FEM1D_MAX_NODES nodes per mesh (one lane per node)");
    // the quadrature, as gadapt_fem1d_poisson_forward refuses it in an epoch (and under its name); the Poisson layout fits any
    // max_nodes that got here (fem1d_common.h)
    if (epochs > 0 && (k_load < 2 || k_stiff < 1))
        return fem_fail(GADAPT_FEM_E_BADARG, "gadapt_fem1d_poisson_forward: need load_quad_points >= 2 and stiff_quad_points >= 1");
    const Fem1dBatch b = FEM1D_BATCH(gptr, gpar, k_load, k_stiff);
    const Fem1dPlan solve = fem1d_plan(Fem1dOp::poisson, max_nodes), step = fem1d_plan(Fem1dOp::descent_step, max_nodes);
    hipStream_t s = (hipStream_t)stream;
    FEM_LAUNCH(fem1d_descent_init_kernel, (n_meshes + DESC_THREADS - 1) / DESC_THREADS, DESC_THREADS, 0, n_meshes, first_tangled, min_area);
    for (int j = 0; j < epochs; ++j) {
        if (int rc = fem1d_launch_poisson_forward(b, solve, coeffs, sol, flags, s)) return rc;
        FEM_LAUNCH(fem1d_l2_seed_kernel, n_meshes, DESC_THREADS, 0, gptr, gpar, n_pts, pts, sol, loss, g_sol);
        if (int rc = fem1d_launch_poisson_backward(b, solve, coeffs, nullptr, g_sol, gx, s)) return rc;
        FEM_LAUNCH(fem1d_descent_step_kernel, n_meshes, step.threads, (size_t)step.lds_bytes, node_off, gx, loss, lr,
                   mesh_params == GADAPT_FEM1D_DESCEND_ALL, j, n_meshes, n_nodes, x, loss_hist, mesh_hist, first_tangled, min_area);
    }
    return GADAPT_FEM_OK;
}
