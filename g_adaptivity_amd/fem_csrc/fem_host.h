// fem_host.h - host side of libgadapt_fem.so shared by its translation units: the error slot, and what an entry point
// (include/gadapt_fem.h) turns its positional arguments into.  A 2-D one fills a FemBatch, a FemScratch and a FemAdjoint, checks
// them (check_batch, make_plan: fem_kernels.hip) and calls the launch sequences there; a sequence picks its route's kernel with an
// `if`.  A 1-D one fills a Fem1dBatch, checks it (fem1d_check), takes its workgroup and LDS sizes from fem1d_plan (both in
// fem1d_kernels.hip, the sizes from the layouts of fem1d_common.h) and launches with FEM_LAUNCH.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gadapt_fem.h"

int fem_fail(int code, const char* msg);   // leaves msg in gadapt_fem_last_error()'s slot and returns code
int fem_fail_as(int code, const char* who, const char* what);   // the same with "<who>: <what>" as the message
int fem_launched(const char* what);        // after a launch: GADAPT_FEM_OK, or GADAPT_FEM_E_LAUNCH with "<what>: <error>" in the slot
// kernel<<<grid, block, lds, s>>>(...) on the stream `s` of the calling function, which returns fem_launched's code if that fails
#define FEM_LAUNCH(kernel, grid, block, lds, ...)                 \
    do {                                                          \
        kernel<<<grid, block, lds, s>>>(__VA_ARGS__);             \
        if (int rc_ = fem_launched(#kernel)) return rc_;          \
    } while (0)

enum class Band { lds, window };

struct FemBatch {
    int B, N, T;
    const int32_t *meta, *cells, *node_mesh, *tri_mesh, *int_idx, *int_node, *nt_ptr, *nt_idx, *gptr;
    const float *gpar, *x, *lat_x, *lat_y;
    int nlat, max_lds_bytes, max_tris;
};
// from the arguments of an entry point, which carry these names in every one; tri_mesh and max_tris where it has them, else 0
#define FEM_BATCH(tri_mesh_, max_tris_) \
    FemBatch { B, N, T, meta, cells, node_mesh, tri_mesh_, int_idx, int_node, nt_ptr, nt_idx, gptr, gpar, x, lat_x, lat_y, nlat, max_lds_bytes, max_tris_ }

// factor: lfac on Band::lds (NULL where the factor is not kept), the fp64 workspace on Band::window
struct FemScratch { float *rhs, *coeffs, *factor; };
struct FemAdjoint { float *gc, *mu, *tgrad, *gx; };
// dynamic LDS of the solve (and adjoint solve) and of the evaluation; slab: triangle ids per evaluation slab (Band::window)
struct FemPlan { int64_t solve_lds, eval_lds; int slab; };

// What the descent shares with the entry points (fem_kernels.hip), four launches each; the caller has checked everything.
// load vector, solve, evaluation to sol, lattice loss and its derivative; wave (Band::lds alone): the first as a wave per node
// and the third as a wave per chunk with two phases per point (fem_wave_fwd_kernels.hip), with the lane kernels' bits
int fem_launch_modular_forward(Band band, const FemBatch& b, const FemPlan& P, const FemScratch& sc, int reduction, float* sol, float* loss,
                               float* g_sol, hipStream_t s, bool wave = false);
// d L / d c, adjoint solve on the kept factor, per-triangle chain rule, per-node gather; wave: the first and the third as a wave
// per node and per triangle (fem_wave_grad_kernels.hip), with the lane kernels' bits
int fem_launch_backward(Band band, const FemBatch& b, const FemPlan& P, const FemScratch& sc, const float* g_coeffs, const float* g_sol,
                        const FemAdjoint& a, hipStream_t s, bool wave = false);

// ---------------------------------------------------------------------------------------------------- 1-D
// What the 1-D entry points receive under the same names; an entry point without Gaussians or quadrature leaves those 0.
struct Fem1dBatch {
    int n_meshes, max_nodes;
    const int32_t* node_off;
    const float* x;
    const int32_t* gptr;
    const float* gpar;
    int k_load, k_stiff, n_pts;
    const float* pts;
};
// from the arguments of an entry point; the Gaussians and the quadrature where it has them
#define FEM1D_BATCH(gptr_, gpar_, k_load_, k_stiff_) \
    Fem1dBatch { n_meshes, max_nodes, node_off, x, gptr_, gpar_, k_load_, k_stiff_, n_pts, pts }

enum class Fem1dOp { burgers_forward, burgers_backward, poisson, expand, spline, descent_step };
struct Fem1dPlan { int threads; int64_t lds_bytes; };
// workgroup size and dynamic LDS of one launch of `op` for meshes (or spline sets) of up to max_nodes nodes
Fem1dPlan fem1d_plan(Fem1dOp op, int max_nodes, int n_fine = 0);

// The checks of a FEM entry point `who`, in their order: batch and points, max_nodes in min_nodes..GADAPT_FEM1D_MAX_NODES, the
// quadrature (check_quadrature), then the entry point's own (`own_bad`: refused with "<who>: <own_msg>"), then the LDS budget.
int fem1d_check(const char* who, const Fem1dBatch& b, int min_nodes, bool check_quadrature, bool own_bad, const char* own_msg,
                int64_t lds_bytes);

// What the descent shares with the Poisson entry points, one launch each; the caller has checked everything.
int fem1d_launch_poisson_forward(const Fem1dBatch& b, const Fem1dPlan& P, float* coeffs, float* sol, int32_t* flags, hipStream_t s);
int fem1d_launch_poisson_backward(const Fem1dBatch& b, const Fem1dPlan& P, const float* coeffs, const float* g_coeffs, const float* g_sol,
                                  float* gx, hipStream_t s);
