// fem_host.h - host side of libgadapt_fem.so shared by its translation units: the error slot, and what a 2-D entry point
// (include/gadapt_fem.h) turns its positional arguments into.  It fills a FemBatch, a FemScratch and a FemAdjoint, checks them
// (check_batch, make_plan: fem_kernels.hip) and calls the launch sequences there; a sequence picks its route's kernel with an `if`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gadapt_fem.h"

int fem_fail(int code, const char* msg);   // leaves msg in gadapt_fem_last_error()'s slot and returns code
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
// from the arguments of an entry point, which carry these names in all nine; tri_mesh and max_tris where it has them, else 0
#define FEM_BATCH(tri_mesh_, max_tris_) \
    FemBatch { B, N, T, meta, cells, node_mesh, tri_mesh_, int_idx, int_node, nt_ptr, nt_idx, gptr, gpar, x, lat_x, lat_y, nlat, max_lds_bytes, max_tris_ }

// factor: lfac on Band::lds (NULL where the factor is not kept), the fp64 workspace on Band::window
struct FemScratch { float *rhs, *coeffs, *factor; };
struct FemAdjoint { float *gc, *mu, *tgrad, *gx; };
// dynamic LDS of the solve (and adjoint solve) and of the evaluation; slab: triangle ids per evaluation slab (Band::window)
struct FemPlan { int64_t solve_lds, eval_lds; int slab; };

// What the descent shares with the entry points (fem_kernels.hip), four launches each; the caller has checked everything.
// load vector, solve, evaluation to sol, lattice loss and its derivative
int fem_launch_modular_forward(Band band, const FemBatch& b, const FemPlan& P, const FemScratch& sc, int reduction, float* sol, float* loss,
                               float* g_sol, hipStream_t s);
// d L / d c, adjoint solve on the kept factor, per-triangle chain rule, per-node gather
int fem_launch_backward(Band band, const FemBatch& b, const FemPlan& P, const FemScratch& sc, const float* g_coeffs, const float* g_sol,
                        const FemAdjoint& a, hipStream_t s);
