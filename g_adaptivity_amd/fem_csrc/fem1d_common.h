// fem1d_common.h - what the 1-D units of libgadapt_fem.so share (fem1d_kernels.hip, spline_kernels.hip, descent_kernels.hip):
// the one definition of each launch's dynamic-LDS layout, read by the kernels that carve it and by the host code that sizes it
// (fem1d_plan, gadapt_fem1d_lds_bytes), and the device helpers more than one unit evaluates.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gadapt_fem.h"

#pragma clang fp contract(off)

namespace f1 {

// One mesh's LDS working set (the arrays a given launch uses).
struct W1 {
    float *m, *c, *r, *cp, *Sl, *Sd, *Su, *t0, *t1, *t2, *t3;
    int n;
};

// A layout is rows of `cap` elements (the launch's node cap); the numbers below are row indices and row counts.
struct Layout {
    // W1 on fp32 rows: m, c, r, cp, Sl, Sd, Su in rows 0..6, the scratch rows t0..t3 from T0 on
    static constexpr int SL = 4, T0 = 7, W1_ROWS = 11;
    // Burgers forward: a W1 of max_nodes per row and, with a fine mesh, a second one of n_fine per row behind it
    // Burgers backward: W1's rows 0..6 (c, r, cp are u^n, g, gu there), the mass rows Ml, Md, Mu, s0..s3 (W1's scratch), gxs
    static constexpr int BWD_ML = 7, BWD_S0 = 10, BWD_GXS = 14, BWD_ROWS = 15;
    // Poisson: a W1, one spare row so that the fp64 elimination (cp, rr: two fp64 rows) starts 8-aligned, and the three fp64
    // stiffness rows of the forward over the six fp32 rows Sl..t2, which it does not use otherwise
    static constexpr int POISSON_D64 = 12, POISSON_D64_ROWS = 2, POISSON_S64 = SL, POISSON_S64_ROWS = 3;
    // The fused Poisson tail (poisson_loss_kernel): the Poisson layout and, behind its POISSON_ROWS fp32 rows, one row of n_pts
    // floats (not of the node cap): sol - target per evaluation point, then the seed d loss / d sol
    static constexpr int POISSON_ROWS = POISSON_D64 + 2 * POISSON_D64_ROWS;
    // fn_expansion: m, c.  The spline, on fp64 rows: x, y, M, the sweep's ratios.  The descent's step: the new nodes.
    static constexpr int EXPAND_ROWS = 2, SPLINE_ROWS = 4, DESCENT_ROWS = 1;

    static constexpr int64_t burgers_forward_bytes(int64_t max_nodes, int64_t n_fine) {
        return 4 * W1_ROWS * (max_nodes + (n_fine > 1 ? n_fine : 0));
    }
    static constexpr int64_t burgers_backward_bytes(int64_t max_nodes) { return 4 * BWD_ROWS * max_nodes; }
    static constexpr int64_t poisson_bytes(int64_t max_nodes) { return (4 * POISSON_D64 + 8 * POISSON_D64_ROWS) * max_nodes; }
    static constexpr int64_t poisson_loss_bytes(int64_t max_nodes, int64_t n_pts) { return poisson_bytes(max_nodes) + 4 * n_pts; }
    static constexpr int64_t expand_bytes(int64_t max_nodes) { return 4 * EXPAND_ROWS * max_nodes; }
    static constexpr int64_t spline_bytes(int64_t max_nodes) { return 8 * SPLINE_ROWS * max_nodes; }
    static constexpr int64_t descent_step_bytes(int64_t max_nodes) { return 4 * DESCENT_ROWS * max_nodes; }
};
// a row starts at 4 * row * cap bytes: 8-aligned for any cap when the row index is even
static_assert(Layout::POISSON_D64 % 2 == 0 && Layout::POISSON_S64 % 2 == 0, "the fp64 rows start 8-aligned for any node cap");
static_assert(Layout::POISSON_D64 >= Layout::W1_ROWS && Layout::POISSON_S64 + 2 * Layout::POISSON_S64_ROWS <= Layout::T0 + 3,
              "the fp64 elimination lies behind W1; the fp64 stiffness rows end with t2 (t3 is not used by the Poisson launches)");
static_assert(Layout::BWD_S0 + 4 == Layout::BWD_GXS && Layout::BWD_GXS + 1 == Layout::BWD_ROWS && Layout::BWD_ML + 3 == Layout::BWD_S0,
              "the backward's rows follow one another");
static_assert(Layout::poisson_bytes(GADAPT_FEM1D_MAX_NODES) == GADAPT_FEM_LDS_BUDGET, "the Poisson layout at the node cap is the whole budget");
static_assert(4 * Layout::POISSON_ROWS * GADAPT_FEM1D_MAX_NODES == Layout::poisson_bytes(GADAPT_FEM1D_MAX_NODES),
              "the seed row of the fused Poisson tail starts where the Poisson layout ends");
static_assert(Layout::poisson_loss_bytes(1017, 101) <= GADAPT_FEM_LDS_BUDGET && Layout::poisson_loss_bytes(1018, 101) > GADAPT_FEM_LDS_BUDGET,
              "the fused Poisson tail with its seed row: 1017 nodes at 101 evaluation points, not the node cap");
static_assert(Layout::burgers_backward_bytes(GADAPT_FEM1D_MAX_NODES) <= GADAPT_FEM_LDS_BUDGET, "the backward's rows fit at the node cap");
static_assert(Layout::spline_bytes(GADAPT_FEM1D_MAX_NODES) <= GADAPT_FEM_LDS_BUDGET, "the spline's rows fit at the node cap");

// The maker of a W1 on the rows of `cap` floats from `base`: W1 w{F1_W1_ROWS(base, cap), n}.  (The Burgers backward carves its
// own: Ml, Md, Mu lie before its scratch rows.)  A macro like FEM_BATCH, not a function: as a function, even one inlined by
// force, the Poisson forward compiles to other machine code than with the rows written out in it - the compiler merges and
// strength-reduces the row addresses in the order in which it first meets them.
#define F1_W1_ROWS(base, cap)                                                                                                   \
    (base), (base) + (cap), (base) + 2 * (cap), (base) + 3 * (cap), (base) + f1::Layout::SL * (cap),                            \
        (base) + (f1::Layout::SL + 1) * (cap), (base) + (f1::Layout::SL + 2) * (cap), (base) + f1::Layout::T0 * (cap),          \
        (base) + (f1::Layout::T0 + 1) * (cap), (base) + (f1::Layout::T0 + 2) * (cap), (base) + (f1::Layout::T0 + 3) * (cap)

// sum_g exp(-(x-c)^2/s^2)
__device__ inline float gauss(float x, const float* __restrict__ gpar, int g0, int g1) {
    float sol = 0.0f;
    for (int g = g0; g < g1; ++g) {
        const float c = gpar[2 * g], s = gpar[2 * g + 1], r = x - c;
        sol += expf(-(r * r) / (s * s));
    }
    return sol;
}

}  // namespace f1
