// fem_common.h - device helpers of the P1 FEM tail (include/gadapt_fem.h): the reference's hat function and its derivative.
//
// Everything here is evaluated WITHOUT FMA contraction (also -ffp-contract=off in the Makefile): the inclusive edge test of
// difFEM_2d.py:16-23 classifies points on element edges - which the Simpson boxes and the evaluation lattice hit on every
// unmoved mesh - by comparing two rounded sums, and a contracted evaluation classifies some of them differently from the
// fp32 reference.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gadapt_fem.h"

#pragma clang fp contract(off)

// Points per dimension of the load-vector rule.  The reference integrates with torchquad's
// Simpson().integrate(N=load_quad_points=101, dim=2) (difFEM_2d.py:320-325).  Simpson._adjust_N takes
// floor(101^(1/2)) = 10 points per dimension and lowers an even count by one (the composite rule needs an odd count):
// 9 x 9 points, torch.linspace per dimension, weights h/3 [1,4,2,...,4,1] in tensor product.
#define FEM_SIMPSON_N GADAPT_FEM_SIMPSON_N

namespace fem {

struct V2 { float x, y; };

__device__ inline V2 ld2(const float* __restrict__ x, int v) { return V2{x[2 * v], x[2 * v + 1]}; }

// checkleft / checkright of the directed edge (p,q) at point (x0,x1) (difFEM_2d.py:16-20), operation order as written there
__device__ inline void edge_test(float x0, float x1, V2 p, V2 q, float& left, float& right) {
    const float u = p.y - q.y, v = q.x - p.x;
    const float lhs = u * x0 + v * x1;
    const float rhs = u * p.x + v * p.y;
    left = lhs >= rhs ? 1.0f : 0.0f;
    right = lhs <= rhs ? 1.0f : 0.0f;
}

// the indicator factor of aux(x, a, b, c) (difFEM_2d.py:25-26): 1 inside or on the triangle (2 only if degenerate), else 0.
// The same three directed edges appear for every rotation (a,b,c) of one triangle, so the value does not depend on which
// vertex is c.
__device__ inline float inside(float x0, float x1, V2 a, V2 b, V2 c) {
    float l1, r1, l2, r2, l3, r3;
    edge_test(x0, x1, a, b, l1, r1);
    edge_test(x0, x1, b, c, l2, r2);
    edge_test(x0, x1, c, a, l3, r3);
    return l1 * l2 * l3 + r1 * r2 * r3;
}

// aux(x, a, b, c) given its indicator: ind * (1 + num / den)
__device__ inline float aux_value(float x0, float x1, V2 a, V2 b, V2 c, float ind) {
    const float num = (x0 - c.x) * (a.y - b.y) + (x1 - c.y) * (b.x - a.x);
    const float den = (a.y - b.y) * (c.x - a.x) + (c.y - a.y) * (b.x - a.x);
    return ind * (1.0f + num / den);
}

// w * d aux / d (a, b, c) with the indicator held constant (it is a step function: no gradient)
__device__ inline void aux_grad(float x0, float x1, V2 a, V2 b, V2 c, float w, V2& ga, V2& gb, V2& gc) {
    const float u = a.y - b.y, v = b.x - a.x;
    const float num = (x0 - c.x) * u + (x1 - c.y) * v;
    const float den = u * (c.x - a.x) + (c.y - a.y) * v;
    const float q = num / den, s = w / den;
    ga.x += s * (-(x1 - c.y) - q * (b.y - c.y));
    ga.y += s * ((x0 - c.x) - q * (c.x - b.x));
    gb.x += s * ((x1 - c.y) - q * (c.y - a.y));
    gb.y += s * (-(x0 - c.x) + q * (c.x - a.x));
    gc.x += s * (-u - q * u);
    gc.y += s * (-v - q * v);
}

// rotation of difFEM_2d.py:44-47: c = node, a = cell[(l-1) mod 3], b = cell[(l-2) mod 3]
__device__ inline void rotation(const int32_t* __restrict__ cells, int t, int l, int& va, int& vb, int& vc) {
    vc = cells[3 * t + l];
    va = cells[3 * t + (l + 2) % 3];
    vb = cells[3 * t + (l + 1) % 3];
}

// phim(x, m) = output / (repeat, or 1 if repeat == 0) (difFEM_2d.py:28-61): returns that divisor; *out gets output
__device__ inline float phim_parts(float x0, float x1, int m, const int32_t* __restrict__ nt_ptr, const int32_t* __restrict__ nt_idx,
                                   const int32_t* __restrict__ cells, const float* __restrict__ x, float* out) {
    float o = 0.0f, rep = 0.0f;
    for (int e = nt_ptr[m]; e < nt_ptr[m + 1]; ++e) {
        const int t = nt_idx[e] >> 2, l = nt_idx[e] & 3;
        int va, vb, vc;
        rotation(cells, t, l, va, vb, vc);
        const V2 a = ld2(x, va), b = ld2(x, vb), c = ld2(x, vc);
        const float inc = aux_value(x0, x1, a, b, c, inside(x0, x1, a, b, c));
        o = o + inc;
        rep = rep + (inc > 0.0f ? 1.0f : 0.0f);
    }
    if (out) *out = o;
    return rep + (rep == 0.0f ? 1.0f : 0.0f);
}

// torch.linspace(lo, hi, n)[i] as the CPU kernel computes it: from the start below n/2, from the end above
__device__ inline float linspace_at(float lo, float hi, int n, int i) {
    const float step = (hi - lo) / (float)(n - 1);
    return i < n / 2 ? lo + step * (float)i : hi - step * (float)(n - 1 - i);
}

// composite Simpson coefficient of point i of n: 1, 4, 2, 4, ..., 4, 1
__device__ inline float simpson_coef(int i, int n) {
    return (i == 0 || i == n - 1) ? 1.0f : ((i & 1) ? 4.0f : 2.0f);
}

// f = Laplace(u_true) of the Gaussians [g0, g1) (difFEM_2d.py:260-265, term order as written there)
__device__ inline float forcing(float x0, float x1, const float* __restrict__ gpar, int g0, int g1) {
    float sol = 0.0f;
    for (int g = g0; g < g1; ++g) {
        const float c0 = gpar[4 * g], c1 = gpar[4 * g + 1], s0 = gpar[4 * g + 2], s1 = gpar[4 * g + 3];
        const float s02 = s0 * s0, s12 = s1 * s1, s04 = s02 * s02, s14 = s12 * s12;
        const float d0 = c0 - x0, d1 = c1 - x1;
        const float e = expf(-(d0 * d0 / s02) - d1 * d1 / s12);
        const float poly = 4.0f * (c1 * c1) * s04 - 2.0f * s02 * s14 + 4.0f * s14 * (d0 * d0) - 8.0f * c1 * s04 * x1
                           - 2.0f * s04 * (s12 - 2.0f * (x1 * x1));
        sol += (1.0f / (s04 * s14)) * e * poly;
    }
    return sol;
}

// u_true (difFEM_2d.py:268-277)
__device__ inline float u_true(float x0, float x1, const float* __restrict__ gpar, int g0, int g1) {
    float sol = 0.0f;
    for (int g = g0; g < g1; ++g) {
        const float c0 = gpar[4 * g], c1 = gpar[4 * g + 1], s0 = gpar[4 * g + 2], s1 = gpar[4 * g + 3];
        const float d0 = x0 - c0, d1 = x1 - c1;
        sol += expf(-(d0 * d0) / (s0 * s0) - (d1 * d1) / (s1 * s1));
    }
    return sol;
}

}  // namespace fem
