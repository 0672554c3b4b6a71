// fem1d_kernels.hip - differentiable 1-D P1 FEM tails (Burgers steps, Poisson) for gfx950 (include/gadapt_fem.h, 1-D part).
//
// One workgroup per mesh, one lane per node and per interval (lane i owns node i and interval [x_i, x_{i+1}]); the mesh's
// whole state lives in LDS.  Each lane integrates its interval serially over the reference's quadrature points, rows are
// assembled from the two neighbouring intervals, and lane 0 runs the tridiagonal (Thomas) solves.  The backward re-assembles
// M and A, walks the T steps backwards with the adjoint (transposed) solve, and gathers every per-interval contribution per
// node in a fixed order.  Everything is evaluated without FMA contraction: the inclusive interval tests and the quadrature
// points must round as in the fp32 reference.
#include <stdio.h>
#include "fem_common.h"
#include "fem1d_common.h"
#include "fem_host.h"

#pragma clang fp contract(off)

namespace f1 {

// torch.searchsorted(mesh, v, right=False) - 1, clamped to [0, n-1]: torch's CPU lower-bound search, literally, so that a
// non-monotone mesh gives the reference's index as well
__device__ inline int locate(const float* m, int n, float v) {
    int s = 0, e = n;
    while (s < e) {
        const int mid = s + ((e - s) >> 1);
        if (!(m[mid] >= v)) s = mid + 1;
        else e = mid;
    }
    const int i = s - 1;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

// quadrature point j of an interval starting at a with length d, k points: a + (d*j)/(k-1)
__device__ inline float qpt(float a, float d, int j, int km1) { return a + (d * (float)j) / (float)km1; }

// aux(x, a, b) = [min(a,b) <= x <= max(a,b)] (x-a)/(b-a); the indicator is returned in ind
__device__ inline float aux(float x, float a, float b, float& ind) {
    ind = (x >= fminf(a, b) ? 1.0f : 0.0f) * (x <= fmaxf(a, b) ? 1.0f : 0.0f);
    return ind * (x - a) / (b - a);
}

// phim(x, n): the reference's hat function of node n
__device__ inline float phim(const float* m, int n, int N, float x) {
    float i0, i1;
    if (n == 0) return aux(x, m[1], m[0], i0);
    if (n == N - 1) return aux(x, m[N - 2], m[N - 1], i0);
    return aux(x, m[n - 1], m[n], i0) + aux(x, m[n + 1], m[n], i1) - (x == m[n] ? 1.0f : 0.0f);
}

// w * d phim(x, n) / d (x, m[n-1], m[n], m[n+1]): g[0] gets the x part, g[1..3] the nodes n-1, n, n+1
__device__ inline void aux_grad(float x, float a, float b, float w, float& gx, float& ga, float& gb) {
    float ind;
    aux(x, a, b, ind);
    const float d = b - a, s = w * ind / d;
    gx += s;
    ga += s * (x - b) / d;
    gb -= s * (x - a) / d;
}
__device__ inline void phim_grad(const float* m, int n, int N, float x, float w, float g[4]) {
    if (n == 0) {
        aux_grad(x, m[1], m[0], w, g[0], g[3], g[2]);
    } else if (n == N - 1) {
        aux_grad(x, m[N - 2], m[N - 1], w, g[0], g[1], g[2]);
    } else {
        aux_grad(x, m[n - 1], m[n], w, g[0], g[1], g[2]);
        aux_grad(x, m[n + 1], m[n], w, g[0], g[3], g[2]);
    }
}

// fn_expansion(c, m, p): c[I] + slope[I] (p - m[I]), slope[N-1] = 0
__device__ inline float expand(const float* m, const float* c, int N, float p, int I) {
    const float s = I < N - 1 ? (c[I + 1] - c[I]) / (m[I + 1] - m[I]) : 0.0f;
    return c[I] + s * (p - m[I]);
}
// dxfn_expansion(c, m, p): c[J+1]/dx - c[J]/dx with J = min(I, N-2)
__device__ inline float dexpand(const float* m, const float* c, int N, int I) {
    const int J = I < N - 2 ? I : N - 2;
    const float dphi = 1.0f / (m[J + 1] - m[J]);
    return c[J + 1] * dphi - c[J] * dphi;
}

// gauss(x, gpar, g0, g1) = sum_g exp(-(x-c)^2/s^2): fem1d_common.h
// the reference's Poisson forcing f = sum_g -2 exp(-(x-c)^2/s^2) (s^2 - 2 (x-c)^2) / s^4 and its derivative in x
__device__ inline float forcing(float x, const float* __restrict__ gpar, int g0, int g1, float* dfdx) {
    float sol = 0.0f, ds = 0.0f;
    for (int g = g0; g < g1; ++g) {
        const float c = gpar[2 * g], s = gpar[2 * g + 1], r = x - c, s2 = s * s, s4 = s2 * s2;
        const float e = expf(-(r * r) / s2), poly = s2 - 2.0f * (r * r);
        sol += -2.0f * e * poly / s4;
        ds += -2.0f * e / s4 * (-2.0f * r * poly / s2 - 4.0f * r);
    }
    if (dfdx) *dfdx = ds;
    return sol;
}

// Compensated (Kahan) sum: the reference's trapezoids are summed pairwise by torch, so a plain running fp32 sum over the
// k points would be noisier than the reference; without FMA contraction or reassociation the compensation survives.
struct KSum {
    float s = 0.0f, c = 0.0f;
    __device__ void add(float v) {
        const float y = v - c, t = s + y;
        c = (t - s) - y;
        s = t;
    }
};

// ------------------------------------------------------------------------------------------- trapezoid per interval
// torch.trapezoid(y, xs) = sum_j (x_{j+1}-x_j)(y_j+y_{j+1}) / 2 over the interval's k points.  Z(j, x, p, pr) returns the
// integrand (p = j/(k-1) and pr = (k-1-j)/(k-1) are the reference's phis and reversed phis).
struct Phis {
    float p, pr;
};
__device__ inline Phis phis(int j, int km1) { return Phis{(float)j / (float)km1, (float)(km1 - j) / (float)km1}; }

// Backward of L = trapz(z, xs): calls B(j, x, ph, dL/dz_j) which returns dL/dz_j * dz_j/dx_j (the integrand's own x
// dependence) and accumulates the rest; the quadrature points' dependence is returned in ga (start) and gb (end).
template <class ZF, class BF>
__device__ inline void trapz_backward(float a, float d, int k, ZF Z, BF Bk, float& ga, float& gb) {
    const int km1 = k - 1;
    KSum sa, sb;
    float xm = 0.0f, zm = 0.0f;
    float x0 = qpt(a, d, 0, km1), z0 = Z(0, x0, phis(0, km1));
    for (int j = 0; j < k; ++j) {
        float xp = 0.0f, zp = 0.0f;
        if (j + 1 < k) {
            xp = qpt(a, d, j + 1, km1);
            zp = Z(j + 1, xp, phis(j + 1, km1));
        }
        const float sz = 0.5f * ((j + 1 < k ? xp : x0) - (j > 0 ? xm : x0));
        float gxj = 0.5f * ((j > 0 ? (zm + z0) : 0.0f) - (j + 1 < k ? (z0 + zp) : 0.0f));
        gxj += Bk(j, x0, phis(j, km1), sz);
        const float t = (float)j / (float)km1;
        sa.add(gxj * (1.0f - t));
        sb.add(gxj * t);
        xm = x0; zm = z0; x0 = xp; z0 = zp;
    }
    ga += sa.s;
    gb += sb.s;
}

// Four per-node accumulators of one interval i: nodes i-1, i, i+1, i+2.  Contributions to other nodes (only on folded
// meshes) are "spilled": counted here and applied by a serial pass.
struct Acc4 {
    float v[4];
    __device__ void zero() { v[0] = v[1] = v[2] = v[3] = 0.0f; }
    __device__ bool add(int slot, float w) {
        switch (slot) {
            case 0: v[0] += w; return true;
            case 1: v[1] += w; return true;
            case 2: v[2] += w; return true;
            case 3: v[3] += w; return true;
            default: return false;
        }
    }
};

// W1, one mesh's LDS working set, and F1_W1_ROWS, which carves it: fem1d_common.h

__device__ inline void thomas(const float* l, const float* d, const float* u, float* r, float* cp, int lo, int hi) {
    float c = u[lo] / d[lo];
    cp[lo] = c;
    r[lo] = r[lo] / d[lo];
    for (int i = lo + 1; i < hi; ++i) {
        const float den = d[i] - l[i] * cp[i - 1];
        cp[i] = u[i] / den;
        r[i] = (r[i] - l[i] * r[i - 1]) / den;
    }
    for (int i = hi - 2; i >= lo; --i) r[i] = r[i] - cp[i] * r[i + 1];
}
// the same with the transposed matrix: lower'[i] = u[i-1], upper'[i] = l[i+1]
__device__ inline void thomas_t(const float* l, const float* d, const float* u, float* r, float* cp, int lo, int hi) {
    cp[lo] = (lo + 1 < hi ? l[lo + 1] : 0.0f) / d[lo];
    r[lo] = r[lo] / d[lo];
    for (int i = lo + 1; i < hi; ++i) {
        const float lt = u[i - 1], ut = i + 1 < hi ? l[i + 1] : 0.0f;
        const float den = d[i] - lt * cp[i - 1];
        cp[i] = ut / den;
        r[i] = (r[i] - lt * r[i - 1]) / den;
    }
    for (int i = hi - 2; i >= lo; --i) r[i] = r[i] - cp[i] * r[i + 1];
}

// Thomas in fp64 (the Poisson system: its condition grows as N^2, and the fp32 elimination alone would be noisier than the
// reference's pivoted LU); r is read and written in fp32, the elimination runs in cp64 / r64.  transposed: solve with A^T.
__device__ inline void thomas64(const float* l, const float* d, const float* u, float* r, double* cp, double* rr, int lo, int hi,
                                bool transposed) {
    auto lo_of = [&](int i) -> double { return transposed ? u[i - 1] : l[i]; };
    auto up_of = [&](int i) -> double { return i + 1 < hi ? (transposed ? l[i + 1] : u[i]) : 0.0; };
    cp[lo] = up_of(lo) / (double)d[lo];
    rr[lo] = (double)r[lo] / (double)d[lo];
    for (int i = lo + 1; i < hi; ++i) {
        const double li = lo_of(i), den = (double)d[i] - li * cp[i - 1];
        cp[i] = up_of(i) / den;
        rr[i] = ((double)r[i] - li * rr[i - 1]) / den;
    }
    r[hi - 1] = (float)rr[hi - 1];
    for (int i = hi - 2; i >= lo; --i) {
        rr[i] = rr[i] - cp[i] * rr[i + 1];
        r[i] = (float)rr[i];
    }
}

// Mass matrix rows (build_mass_matrix with k points): interval i gives M[i+1][i], M[i+1][i+1] (weights phis) and M[i][i],
// M[i][i+1] (reversed phis); row t returned in (ml, md, mu).  Couplings beyond the neighbours (rounding-level terms at the
// interval ends, or folds) are not assembled.
__device__ inline void mass_rows(const W1& w, int k, float& ml, float& md, float& mu) {
    const int t = threadIdx.x, n = w.n;
    if (t < n - 1) {
        const float a = w.m[t], d = w.m[t + 1] - w.m[t];
        const int km1 = k - 1;
        KSum LL, LR, RL, RR;
        float xp = 0, ll = 0, lr = 0, rl = 0, rr = 0;
        for (int j = 0; j < k; ++j) {
            const float x = qpt(a, d, j, km1);
            const Phis ph = phis(j, km1);
            const float pi = phim(w.m, t, n, x), pi1 = phim(w.m, t + 1, n, x);
            const float zll = pi * ph.p, zlr = pi1 * ph.p, zrl = pi * ph.pr, zrr = pi1 * ph.pr;
            if (j > 0) {
                const float dx = x - xp;
                LL.add(dx * (ll + zll)); LR.add(dx * (lr + zlr)); RL.add(dx * (rl + zrl)); RR.add(dx * (rr + zrr));
            }
            xp = x; ll = zll; lr = zlr; rl = zrl; rr = zrr;
        }
        w.t0[t] = LL.s / 2.0f; w.t1[t] = LR.s / 2.0f; w.t2[t] = RL.s / 2.0f; w.t3[t] = RR.s / 2.0f;
    }
    __syncthreads();
    ml = md = mu = 0.0f;
    if (t < n) {
        if (t > 0) { ml = w.t0[t - 1]; md = w.t1[t - 1]; }
        if (t < n - 1) { md = md + w.t2[t]; mu = w.t3[t]; }
    }
    __syncthreads();
}

// Stiffness rows (build_stiffness_matrix, vectorised, k+1 points per interval): off_i = trapz((1/d)(-1/d)),
// A[0][0] = trapz((1/d_0)^2), A[n-1][n-1] = trapz((-1/d_{n-2})^2), interior diagonal trapz over both neighbours.
// t0[i] keeps off_i for the caller.
__device__ inline void stiff_rows(const W1& w, int k, float& al, float& ad, float& au) {
    const int t = threadIdx.x, n = w.n;
    if (t < n - 1) {
        const float a = w.m[t], d = w.m[t + 1] - w.m[t];
        const float L = 1.0f / d, R = -L, lr = L * R, ll = L * L, rr = R * R;
        float off = 0, dl = 0, dr = 0, xp = a;
        for (int j = 1; j <= k; ++j) {
            const float x = a + ((float)j * d) / (float)k, dx = x - xp;
            off += dx * (lr + lr); dl += dx * (ll + ll); dr += dx * (rr + rr);
            xp = x;
        }
        w.t0[t] = off / 2.0f; w.t1[t] = dl / 2.0f; w.t2[t] = dr / 2.0f;
    }
    __syncthreads();
    al = ad = au = 0.0f;
    if (t < n) {
        if (t > 0) al = w.t0[t - 1];
        if (t < n - 1) au = w.t0[t];
        ad = t == 0 ? w.t1[0] : (t == n - 1 ? w.t2[n - 2] : w.t1[t - 1] + w.t2[t]);
    }
    __syncthreads();
}

// fast_inner_product(mesh, F, k): row t gets (0 + left_{t-1}) + right_t, left/right the trapezoids of F with phis and
// reversed phis over the intervals.  Uses t0, t1.
template <class F>
__device__ inline float load_row(const W1& w, int k, F f) {
    const int t = threadIdx.x, n = w.n;
    if (t < n - 1) {
        const float a = w.m[t], d = w.m[t + 1] - w.m[t];
        const int km1 = k - 1;
        KSum Lf, Rf;
        float xp = 0, zl = 0, zr = 0;
        for (int j = 0; j < k; ++j) {
            const float x = qpt(a, d, j, km1);
            const Phis ph = phis(j, km1);
            const float v = f(x);
            const float l = v * ph.p, r = v * ph.pr;
            if (j > 0) {
                const float dx = x - xp;
                Lf.add(dx * (zl + l)); Rf.add(dx * (zr + r));
            }
            xp = x; zl = l; zr = r;
        }
        w.t0[t] = Lf.s / 2.0f; w.t1[t] = Rf.s / 2.0f;
    }
    __syncthreads();
    float v = 0.0f;
    if (t < n) {
        if (t > 0) v = w.t0[t - 1];
        if (t < n - 1) v = v + w.t1[t];
    }
    __syncthreads();
    return v;
}

__device__ inline void load_mesh(const W1& w, const float* __restrict__ x, int off, int fine_n) {
    const int t = threadIdx.x;
    if (t < w.n) w.m[t] = fine_n ? fem::linspace_at(0.0f, 1.0f, fine_n, t) : x[off + t];
    __syncthreads();
}

// 1 when some x[i+1] - x[i] < 0 (build_stiffness_matrix's warning)
__device__ inline int not_increasing(const W1& w) {
    const int t = threadIdx.x;
    const int bad = (t < w.n - 1 && w.m[t + 1] - w.m[t] < 0.0f) ? 1 : 0;
    return __syncthreads_or(bad);
}

// u^0: the L2 projection of amp * gauss with identity boundary rows (get_Burgers_initial_coeffs) -> w.c
__device__ void project(const W1& w, int k_proj, int k_load, float amp, const float* gpar, int g0, int g1) {
    const int t = threadIdx.x, n = w.n;
    float ml, md, mu;
    mass_rows(w, k_proj, ml, md, mu);
    const float rhs = load_row(w, k_load, [&](float x) { return amp * gauss(x, gpar, g0, g1); });
    if (t < n) {
        const bool bnd = t == 0 || t == n - 1;
        w.Sl[t] = bnd ? 0.0f : ml; w.Sd[t] = bnd ? 1.0f : md; w.Su[t] = bnd ? 0.0f : mu;
        w.r[t] = bnd ? amp * gauss(t == 0 ? 0.0f : 1.0f, gpar, g0, g1) : rhs;
    }
    __syncthreads();
    if (t == 0) thomas(w.Sl, w.Sd, w.Su, w.r, w.cp, 0, n);
    __syncthreads();
    if (t < n) w.c[t] = w.r[t];
    __syncthreads();
}

// (M + taunu A) with identity boundary rows -> Sl/Sd/Su; this lane's M row is returned
__device__ void burgers_matrix(const W1& w, int k_load, int k_stiff, float taunu, float& ml, float& md, float& mu) {
    const int t = threadIdx.x, n = w.n;
    float al, ad, au;
    mass_rows(w, k_load, ml, md, mu);
    stiff_rows(w, k_stiff, al, ad, au);
    if (t < n) {
        const bool bnd = t == 0 || t == n - 1;
        w.Sl[t] = bnd ? 0.0f : ml + taunu * al;
        w.Sd[t] = bnd ? 1.0f : md + taunu * ad;
        w.Su[t] = bnd ? 0.0f : mu + taunu * au;
    }
    __syncthreads();
}

// one step u^n (w.c) -> u^{n+1} (w.c)
__device__ void burgers_step(const W1& w, int k_load, float tau, float ml, float md, float mu, const float* bc) {
    const int t = threadIdx.x, n = w.n;
    const float* m = w.m;
    const float* c = w.c;
    const float fv = load_row(w, k_load, [&](float x) {
        const int I = locate(m, n, x);
        return expand(m, c, n, x, I) * dexpand(m, c, n, I);
    });
    if (t < n) {
        if (t == 0) w.r[0] = bc ? bc[0] : c[0];
        else if (t == n - 1) w.r[t] = bc ? bc[1] : c[t];
        else w.r[t] = ((ml * c[t - 1] + md * c[t]) + mu * c[t + 1]) - tau * fv;
    }
    __syncthreads();
    if (t == 0) thomas(w.Sl, w.Sd, w.Su, w.r, w.cp, 0, n);
    __syncthreads();
    if (t < n) w.c[t] = w.r[t];
    __syncthreads();
}

__device__ inline void evaluate(const W1& w, const float* c, int P, const float* __restrict__ pts, float* __restrict__ out) {
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
        const float v = pts[p];
        out[p] = expand(w.m, c, w.n, v, locate(w.m, w.n, v));
    }
}

// d sol / d (c_q, x_q) of node q for sol = fn_expansion(c, m, pts), weighted by g [P]; points in increasing p order
__device__ inline void eval_adjoint_node(const float* m, const float* c, int n, int q, int P, const float* __restrict__ pts,
                                         const float* __restrict__ g, float& gc, float& gx) {
    for (int p = 0; p < P; ++p) {
        const float v = pts[p];
        const int I = locate(m, n, v);
        if (I != q && I + 1 != q) continue;
        const float w = g[p];
        if (I == n - 1) {                 // slope 0: u = c[I]
            if (I == q) gc += w;
            continue;
        }
        const float dx = m[I + 1] - m[I], tt = v - m[I], s = (c[I + 1] - c[I]) / dx, f = tt / dx;
        if (I == q) {
            gc += w * (1.0f - f);
            gx += w * (s * f - s);
        } else {
            gc += w * f;
            gx -= w * s * f;
        }
    }
}

}  // namespace f1

using namespace f1;

#define F1_THREADS 1024

// ------------------------------------------------------------------------------------------------------ Burgers
__global__ void __launch_bounds__(F1_THREADS) burgers_fwd_kernel(
    const int32_t* __restrict__ node_off, const float* __restrict__ x, const float* __restrict__ u0, const float* __restrict__ bc,
    const int32_t* __restrict__ gptr, const float* __restrict__ gpar, float amp, float tau, float taunu, int k_load, int k_stiff,
    int k_proj, int k_proj_fine, int T, int nmax, int n_fine, int P, const float* __restrict__ pts, float* __restrict__ hist,
    float* __restrict__ sol, float* __restrict__ fine_sol, int32_t* __restrict__ flags) {
    extern __shared__ float lds[];
    const int b = blockIdx.x, t = threadIdx.x;
    const int off = node_off[b], n = node_off[b + 1] - off;
    const int g0 = gptr ? gptr[b] : 0, g1 = gptr ? gptr[b + 1] : 0;   // no Gaussians when u0 is given and there is no fine mesh
    const float* bcb = bc ? bc + 2 * b : nullptr;
    for (int pass = 0; pass < (n_fine > 1 ? 2 : 1); ++pass) {
        const bool fine = pass == 1;
        const int cap = fine ? n_fine : nmax;
        float* base = lds + (fine ? Layout::W1_ROWS * nmax : 0);
        const W1 w{F1_W1_ROWS(base, cap), fine ? n_fine : n};
        load_mesh(w, x, off, fine ? n_fine : 0);
        if (!fine) {
            const int bad = not_increasing(w);
            if (t == 0) flags[b] = bad ? GADAPT_FEM1D_F_NOT_INCREASING : 0;
        }
        if (!fine && u0) {
            if (t < n) w.c[t] = u0[off + t];
            __syncthreads();
        } else {
            project(w, fine ? k_proj_fine : k_proj, k_load, amp, gpar, g0, g1);
        }
        float ml, md, mu;
        burgers_matrix(w, k_load, k_stiff, taunu, ml, md, mu);
        float* h = fine ? nullptr : hist + (size_t)(T + 1) * off;
        if (h && t < n) h[t] = w.c[t];
        for (int s = 0; s < T; ++s) {
            burgers_step(w, k_load, tau, ml, md, mu, fine ? nullptr : bcb);
            if (h && t < n) h[(size_t)(s + 1) * n + t] = w.c[t];
        }
        evaluate(w, w.c, P, pts, (fine ? fine_sol : sol) + (size_t)b * P);
        __syncthreads();
    }
}

// Adjoint of one step's u u_x load for interval i: L = sum_rows w_row F_row with w = -tau lambda on interior rows.
// spill == false: node contributions i-1..i+2 go to xs (coordinates) and cs (coefficients), others raise *spilled;
// spill == true: only the others are added, to gxs and gcs (the serial pass).  Returns the quadrature points' part in ga, gb.
__device__ void flux_adjoint(const float* m, const float* c, int n, int i, int k, float wl, float wr, bool spill, Acc4& xs, Acc4& cs,
                             float* gxs, float* gcs, int* spilled, float& ga, float& gb) {
    const float a = m[i], d = m[i + 1] - m[i];
    auto put = [&](Acc4& acc, float* arr, int node, float v) {
        const int slot = node - (i - 1);
        const bool local = slot >= 0 && slot < 4;
        if (spill) {
            if (!local) arr[node] += v;
        } else if (!acc.add(slot, v)) {
            *spilled = 1;
        }
    };
    auto Z = [&](int j, float x, Phis ph) {
        const int I = locate(m, n, x);
        const float h = expand(m, c, n, x, I) * dexpand(m, c, n, I);
        return h * (wl * ph.p + wr * ph.pr);
    };
    auto Bk = [&](int j, float x, Phis ph, float sz) {
        const float sh = sz * (wl * ph.p + wr * ph.pr);
        const int I = locate(m, n, x);
        const int J = I < n - 2 ? I : n - 2;
        const float u = expand(m, c, n, x, I);
        const float dphi = 1.0f / (m[J + 1] - m[J]), dc = c[J + 1] - c[J];
        const float ux = c[J + 1] * dphi - c[J] * dphi;
        // d h = ux d u + u d ux
        const float su = sh * ux, sx = sh * u;
        float dudp = 0.0f;
        if (I < n - 1) {
            const float dx = m[I + 1] - m[I], tt = x - m[I], s = (c[I + 1] - c[I]) / dx, f = tt / dx;
            put(cs, gcs, I, su * (1.0f - f));
            put(cs, gcs, I + 1, su * f);
            put(xs, gxs, I, su * (s * f - s));
            put(xs, gxs, I + 1, -su * s * f);
            dudp = s;
        } else {
            put(cs, gcs, I, su);
        }
        put(cs, gcs, J + 1, sx * dphi);
        put(cs, gcs, J, -sx * dphi);
        put(xs, gxs, J, sx * dc * dphi * dphi);
        put(xs, gxs, J + 1, -sx * dc * dphi * dphi);
        return su * dudp;
    };
    trapz_backward(a, d, k, Z, Bk, ga, gb);
}

// LDS of the backward: m, un, g, gu (also Thomas scratch), Sl, Sd, Su, Ml, Md, Mu, s0..s3, gxs: Layout::BWD_ROWS floats per node
__global__ void __launch_bounds__(F1_THREADS) burgers_bwd_kernel(
    const int32_t* __restrict__ node_off, const float* __restrict__ x, const float* __restrict__ bc, float tau, float taunu,
    int k_load, int k_stiff, int T, int nmax, int P, const float* __restrict__ pts, const float* __restrict__ hist,
    const float* __restrict__ g_sol, const float* __restrict__ g_last, float* __restrict__ gx, float* __restrict__ gu0) {
    extern __shared__ float lds[];
    __shared__ int spilled;
    const int b = blockIdx.x, t = threadIdx.x;
    const int off = node_off[b], n = node_off[b + 1] - off;
    float* L = lds;
    // The rows are formed in increasing order: the compiler strength-reduces them in the order it meets them, and this order
    // keeps the kernel's machine code what it was when the row numbers were written out here.
    auto row = [&](int k) { return L + k * nmax; };
    float *m = row(0), *un = row(1), *g = row(2), *gu = row(3), *Sl = row(Layout::SL), *Sd = row(Layout::SL + 1), *Su = row(Layout::SL + 2);
    float *Ml = row(Layout::BWD_ML), *Md = row(Layout::BWD_ML + 1), *Mu = row(Layout::BWD_ML + 2);
    float *s0 = row(Layout::BWD_S0), *s1 = row(Layout::BWD_S0 + 1), *s2 = row(Layout::BWD_S0 + 2), *s3 = row(Layout::BWD_S0 + 3);
    float* gxs = row(Layout::BWD_GXS);
    // mass_rows / stiff_rows use t0..t3 = s0..s3 as scratch, r / cp are unused there
    W1 w{m, un, g, gu, Sl, Sd, Su, s0, s1, s2, s3, n};
    load_mesh(w, x, off, 0);
    float ml, md, mu;
    burgers_matrix(w, k_load, k_stiff, taunu, ml, md, mu);
    const float* h = hist + (size_t)(T + 1) * off;
    if (t < n) {
        Ml[t] = ml; Md[t] = md; Mu[t] = mu;
        un[t] = h[(size_t)T * n + t];
        gxs[t] = 0.0f;
    }
    if (t == 0) spilled = 0;
    __syncthreads();
    // the evaluation of u^T
    float gxn = 0.0f;
    if (t < n) {
        float gc = g_last ? g_last[off + t] : 0.0f;
        if (g_sol) eval_adjoint_node(m, un, n, t, P, pts, g_sol + (size_t)b * P, gc, gxn);
        g[t] = gc;
    }
    __syncthreads();
    Acc4 xs;
    xs.zero();
    float gml = 0, gmd = 0, gmu = 0, gal = 0, gad = 0, gau = 0;   // d L / d M and d L / d A, row t
    float gxa = 0, gxb = 0;                                         // interval t's quadrature points: nodes t, t+1
    for (int s = T - 1; s >= 0; --s) {
        // lambda = S^-T g (in place), u^n into un; u^{n+1} comes from hist
        if (t < n) un[t] = h[(size_t)s * n + t];
        if (t == 0) thomas_t(Sl, Sd, Su, g, gu, 0, n);
        __syncthreads();
        const float* u1 = h + (size_t)(s + 1) * n;
        const bool interior = t > 0 && t < n - 1;
        if (interior) {
            const float lam = g[t];
            // d L / d M = lambda (u^n - u^{n+1})^T: the difference first (u^n and u^{n+1} are close; it is exact there)
            gml += lam * (un[t - 1] - u1[t - 1]);
            gmd += lam * (un[t] - u1[t]);
            gmu += lam * (un[t + 1] - u1[t + 1]);
            gal -= taunu * (lam * u1[t - 1]);
            gad -= taunu * (lam * u1[t]);
            gau -= taunu * (lam * u1[t + 1]);
        }
        // d L / d u^n: M^T (lambda on interior rows) + the boundary rows (unless bc holds the boundary values)
        float gun = 0.0f;
        if (t < n) {
            auto wi = [&](int r) { return (r > 0 && r < n - 1) ? g[r] : 0.0f; };
            if (t > 0) gun += Mu[t - 1] * wi(t - 1);
            gun += Md[t] * wi(t);
            if (t < n - 1) gun += Ml[t + 1] * wi(t + 1);
            if ((t == 0 || t == n - 1) && !bc) gun += g[t];
        }
        // the flux term, per interval
        Acc4 cs;
        cs.zero();
        if (t < n - 1) {
            const float wl = (t + 1 < n - 1) ? -tau * g[t + 1] : 0.0f, wr = t > 0 ? -tau * g[t] : 0.0f;
            flux_adjoint(m, un, n, t, k_load, wl, wr, false, xs, cs, nullptr, nullptr, &spilled, gxa, gxb);
        }
        __syncthreads();
        if (t < n - 1) { s0[t] = cs.v[0]; s1[t] = cs.v[1]; s2[t] = cs.v[2]; s3[t] = cs.v[3]; }
        __syncthreads();
        if (t < n) {
            if (t + 1 < n - 1) gun += s0[t + 1];
            if (t < n - 1) gun += s1[t];
            if (t >= 1) gun += s2[t - 1];
            if (t >= 2) gun += s3[t - 2];
            gu[t] = gun;
        }
        __syncthreads();
        if (spilled && t == 0) {     // folded mesh: the far contributions, serially, in interval order
            Acc4 dx, dc;
            float ga = 0, gb = 0;
            for (int i = 0; i < n - 1; ++i) {
                const float wl = (i + 1 < n - 1) ? -tau * g[i + 1] : 0.0f, wr = i > 0 ? -tau * g[i] : 0.0f;
                flux_adjoint(m, un, n, i, k_load, wl, wr, true, dx, dc, gxs, gu, nullptr, ga, gb);
            }
        }
        __syncthreads();
        if (t < n) g[t] = gu[t];
        if (t == 0) spilled = 0;
        __syncthreads();
    }
    if (gu0 && t < n) gu0[off + t] = g[t];
    // d L / d M -> x: the mass trapezoids of interval t with the row weights of d L / d M
    if (t < n) { Sl[t] = gml; Sd[t] = gmd; Su[t] = gmu; }
    __syncthreads();
    if (t < n - 1) {
        const float a = m[t], d = m[t + 1] - m[t];
        const float GLL = Sl[t + 1], GLR = Sd[t + 1], GRL = Sd[t], GRR = Su[t];
        auto Z = [&](int j, float xq, Phis ph) {
            return phim(m, t, n, xq) * (GLL * ph.p + GRL * ph.pr) + phim(m, t + 1, n, xq) * (GLR * ph.p + GRR * ph.pr);
        };
        auto Bk = [&](int j, float xq, Phis ph, float sz) {
            float ga[4] = {0, 0, 0, 0}, gb[4] = {0, 0, 0, 0};
            phim_grad(m, t, n, xq, sz * (GLL * ph.p + GRL * ph.pr), ga);
            phim_grad(m, t + 1, n, xq, sz * (GLR * ph.p + GRR * ph.pr), gb);
            xs.add(0, ga[1]); xs.add(1, ga[2]); xs.add(2, ga[3]);   // nodes t-1, t, t+1
            xs.add(1, gb[1]); xs.add(2, gb[2]); xs.add(3, gb[3]);   // nodes t, t+1, t+2
            return ga[0] + gb[0];
        };
        trapz_backward(a, d, k_load, Z, Bk, gxa, gxb);
    }
    __syncthreads();
    // d L / d A -> x: A depends on the interval lengths only (off = -1/d, diagonal 1/d per neighbour); d L / d d_t
    if (t < n) { Sl[t] = gal; Sd[t] = gad; Su[t] = gau; }
    __syncthreads();
    if (t < n - 1) {
        const float d = m[t + 1] - m[t], i2 = 1.0f / (d * d);
        const float gd = (Su[t] + Sl[t + 1]) * i2 - (Sd[t] + Sd[t + 1]) * i2;
        gxa -= gd;
        gxb += gd;
        s0[t] = xs.v[0]; s1[t] = xs.v[1] + gxa; s2[t] = xs.v[2] + gxb; s3[t] = xs.v[3];
    }
    __syncthreads();
    if (t < n) {
        float v = gxn;
        if (t + 1 < n - 1) v += s0[t + 1];
        if (t < n - 1) v += s1[t];
        if (t >= 1) v += s2[t - 1];
        if (t >= 2) v += s3[t - 2];
        gx[off + t] = v + gxs[t];
    }
}

// ------------------------------------------------------------------------------------------------------ Poisson
__device__ inline void poisson_matrix(const W1& w, float& al, float& ad, float& au) {
    const int t = threadIdx.x, n = w.n;
    if (t < n) {   // A_int = -A[1:-1, 1:-1] on rows 1..n-2
        w.Sl[t] = t > 1 ? -al : 0.0f;
        w.Sd[t] = -ad;
        w.Su[t] = t < n - 2 ? -au : 0.0f;
    }
    __syncthreads();
}

// The stiffness trapezoids of stiff_rows per interval in fp64: off (A[i][i+1]), dl and dr (the interval's shares of the
// diagonals of its left and right node).
__device__ inline void stiff_intervals64(const float* m, int n, int k, double* off, double* dl, double* dr) {
    const int t = threadIdx.x;
    if (t < n - 1) {
        const double a = m[t], d = (double)m[t + 1] - (double)m[t];
        const double L = 1.0 / d, R = -L, lr = L * R, ll = L * L, rr = R * R;
        double o = 0, l = 0, r = 0, xp = a;
        for (int j = 1; j <= k; ++j) {
            const double x = a + ((double)j * d) / (double)k, dx = x - xp;
            o += dx * (lr + lr); l += dx * (ll + ll); r += dx * (rr + rr);
            xp = x;
        }
        off[t] = o / 2.0; dl[t] = l / 2.0; dr[t] = r / 2.0;
    }
    __syncthreads();
}

// Thomas in fp64 on rows 1..n-2 of -A assembled from stiff_intervals64 (l_i = -off[i-1], d_i = -(dl[i-1] + dr[i]),
// u_i = -off[i]), right-hand side r[i] plus the boundary terms bc1 off[0] (row 1) and off[n-2] bc2 (row n-2); r[1..n-2] gets
// the solution.  By one lane.
__device__ inline void thomas64_poisson(const double* off, const double* dl, const double* dr, float* r, double bc1, double bc2,
                                        double* cp, double* rr, int n) {
    const int lo = 1, hi = n - 1;
    for (int i = lo; i < hi; ++i) rr[i] = r[i];
    rr[lo] += bc1 * off[0];
    rr[hi - 1] += off[n - 2] * bc2;
    double den = -(dl[lo - 1] + dr[lo]);
    cp[lo] = (lo + 1 < hi ? -off[lo] : 0.0) / den;
    rr[lo] = rr[lo] / den;
    for (int i = lo + 1; i < hi; ++i) {
        const double li = -off[i - 1];
        den = -(dl[i - 1] + dr[i]) - li * cp[i - 1];
        cp[i] = (i + 1 < hi ? -off[i] : 0.0) / den;
        rr[i] = (rr[i] - li * rr[i - 1]) / den;
    }
    r[hi - 1] = (float)rr[hi - 1];
    for (int i = hi - 2; i >= lo; --i) {
        rr[i] = rr[i] - cp[i] * rr[i + 1];
        r[i] = (float)rr[i];
    }
}

// torch_FEM_1D's solve of mesh b by its workgroup: the working set on the launch's LDS, coefficients (BC1, interior, BC2) in w.r.
// The stiffness trapezoids are assembled in fp64.  The reference assembles them in fp32, where the diagonal fl(dl + dr) leaves
// row sums of an ulp of 2/h and the solve answers them with coefficient errors that grow as N^2: a few 1e-6 at 21 nodes (up
// to 3e-4 of an error norm, where e = sol - u_true is ~1e-3 of sol) and 1.4e-4 to 3e-4 of the coefficients at 1023 nodes,
// twice what the reference's own fp32 solve shows there.  In fp64 the coefficients are within 1e-7 of an fp64 solve; the load
// vector, boundary values and expansion stay in fp32.  The forward and the evaluation's error norms share this solve.
__device__ inline W1 poisson_solve(float* L, int b, const int32_t* __restrict__ node_off, const float* __restrict__ x,
                                   const int32_t* __restrict__ gptr, const float* __restrict__ gpar, int k_load, int k_stiff, int nmax,
                                   int32_t* __restrict__ flags) {
    const int t = threadIdx.x;
    const int off = node_off[b], n = node_off[b + 1] - off, g0 = gptr[b], g1 = gptr[b + 1];
    const W1 w{F1_W1_ROWS(L, nmax), n};
    load_mesh(w, x, off, 0);
    const int bad = not_increasing(w);
    if (t == 0) flags[b] = bad ? GADAPT_FEM1D_F_NOT_INCREASING : 0;
    double* d64 = reinterpret_cast<double*>(L + Layout::POISSON_D64 * nmax);
    const float rhs = load_row(w, k_load, [&](float xq) { return forcing(xq, gpar, g0, g1, nullptr); });   // uses t0, t1
    const float bc1 = gauss(w.m[0], gpar, g0, g1), bc2 = gauss(w.m[n - 1], gpar, g0, g1);
    if (t < n) w.r[t] = rhs;
    // three fp64 rows over the six fp32 rows Sl..t2 (Layout::POISSON_S64: 8-aligned for any nmax)
    double *o64 = reinterpret_cast<double*>(L + Layout::POISSON_S64 * nmax), *l64 = o64 + nmax, *r64 = o64 + 2 * nmax;
    stiff_intervals64(w.m, n, k_stiff, o64, l64, r64);
    if (t == 0) {
        thomas64_poisson(o64, l64, r64, w.r, bc1, bc2, d64, d64 + nmax, n);
        w.r[0] = bc1;
        w.r[n - 1] = bc2;
    }
    __syncthreads();
    return w;
}

__global__ void __launch_bounds__(F1_THREADS) poisson_fwd_kernel(
    const int32_t* __restrict__ node_off, const float* __restrict__ x, const int32_t* __restrict__ gptr, const float* __restrict__ gpar,
    int k_load, int k_stiff, int nmax, int P, const float* __restrict__ pts, float* __restrict__ coeffs, float* __restrict__ sol,
    int32_t* __restrict__ flags) {
    extern __shared__ float lds[];
    const int b = blockIdx.x, t = threadIdx.x;
    const W1 w = poisson_solve(lds, b, node_off, x, gptr, gpar, k_load, k_stiff, nmax, flags);
    if (t < w.n) coeffs[node_off[b] + t] = w.r[t];
    evaluate(w, w.r, P, pts, sol + (size_t)b * P);
}

// The Poisson forward (poisson_solve) with the reference's trapezium norms of e = sol - u_true over pts
// (evaluate_error_np) reduced in the same launch: L1 = sum_j (|e_j| + |e_j+1|) (p_j+1 - p_j) / 2, L2 = sqrt of the same sum of squares.  The first wave
// reduces: lane l takes intervals l, l + 64, ... in order and the lanes are added in a fixed butterfly, so the order does not
// depend on the workgroup's size (which follows the largest mesh of the batch).
__global__ void __launch_bounds__(F1_THREADS) poisson_err_kernel(
    const int32_t* __restrict__ node_off, const float* __restrict__ x, const int32_t* __restrict__ gptr, const float* __restrict__ gpar,
    int k_load, int k_stiff, int nmax, int P, const float* __restrict__ pts, float* __restrict__ err, int32_t* __restrict__ flags) {
    extern __shared__ float lds[];
    const int b = blockIdx.x, t = threadIdx.x;
    const W1 w = poisson_solve(lds, b, node_off, x, gptr, gpar, k_load, k_stiff, nmax, flags);
    const int g0 = gptr[b], g1 = gptr[b + 1];
    if (t >= 64) return;                              // no barrier below: the first wave reduces, whatever the workgroup's size
    float s1 = 0.0f, s2 = 0.0f;
    for (int j = t; j + 1 < P; j += 64) {
        const float p0 = pts[j], p1 = pts[j + 1];
        const float e0 = expand(w.m, w.r, w.n, p0, locate(w.m, w.n, p0)) - gauss(p0, gpar, g0, g1);
        const float e1 = expand(w.m, w.r, w.n, p1, locate(w.m, w.n, p1)) - gauss(p1, gpar, g0, g1);
        const float dx = p1 - p0;
        s1 = s1 + (fabsf(e1) + fabsf(e0)) * dx;
        s2 = s2 + (e1 * e1 + e0 * e0) * dx;
    }
    for (int o = 32; o > 0; o >>= 1) {
        s1 = s1 + __shfl_xor(s1, o, 64);
        s2 = s2 + __shfl_xor(s2, o, 64);
    }
    if (t == 0) {
        err[2 * b] = s1 / 2.0f;
        err[2 * b + 1] = sqrtf(s2 / 2.0f);
    }
}

__global__ void __launch_bounds__(F1_THREADS) poisson_bwd_kernel(
    const int32_t* __restrict__ node_off, const float* __restrict__ x, const int32_t* __restrict__ gptr, const float* __restrict__ gpar,
    int k_load, int k_stiff, int nmax, int P, const float* __restrict__ pts, const float* __restrict__ coeffs,
    const float* __restrict__ g_coeffs, const float* __restrict__ g_sol, float* __restrict__ gx) {
    extern __shared__ float lds[];
    const int b = blockIdx.x, t = threadIdx.x;
    const int off = node_off[b], n = node_off[b + 1] - off, g0 = gptr[b], g1 = gptr[b + 1];
    float* L = lds;
    const W1 w{F1_W1_ROWS(L, nmax), n};
    load_mesh(w, x, off, 0);
    if (t < n) w.c[t] = coeffs[off + t];
    float al, ad, au;
    stiff_rows(w, k_stiff, al, ad, au);
    poisson_matrix(w, al, ad, au);
    // d L / d c (the evaluation), then lambda = A_int^-T (d L / d c_int); the boundary values are detached
    float gxn = 0.0f;
    if (t < n) {
        float gc = g_coeffs ? g_coeffs[off + t] : 0.0f;
        if (g_sol) eval_adjoint_node(w.m, w.c, n, t, P, pts, g_sol + (size_t)b * P, gc, gxn);
        w.r[t] = (t == 0 || t == n - 1) ? 0.0f : gc;
    }
    __syncthreads();
    if (t == 0) {
        double* d64 = reinterpret_cast<double*>(L + Layout::POISSON_D64 * nmax);
        thomas64(w.Sl, w.Sd, w.Su, w.r, d64, d64 + nmax, 1, n - 1, true);
    }
    __syncthreads();
    const float* lam = w.r;
    const float* c = w.c;
    const float bc1 = c[0], bc2 = c[n - 1];
    float ga = 0.0f, gb = 0.0f;
    if (t < n - 1) {
        // d L / d A[i][j] = lambda_i c_j on the interior block, plus the boundary adjustments lambda_1 BC1, lambda_{n-2} BC2
        const bool ia = t > 0, ib = t + 1 < n - 1;
        float goff = (ia && ib) ? lam[t] * c[t + 1] + lam[t + 1] * c[t] : 0.0f;
        if (t == 0) goff += lam[1] * bc1;
        if (t == n - 2) goff += lam[n - 2] * bc2;
        const float gdiag = (ia ? lam[t] * c[t] : 0.0f) + (ib ? lam[t + 1] * c[t + 1] : 0.0f);
        const float d = w.m[t + 1] - w.m[t], i2 = 1.0f / (d * d);
        const float gd = goff * i2 - gdiag * i2;
        ga -= gd;
        gb += gd;
        // the load trapezoids of interval t: rows t (reversed phis) and t+1 (phis), interior rows only
        const float wl = ib ? lam[t + 1] : 0.0f, wr = ia ? lam[t] : 0.0f;
        auto Z = [&](int j, float xq, Phis ph) { return forcing(xq, gpar, g0, g1, nullptr) * (wl * ph.p + wr * ph.pr); };
        auto Bk = [&](int j, float xq, Phis ph, float sz) {
            float df;
            forcing(xq, gpar, g0, g1, &df);
            return sz * (wl * ph.p + wr * ph.pr) * df;
        };
        trapz_backward(w.m[t], d, k_load, Z, Bk, ga, gb);
        w.t0[t] = ga;
        w.t1[t] = gb;
    }
    __syncthreads();
    if (t < n) {
        float v = gxn;
        if (t < n - 1) v += w.t0[t];
        if (t > 0) v += w.t1[t - 1];
        gx[off + t] = v;
    }
}

// The 1-D pde_loss tail in one launch: poisson_solve, the loss of sol against `target` over the evaluation points and its
// derivative in the nodes (gadapt_fem_poisson1d_loss).  sol has the bits of `evaluate`, the seed d loss / d sol the expressions of
// the loss launch (loss_forward_kernel), and the backward below is poisson_bwd_kernel's statements with g_coeffs = NULL and g_sol
// this mesh's seed row in LDS (copied, not shared: that kernel's machine code stays what it is), so gx has the bits of the three
// launches.  A mesh's partial is summed by the first wave, lane l over points l, l + 64, ... and the lanes in a fixed butterfly
// (as poisson_err_kernel: the order follows P alone, not the workgroup's size); the workgroup that takes the last ticket adds the
// B partials in index order.  Barriers follow the reduction, so no lane leaves early.
__global__ void __launch_bounds__(F1_THREADS) poisson_loss_kernel(
    const int32_t* __restrict__ node_off, const float* __restrict__ x, const int32_t* __restrict__ gptr, const float* __restrict__ gpar,
    int k_load, int k_stiff, int nmax, int P, const float* __restrict__ pts, const float* __restrict__ target, int l1,
    float* __restrict__ coeffs, float* __restrict__ sol, float* __restrict__ gx, int32_t* __restrict__ flags, float* partials,
    float* __restrict__ loss, unsigned* ticket) {
    extern __shared__ float lds[];
    const int b = blockIdx.x, t = threadIdx.x;
    float* L = lds;
    const W1 w = poisson_solve(L, b, node_off, x, gptr, gpar, k_load, k_stiff, nmax, flags);
    const int off = node_off[b], n = w.n, g0 = gptr[b], g1 = gptr[b + 1];
    float* seed = L + Layout::POISSON_ROWS * nmax;                 // [P]
    const float inv = 1.0f / (float)((int64_t)gridDim.x * P);
    // The coefficients leave w.r for w.c: the backward rebuilds the fp32 stiffness rows over the forward's fp64 ones (Sl..t2) and
    // puts its right-hand side into w.r.  (poisson_solve ends with a barrier; w.c is not read by it.)
    if (t < n) {
        const float cv = w.r[t];
        coeffs[off + t] = cv;
        w.c[t] = cv;
    }
    __syncthreads();
    for (int p = t; p < P; p += blockDim.x) {
        const float v = pts[p];
        const float u = expand(w.m, w.c, n, v, locate(w.m, n, v));
        sol[(size_t)b * P + p] = u;
        seed[p] = u - target[(size_t)b * P + p];
    }
    __syncthreads();
    float part = 0.0f;
    if (t < 64) {
        for (int p = t; p < P; p += 64) {
            const float d = seed[p];
            part = part + (l1 ? fabsf(d) : d * d);
        }
        for (int o = 32; o > 0; o >>= 1) part = part + __shfl_xor(part, o, 64);
    }
    __syncthreads();                                               // the differences are read: the seed takes their place
    for (int p = t; p < P; p += blockDim.x) {
        const float d = seed[p];
        seed[p] = l1 ? (d > 0.f ? inv : (d < 0.f ? -inv : 0.f)) : 2.0f * d * inv;
    }
    __syncthreads();
    // ---- poisson_bwd_kernel from here on (the mesh and the coefficients are in w.m and w.c already)
    float al, ad, au;
    stiff_rows(w, k_stiff, al, ad, au);
    poisson_matrix(w, al, ad, au);
    float gxn = 0.0f;
    if (t < n) {
        float gc = 0.0f;
        eval_adjoint_node(w.m, w.c, n, t, P, pts, seed, gc, gxn);
        w.r[t] = (t == 0 || t == n - 1) ? 0.0f : gc;
    }
    __syncthreads();
    if (t == 0) {
        double* d64 = reinterpret_cast<double*>(L + Layout::POISSON_D64 * nmax);
        thomas64(w.Sl, w.Sd, w.Su, w.r, d64, d64 + nmax, 1, n - 1, true);
    }
    __syncthreads();
    const float* lam = w.r;
    const float* c = w.c;
    const float bc1 = c[0], bc2 = c[n - 1];
    float ga = 0.0f, gb = 0.0f;
    if (t < n - 1) {
        const bool ia = t > 0, ib = t + 1 < n - 1;
        float goff = (ia && ib) ? lam[t] * c[t + 1] + lam[t + 1] * c[t] : 0.0f;
        if (t == 0) goff += lam[1] * bc1;
        if (t == n - 2) goff += lam[n - 2] * bc2;
        const float gdiag = (ia ? lam[t] * c[t] : 0.0f) + (ib ? lam[t + 1] * c[t + 1] : 0.0f);
        const float d = w.m[t + 1] - w.m[t], i2 = 1.0f / (d * d);
        const float gd = goff * i2 - gdiag * i2;
        ga -= gd;
        gb += gd;
        const float wl = ib ? lam[t + 1] : 0.0f, wr = ia ? lam[t] : 0.0f;
        auto Z = [&](int j, float xq, Phis ph) { return forcing(xq, gpar, g0, g1, nullptr) * (wl * ph.p + wr * ph.pr); };
        auto Bk = [&](int j, float xq, Phis ph, float sz) {
            float df;
            forcing(xq, gpar, g0, g1, &df);
            return sz * (wl * ph.p + wr * ph.pr) * df;
        };
        trapz_backward(w.m[t], d, k_load, Z, Bk, ga, gb);
        w.t0[t] = ga;
        w.t1[t] = gb;
    }
    __syncthreads();
    if (t < n) {
        float v = gxn;
        if (t < n - 1) v += w.t0[t];
        if (t > 0) v += w.t1[t - 1];
        gx[off + t] = v;
    }
    // ---- the batch's loss: per-mesh partials, added in index order by the workgroup that finishes last
    if (t == 0) {
        __hip_atomic_store(partials + b, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        if (atomicAdd(ticket, 1u) == gridDim.x - 1) {
            __threadfence();
            float v = 0.0f;
            for (unsigned k = 0; k < gridDim.x; ++k) v = v + __hip_atomic_load(partials + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            loss[0] = v * inv;
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
        }
    }
}

__global__ void __launch_bounds__(F1_THREADS) expand_kernel(const int32_t* __restrict__ node_off, const float* __restrict__ x,
                                                            const float* __restrict__ c, int nmax, int P, const float* __restrict__ pts,
                                                            float* __restrict__ sol) {
    extern __shared__ float lds[];
    const int b = blockIdx.x, t = threadIdx.x;
    const int off = node_off[b], n = node_off[b + 1] - off;
    float *m = lds, *cc = lds + nmax;            // Layout::EXPAND_ROWS
    if (t < n) { m[t] = x[off + t]; cc[t] = c[off + t]; }
    __syncthreads();
    for (int p = t; p < P; p += blockDim.x) {
        const float v = pts[p];
        sol[(size_t)b * P + p] = expand(m, cc, n, v, locate(m, n, v));
    }
}

// ------------------------------------------------------------------------------------------------------ host side
// the largest of the Burgers and Poisson layouts (fem1d_common.h): what a caller that runs any of them has to find in the budget
extern "C" int64_t gadapt_fem1d_lds_bytes(int max_nodes, int n_fine) {
    const int64_t fwd = Layout::burgers_forward_bytes(max_nodes, n_fine), bwd = Layout::burgers_backward_bytes(max_nodes);
    const int64_t burgers = fwd > bwd ? fwd : bwd, poisson = Layout::poisson_bytes(max_nodes);
    return burgers > poisson ? burgers : poisson;
}

// One lane per node in whole waves; the spline takes one wave per set, four for the larger sets' fill and queries.  The Burgers
// launches are sized by gadapt_fem1d_lds_bytes, as their callers budget them.
Fem1dPlan fem1d_plan(Fem1dOp op, int max_nodes, int n_fine) {
    const int lanes = op == Fem1dOp::burgers_forward && n_fine > max_nodes ? n_fine : max_nodes;
    const int threads = lanes < 64 ? 64 : ((lanes + 63) / 64) * 64;
    switch (op) {
        case Fem1dOp::burgers_forward: return {threads, gadapt_fem1d_lds_bytes(max_nodes, n_fine)};
        case Fem1dOp::burgers_backward: return {threads, gadapt_fem1d_lds_bytes(max_nodes, 0)};
        case Fem1dOp::poisson: return {threads, Layout::poisson_bytes(max_nodes)};
        case Fem1dOp::expand: return {threads, Layout::expand_bytes(max_nodes)};
        case Fem1dOp::spline: return {max_nodes <= 256 ? 64 : 256, Layout::spline_bytes(max_nodes)};
        case Fem1dOp::descent_step: return {threads, Layout::descent_step_bytes(max_nodes)};
    }
    return {0, 0};
}

int fem1d_check(const char* who, const Fem1dBatch& b, int min_nodes, bool check_quadrature, bool own_bad, const char* own_msg,
                int64_t lds_bytes) {
    char msg[200];
    int code = GADAPT_FEM_E_BADARG;
    if (b.n_meshes < 1 || !b.node_off || !b.x || (b.n_pts > 0 && !b.pts) || b.n_pts < 0) {
        snprintf(msg, sizeof msg, "%s: bad batch, pointers or point count", who);
    } else if (b.max_nodes < min_nodes || b.max_nodes > GADAPT_FEM1D_MAX_NODES) {
        snprintf(msg, sizeof msg, "%s: %d nodes per mesh; %d..%d supported (one lane per node, state in LDS)", who, b.max_nodes, min_nodes,
                 GADAPT_FEM1D_MAX_NODES);
        if (b.max_nodes > GADAPT_FEM1D_MAX_NODES) code = GADAPT_FEM_E_LDS;
    } else if (check_quadrature && (b.k_load < 2 || b.k_stiff < 1)) {
        snprintf(msg, sizeof msg, "%s: need load_quad_points >= 2 and stiff_quad_points >= 1", who);
    } else if (own_bad) {
        snprintf(msg, sizeof msg, "%s: %s", who, own_msg);
    } else if (lds_bytes > GADAPT_FEM_LDS_BUDGET) {
        snprintf(msg, sizeof msg, "%s: needs %lld B of LDS, the budget is %d B", who, (long long)lds_bytes, GADAPT_FEM_LDS_BUDGET);
        code = GADAPT_FEM_E_LDS;
    } else {
        return GADAPT_FEM_OK;
    }
    return fem_fail(code, msg);
}

int fem1d_launch_poisson_forward(const Fem1dBatch& b, const Fem1dPlan& P, float* coeffs, float* sol, int32_t* flags, hipStream_t s) {
    FEM_LAUNCH(poisson_fwd_kernel, b.n_meshes, P.threads, (size_t)P.lds_bytes, b.node_off, b.x, b.gptr, b.gpar, b.k_load, b.k_stiff,
               b.max_nodes, b.n_pts, b.pts, coeffs, sol, flags);
    return GADAPT_FEM_OK;
}

int fem1d_launch_poisson_backward(const Fem1dBatch& b, const Fem1dPlan& P, const float* coeffs, const float* g_coeffs, const float* g_sol,
                                  float* gx, hipStream_t s) {
    FEM_LAUNCH(poisson_bwd_kernel, b.n_meshes, P.threads, (size_t)P.lds_bytes, b.node_off, b.x, b.gptr, b.gpar, b.k_load, b.k_stiff,
               b.max_nodes, b.n_pts, b.pts, coeffs, g_coeffs, g_sol, gx);
    return GADAPT_FEM_OK;
}

// Every entry point: fill the batch (the parameters carry the header's names), its own checks inside fem1d_check, the plan, launch.
extern "C" int gadapt_fem1d_burgers_forward(int n_meshes, int max_nodes, const int32_t* node_off, const float* x, const float* u0,
                                            const float* bc, const int32_t* gptr, const float* gpar, float amp, float tau, float taunu,
                                            int k_load, int k_stiff, int k_proj, int k_proj_fine, int n_steps, int n_fine, int n_pts,
                                            const float* pts, float* hist, float* sol, float* fine_sol, int32_t* flags, void* stream) {
    const Fem1dBatch b = FEM1D_BATCH(gptr, gpar, k_load, k_stiff);
    const bool own_bad = n_steps < 1 || !hist || !sol || !flags || (!u0 && (!gptr || !gpar || k_proj < 2)) ||
                         (n_fine > 1 && (!fine_sol || !gptr || !gpar || k_proj_fine < 2)) || n_fine > GADAPT_FEM1D_MAX_NODES;
    const Fem1dPlan P = fem1d_plan(Fem1dOp::burgers_forward, max_nodes, n_fine);
    if (int rc = fem1d_check("gadapt_fem1d_burgers_forward", b, 2, true, own_bad, "bad steps, pointers, projection or fine mesh", P.lds_bytes))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    FEM_LAUNCH(burgers_fwd_kernel, n_meshes, P.threads, (size_t)P.lds_bytes, node_off, x, u0, bc, gptr, gpar, amp, tau, taunu, k_load, k_stiff,
               k_proj, k_proj_fine, n_steps, max_nodes, n_fine, n_pts, pts, hist, sol, fine_sol, flags);
    return GADAPT_FEM_OK;
}

extern "C" int gadapt_fem1d_burgers_backward(int n_meshes, int max_nodes, const int32_t* node_off, const float* x, const float* bc, float tau,
                                             float taunu, int k_load, int k_stiff, int n_steps, int n_pts, const float* pts,
                                             const float* hist, const float* g_sol, const float* g_last, float* gx, float* gu0,
                                             void* stream) {
    const Fem1dBatch b = FEM1D_BATCH(nullptr, nullptr, k_load, k_stiff);
    const Fem1dPlan P = fem1d_plan(Fem1dOp::burgers_backward, max_nodes);
    if (int rc = fem1d_check("gadapt_fem1d_burgers_backward", b, 2, true, n_steps < 1 || !hist || !gx, "bad steps or pointers", P.lds_bytes))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    FEM_LAUNCH(burgers_bwd_kernel, n_meshes, P.threads, (size_t)P.lds_bytes, node_off, x, bc, tau, taunu, k_load, k_stiff, n_steps, max_nodes,
               n_pts, pts, hist, g_sol, g_last, gx, gu0);
    return GADAPT_FEM_OK;
}

extern "C" int gadapt_fem1d_poisson_forward(int n_meshes, int max_nodes, const int32_t* node_off, const float* x, const int32_t* gptr,
                                            const float* gpar, int k_load, int k_stiff, int n_pts, const float* pts, float* coeffs,
                                            float* sol, int32_t* flags, void* stream) {
    const Fem1dBatch b = FEM1D_BATCH(gptr, gpar, k_load, k_stiff);
    const Fem1dPlan P = fem1d_plan(Fem1dOp::poisson, max_nodes);
    if (int rc = fem1d_check("gadapt_fem1d_poisson_forward", b, 3, true, !gptr || !gpar || !coeffs || !sol || !flags, "null pointer", P.lds_bytes))
        return rc;
    return fem1d_launch_poisson_forward(b, P, coeffs, sol, flags, (hipStream_t)stream);
}

extern "C" int gadapt_fem1d_poisson_eval_errors(int n_meshes, int max_nodes, const int32_t* node_off, const float* x, const int32_t* gptr,
                                                const float* gpar, int k_load, int k_stiff, int n_pts, const float* pts, float* err,
                                                int32_t* flags, void* stream) {
    const Fem1dBatch b = FEM1D_BATCH(gptr, gpar, k_load, k_stiff);
    const Fem1dPlan P = fem1d_plan(Fem1dOp::poisson, max_nodes);
    if (int rc = fem1d_check("gadapt_fem1d_poisson_eval_errors", b, 3, true, !gptr || !gpar || !err || !flags || n_pts < 2,
                             "null pointer or fewer than 2 evaluation points", P.lds_bytes))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    FEM_LAUNCH(poisson_err_kernel, n_meshes, P.threads, (size_t)P.lds_bytes, node_off, x, gptr, gpar, k_load, k_stiff, max_nodes, n_pts, pts, err,
               flags);
    return GADAPT_FEM_OK;
}

extern "C" int gadapt_fem1d_poisson_backward(int n_meshes, int max_nodes, const int32_t* node_off, const float* x, const int32_t* gptr,
                                             const float* gpar, int k_load, int k_stiff, int n_pts, const float* pts, const float* coeffs,
                                             const float* g_coeffs, const float* g_sol, float* gx, void* stream) {
    const Fem1dBatch b = FEM1D_BATCH(gptr, gpar, k_load, k_stiff);
    const Fem1dPlan P = fem1d_plan(Fem1dOp::poisson, max_nodes);
    if (int rc = fem1d_check("gadapt_fem1d_poisson_backward", b, 3, true, !gptr || !gpar || !coeffs || !gx, "null pointer", P.lds_bytes))
        return rc;
    return fem1d_launch_poisson_backward(b, P, coeffs, g_coeffs, g_sol, gx, (hipStream_t)stream);
}

extern "C" int64_t gadapt_fem_poisson1d_loss_lds_bytes(int max_nodes, int n_pts) { return Layout::poisson_loss_bytes(max_nodes, n_pts); }

// The Poisson launches' workgroup; the LDS is the Poisson layout's and the seed row's, so the node cap of this entry point lies
// below GADAPT_FEM1D_MAX_NODES (1017 at 101 points) and the budget check is what refuses the sizes between.
extern "C" int gadapt_fem_poisson1d_loss(int n_meshes, int max_nodes, const int32_t* node_off, const float* x, const int32_t* gptr,
                                         const float* gpar, int k_load, int k_stiff, int n_pts, const float* pts, const float* target,
                                         int loss_kind, float* coeffs, float* sol, float* gx, int32_t* flags, float* partials, float* loss,
                                         int32_t* ticket, void* stream) {
    const Fem1dBatch b = FEM1D_BATCH(gptr, gpar, k_load, k_stiff);
    Fem1dPlan P = fem1d_plan(Fem1dOp::poisson, max_nodes);
    P.lds_bytes = Layout::poisson_loss_bytes(max_nodes, n_pts);
    const bool own_bad = !gptr || !gpar || !target || !coeffs || !sol || !gx || !flags || !partials || !loss || !ticket || n_pts < 1 ||
                         (loss_kind != GADAPT_FEM1D_LOSS_L1 && loss_kind != GADAPT_FEM1D_LOSS_MSE);
    if (int rc = fem1d_check("gadapt_fem_poisson1d_loss", b, 3, true, own_bad, "null pointer, no evaluation points or unknown loss_kind",
                             P.lds_bytes))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    FEM_LAUNCH(poisson_loss_kernel, n_meshes, P.threads, (size_t)P.lds_bytes, node_off, x, gptr, gpar, k_load, k_stiff, max_nodes, n_pts, pts,
               target, loss_kind == GADAPT_FEM1D_LOSS_L1 ? 1 : 0, coeffs, sol, gx, flags, partials, loss, reinterpret_cast<unsigned*>(ticket));
    return GADAPT_FEM_OK;
}

extern "C" int gadapt_fem1d_expand(int n_meshes, int max_nodes, const int32_t* node_off, const float* x, const float* c, int n_pts,
                                   const float* pts, float* sol, void* stream) {
    const Fem1dBatch b = FEM1D_BATCH(nullptr, nullptr, 0, 0);
    const Fem1dPlan P = fem1d_plan(Fem1dOp::expand, max_nodes);
    if (int rc = fem1d_check("gadapt_fem1d_expand", b, 2, false, !c || !sol, "null pointer", P.lds_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    FEM_LAUNCH(expand_kernel, n_meshes, P.threads, (size_t)P.lds_bytes, node_off, x, c, max_nodes, n_pts, pts, sol);
    return GADAPT_FEM_OK;
}
