// spline_kernels.hip - batched not-a-knot interpolating cubic splines (include/gadapt_fem.h, gadapt_fem1d_spline).
//
// The reference's Burgers rollout (src/utils_eval_Burgers.py:215-239, :313-315) builds scipy's UnivariateSpline(x, y, s=0)
// per outer step: FITPACK's cubic through all points with knots x[2..n-3], i.e. the C2 piecewise cubic whose third
// derivative is continuous at x[1] and x[n-2].  One workgroup per data set; x, y and the second-derivative vector M live in
// LDS as fp64 (FITPACK works in fp64 on the fp32 data it is handed, and s'' divides by h^2).
//
//   fit    rows i = 1..n-2 of  h[i-1] M[i-1] + 2 (h[i-1] + h[i]) M[i] + h[i] M[i+1] = 6 (d[i] - d[i-1]),  d[i] = (y[i+1]-y[i])/h[i],
//          with M[0] = M[1] - h[0] (M[2] - M[1]) / h[1] (and its mirror) substituted into the first and last row: a tridiagonal
//          system in M[1..n-2], strictly diagonally dominant in its end rows and weakly elsewhere.  One lane runs the Thomas
//          sweep (n <= 1024 dependent steps; cyclic reduction would trade them for 10 barriers and twice the LDS, not worth it
//          at 21..101 points); the other lanes wait at the barrier.
//   eval   one query per lane, strided: binary search for the last x[i] <= q on the LDS copy, clamped to [0, n-2] so that
//          queries outside [x[0], x[n-1]] use the end pieces (FITPACK's ext=0), then the cubic in t = q - x[i].
//
// Flagged sets (non-increasing abscissae, non-finite input, a count outside 4..max_nodes) write NaN to their own outputs
// and nothing else; no index is formed from their data.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "fem1d_common.h"
#include "fem_host.h"

#pragma clang fp contract(off)

namespace {

__global__ void spline_kernel(const int32_t* __restrict__ set_off, const float* __restrict__ x, const float* __restrict__ y,
                              const float* __restrict__ q, const int32_t* __restrict__ q_off, int Q, int deriv, int nmax,
                              float* __restrict__ out, int32_t* __restrict__ status) {
    extern __shared__ double lds[];  // f1::Layout::SPLINE_ROWS rows of nmax doubles
    double* sx = lds;                // [nmax] abscissae
    double* sy = sx + nmax;          // [nmax] ordinates
    double* sm = sy + nmax;          // [nmax] second derivatives M (the Thomas right-hand side on the way)
    double* sc = sm + nmax;          // [nmax] the sweep's upper-diagonal ratios
    static_assert(f1::Layout::SPLINE_ROWS == 4, "sx, sy, sm, sc");
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int o = set_off[b], n = set_off[b + 1] - o;
    const int64_t q0 = q_off ? (int64_t)q_off[b] : 0, o0 = q_off ? q0 : (int64_t)b * Q;
    const int nq = q_off ? q_off[b + 1] - q_off[b] : Q;

    // what is wrong with this set, as bits (1: not increasing, 2: not finite, 4: bad count), gathered over the workgroup in LDS
    __shared__ int s_bad;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    int bad = 0;
    if (n >= 4 && n <= nmax) {
        for (int i = tid; i < n; i += nt) {
            const float xi = x[o + i], yi = y[o + i];
            sx[i] = (double)xi;
            sy[i] = (double)yi;
            if (!isfinite(xi) || !isfinite(yi)) bad |= 2;
            if (i + 1 < n && !(x[o + i + 1] > xi)) bad |= 1;
        }
    } else {
        bad = 4;
    }
    if (bad) atomicOr(&s_bad, bad);
    __syncthreads();                                                // the LDS fill and the flags
    bad = s_bad;
    if (bad) {
        // a NaN makes its own comparison fail too: report it as non-finite alone
        const int st = (bad & 4) ? GADAPT_SPLINE_S_BAD_COUNT : (bad & 2) ? GADAPT_SPLINE_S_NOT_FINITE : GADAPT_SPLINE_S_NOT_INCREASING;
        if (tid == 0) status[b] = st;
        for (int j = tid; j < nq; j += nt) out[o0 + j] = nanf("");
        return;
    }

    if (tid == 0) {
        status[b] = GADAPT_SPLINE_S_OK;
        const int m = n - 2;                                        // unknowns M[1..n-2], row r <-> M[r+1]
        double cprev = 0.0, dprev = 0.0;
        for (int r = 0; r < m; ++r) {
            const int i = r + 1;
            const double hl = sx[i] - sx[i - 1], hr = sx[i + 1] - sx[i];
            const double rhs = 6.0 * ((sy[i + 1] - sy[i]) / hr - (sy[i] - sy[i - 1]) / hl);
            double lo, di, up, f;
            if (r == 0) {                                           // M[0] eliminated
                lo = 0.0; di = hl + 2.0 * hr; up = hr - hl; f = rhs * hr / (hl + hr);
            } else {
                lo = hl; di = 2.0 * (hl + hr); up = hr; f = rhs;
            }
            if (r == m - 1) {                                       // M[n-1] eliminated (for n = 4 only the second row is this one)
                lo = hl - hr; di = 2.0 * hl + hr; up = 0.0; f = rhs * hl / (hl + hr);
            }
            const double den = di - lo * cprev;
            cprev = up / den;
            dprev = (f - lo * dprev) / den;
            sc[i] = cprev;
            sm[i] = dprev;
        }
        for (int i = n - 3; i >= 1; --i) sm[i] = sm[i] - sc[i] * sm[i + 1];
        const double h0 = sx[1] - sx[0], h1 = sx[2] - sx[1];
        const double ha = sx[n - 1] - sx[n - 2], hb = sx[n - 2] - sx[n - 3];
        sm[0] = sm[1] - h0 * (sm[2] - sm[1]) / h1;
        sm[n - 1] = sm[n - 2] + ha * (sm[n - 2] - sm[n - 3]) / hb;
    }
    __syncthreads();

    for (int j = tid; j < nq; j += nt) {
        const double p = (double)q[q0 + j];
        int lo = 0, hi = n - 1;                                     // last i in [0, n-2] with x[i] <= p (0 if none)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (sx[mid] <= p) lo = mid; else hi = mid;
        }
        const double h = sx[lo + 1] - sx[lo], t = p - sx[lo];
        const double m0 = sm[lo], m1 = sm[lo + 1];
        const double c3 = (m1 - m0) / (6.0 * h);
        const double c1 = (sy[lo + 1] - sy[lo]) / h - h * (2.0 * m0 + m1) / 6.0;
        double v;
        if (deriv == 0) v = sy[lo] + t * (c1 + t * (0.5 * m0 + t * c3));
        else if (deriv == 1) v = c1 + t * (m0 + t * 3.0 * c3);
        else v = m0 + t * 6.0 * c3;
        out[o0 + j] = (float)v;                                     // a NaN query gives a NaN value, from interval 0
    }
}

}  // namespace

// Sets and queries where the FEM entry points have meshes and points: its checks are its own, in its order; the plan and the
// launch are the shared ones (fem_host.h).
extern "C" int gadapt_fem1d_spline(int n_sets, int max_nodes, const int32_t* set_off, const float* x, const float* y, int n_queries,
                                   const float* q, const int32_t* q_off, int deriv, float* out, int32_t* status, void* stream) {
    if (n_sets < 1 || !set_off || !x || !y || !q || !out || !status || n_queries < 0 || (!q_off && n_queries < 1))
        return fem_fail(GADAPT_FEM_E_BADARG, "gadapt_fem1d_spline: bad batch, pointers or query count");
    if (deriv < 0 || deriv > 2) return fem_fail(GADAPT_FEM_E_BADARG, "gadapt_fem1d_spline: deriv is 0, 1 or 2");
    if (max_nodes < 4 || max_nodes > GADAPT_FEM1D_MAX_NODES) {
        char msg[160];
        snprintf(msg, sizeof msg, "gadapt_fem1d_spline: %d points per set; 4..%d supported (the set lives in LDS)", max_nodes,
                 GADAPT_FEM1D_MAX_NODES);
        return fem_fail(max_nodes > GADAPT_FEM1D_MAX_NODES ? GADAPT_FEM_E_LDS : GADAPT_FEM_E_BADARG, msg);
    }
    const Fem1dPlan P = fem1d_plan(Fem1dOp::spline, max_nodes);
    hipStream_t s = (hipStream_t)stream;
    FEM_LAUNCH(spline_kernel, n_sets, P.threads, (size_t)P.lds_bytes, set_off, x, y, q, q_off, n_queries, deriv, max_nodes, out, status);
    return GADAPT_FEM_OK;
}
