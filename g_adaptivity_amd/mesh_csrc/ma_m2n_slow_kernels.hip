// ma_m2n_slow_kernels.hip - Monge-Ampere target meshes with the reference's M2N 'slow' monitor, 2-D up to 24 x 24
// (include/gadapt_mesh.h has the iteration): m = reg + alpha (u_h - u)^2 / max + beta F / max, with u_h the P1 solution of the
// Poisson problem ON THE MOVING MESH, solved again inside the launch at every monitor evaluation.
//
// ma_m2n_slow_kernel is ma_m2n_kernel (ma_kernels.hip, on the lane route of ma_iteration.h: one workgroup per mesh, one lane per
// node, phi in a register, two LDS images) with a banded Cholesky solve between its first and second phase.  The phases of one update, each ended by a barrier
// that EVERY lane of the workgroup reaches (a mixed batch launches with the largest mesh's thread count, so the waves beyond a
// small mesh's own walk the same loops: every trip count below depends on N alone, never on a lane):
//   1  the image is complete and only read: x, y, det, lambda, u, f = -(u_xx + u_yy) and F of the lane's node; x, y, u, f go to
//      the four node arrays, the wave maxima of F to row 4 of the partials
//   2  the lane of an interior node assembles its own band row of K_II and its own right-hand side from its six triangles (no
//      atomics: nobody else writes that row)
//   3  the factor sweep, two barriers a column.  First half: every lane reads the pivot p from LDS, d = sqrtf(p) (NaN unless
//      p > 0); lanes 1..w divide the column below the pivot by d and lane 0 divides b[k] by d.  Second half: lane 0 stores d,
//      the rank-1 update of the trailing w x w triangle is spread over the lanes, one (i, j) pair each (w (w + 1) / 2 <= 253
//      pairs are fewer than any mesh's own lanes; a lane finds its pair once, by index arithmetic, and keeps it in registers),
//      and lanes 1..w carry the forward substitution along: b[k+i] -= L[k+i][k] * b[k].  What is written in a half is not read in
//      it: the update reads column k (offsets i >= 1 of rows k+i) and writes offsets i - j < i.
//   4  the backward substitution, one barrier a column: every lane forms y = b[k] / d_k, lanes 1..w subtract from b[k-j]; b[k]
//      itself is left as the numerator, and the node's own lane forms c = b[r] / d_r afterwards (the same operands, the same bits)
//   5  e = c - u, E = e e, the wave maxima of E to row 5; barrier; Fmax and Emax combined in increasing wave order, m, r, the four
//      wave reductions of ma_kernel to rows 0..3; barrier; the combine, the exits and the update of ma_kernel; the next image
// 3 (N - 2)^2 + 5 barriers an update: 248 at 11 x 11, 512 at 15 x 15, 1 328 at 23 x 23.
// Every lane keeps `ok`, whether all the pivots it read from LDS were positive: the same bit in all lanes.  A failed pivot makes
// m NaN at every node, so res is NaN and the loop ends as NONCONVEX; max-reductions drop NaNs, so E alone could not carry it.
// Row 4 is written in phase 1 and read in phase 5; row 5 and rows 0..3 are written and read in phase 5, each across one barrier;
// the node arrays are written in phase 1 and last read in phase 2 (u of the lane's own node stays in a register); the band and b
// are written from phase 2 on and last read before the first barrier of phase 5.
//
// LDS (ma_host.h, slow_lds_bytes): 4 * (6*16 + 8*8 + 4 + 6 nodes + (N-2)^2 (N-1) + (N-2)^2) bytes: six rows of wave partials, the
// Gaussians' constants, Cxy, two images, four node arrays, the band and the right-hand side.  60 944 bytes at 24 x 24, below the
// 64 KB that need no raised limit.  The pair table of fem_kernels.hip is not needed: a lane has one pair.
//
// expf / logf / sqrtf are the accurate ones; no FMA contraction (Makefile and the pragma below).  The arithmetic up to F is
// ma_m2n_kernel's source, so alpha = 0 gives that kernel's bits (reg + 0 is exact).
//
// ma_m2n_slow_kernel: 111 VGPRs, no AGPRs, 106 SGPRs, no scratch, no VGPR spills; 39 SGPRs are spilled to VGPR lanes, which
// costs no memory traffic (hipcc -Rpass-analysis=kernel-resource-usage, gfx950).  __launch_bounds__(576): 9 waves a workgroup,
// at most 3 on a SIMD, which allows 168 VGPRs.
#include "ma_iteration.h"                            // and through it ma_host.h, mesh_common.h, gadapt_mesh.h

#pragma clang fp contract(off)

using namespace gadapt_ma;

namespace {

struct V2 { float x, y; };

// fem_kernels.hip's tri_geometry, term for term
__device__ __forceinline__ void tri_geometry(V2 p0, V2 p1, V2 p2, V2 r[3], float& D) {
    r[0] = V2{p1.y - p2.y, p2.x - p1.x};
    r[1] = V2{p2.y - p0.y, p0.x - p2.x};
    r[2] = V2{p0.y - p1.y, p1.x - p0.x};
    D = p0.x * (p1.y - p2.y) + p1.x * (p2.y - p0.y) + p2.x * (p0.y - p1.y);
}

// One triangle of quad (a, b) seen from its vertex l: `up` false is (v0, v1, v3), true is (v1, v2, v3) with v0 = (a, b),
// v1 = (a, b+1), v2 = (a+1, b+1), v3 = (a+1, b).  Adds the load, then the three stiffness terms in vertex order.
__device__ __forceinline__ void tri_terms(int a, int b, bool up, int l, int N, int w, int row, const float* __restrict__ xs,
                                          const float* __restrict__ ys, const float* __restrict__ us, const float* __restrict__ fs,
                                          float* __restrict__ Arow, float& bacc) {
    const int hi[3] = {a, up ? a + 1 : a, a + 1};
    const int hj[3] = {up ? b + 1 : b, b + 1, b};
    V2 p[3], r[3];
    float uu[3], ff[3], D;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int h = hi[k] * N + hj[k];
        p[k] = V2{xs[h], ys[h]};
        uu[k] = us[h];
        ff[k] = fs[h];
    }
    tri_geometry(p[0], p[1], p[2], r, D);
    const float aD = fabsf(D);
    const float inv = 1.0f / (2.0f * aD);
    bacc = bacc + (aD / 24.0f) * (ff[l] + ((ff[0] + ff[1]) + ff[2]));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float pk = (r[l].x * r[k].x + r[l].y * r[k].y) * inv;
        const bool bnd = hi[k] == 0 || hi[k] == N - 1 || hj[k] == 0 || hj[k] == N - 1;
        const int ih = (hi[k] - 1) * w + (hj[k] - 1);
        if (bnd) bacc = bacc - pk * uu[k];
        else if (ih <= row) Arow[row - ih] = Arow[row - ih] + pk;
    }
}

__global__ __launch_bounds__(SLOW_MAX_NODES) void ma_m2n_slow_kernel(const int32_t* __restrict__ desc, const float* __restrict__ gauss,
                                                               const float* __restrict__ mon, double cfl, float tol, int tol_zero,
                                                               int max_steps, float* __restrict__ xo, float* __restrict__ yo,
                                                               int32_t* __restrict__ steps_out, float* __restrict__ res_out,
                                                               int32_t* __restrict__ status_out, float* __restrict__ mon_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x;
    const int32_t* d = desc + GADAPT_MA_DESC * b;
    const int N = d[GADAPT_MA_D_N], noff = d[GADAPT_MA_D_NODE_OFF], goff = d[GADAPT_MA_D_GAUSS_OFF], ng = d[GADAPT_MA_D_GAUSS_N];
    const int nodes = N * N, nw = (nodes + 63) >> 6;     // whole waves: N <= 32 is within ma_threads' cap
    const int w = N - 2, n = w * w, ld = w + 1;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* red = lds;
    float* gc = lds + 6 * ROW;
    float* img[2] = {lds + SLOW_HEAD, lds + SLOW_HEAD + nodes};
    float* xs = lds + SLOW_HEAD + 2 * nodes;
    float* ys = xs + nodes;
    float* us = ys + nodes;
    float* fs = us + nodes;
    float* A = fs + nodes;
    float* bv = A + n * ld;

    const bool own = tid < nodes;
    const int c = own ? tid : 0;
    const int i = c / N, j = c - i * N;
    // even reflection: the neighbour beyond an edge is the one inside it
    const int rowE = (i == N - 1 ? N - 2 : i + 1) * N, rowW = (i == 0 ? 1 : i - 1) * N;
    const int jN = j == N - 1 ? N - 2 : j + 1, jS = j == 0 ? 1 : j - 1;
    const float n1 = (float)(N - 1);
    const float xi = (float)i / n1, xj = (float)j / n1;
    const float inv2h = 0.5f * n1, invh2 = n1 * n1, inv4h2 = 0.25f * invh2;   // exact: n1 <= 23
    const float wgt = ((i == 0 || i == N - 1) ? 0.5f : 1.0f) * ((j == 0 || j == N - 1) ? 0.5f : 1.0f);
    const float dt = (float)(cfl / ((double)(N - 1) * (double)(N - 1)));
    const float reg = mon[3 * b], alpha = mon[3 * b + 1], beta = mon[3 * b + 2];
    const bool inner = own && i >= 1 && i <= N - 2 && j >= 1 && j <= N - 2;
    const int row = inner ? (i - 1) * w + (j - 1) : 0;
    // this lane's pair of the rank-1 update: pairs are numbered row by row, (1,1), (2,1), (2,2), (3,1), ...
    int pi = 1, pj = tid;
    while (pj >= pi) { pj -= pi; ++pi; }
    ++pj;
    const bool has_pair = pi <= w;
    const bool sub = tid >= 1 && tid <= w;               // lanes 1..w: the column below the pivot and the substitutions

    if (tid < ng) {                                      // ng <= 8 <= the threads of any mesh
        const float* g = gauss + 4 * (int64_t)(goff + tid);
        const float q0 = g[2] * g[2], q1 = g[3] * g[3];
        float* o = gc + GAUSS_CONSTS * tid;
        o[0] = g[0], o[1] = g[1], o[2] = 1.0f / q0, o[3] = 1.0f / q1;
        o[4] = 4.0f / (q0 * q0), o[5] = 2.0f / q0, o[6] = 4.0f / (q1 * q1), o[7] = 2.0f / q1;
        if (tid == ng - 1) lds[SLOW_HEAD - 4] = (16.0f * o[2]) * o[3];   // u_xy is the LAST Gaussian's only, as in the reference
    }
    if (tid == 0 && ng == 0) lds[SLOW_HEAD - 4] = 0.0f;           // read below whatever ng is: never an unwritten word
    float phi = 0.0f, x = xi, y = xj, res = 0.0f, m = reg;
    if (own) img[0][c] = phi;
    int steps = 0, cur = 0, status;

    for (;;) {
        __syncthreads();                                 // image `cur` is complete (and, the first time, the constants)
        const float* p = img[cur];
        const float pE = p[rowE + j], pW = p[rowW + j], pN = p[i * N + jN], pS = p[i * N + jS];
        const float pEN = p[rowE + jN], pES = p[rowE + jS], pWN = p[rowW + jN], pWS = p[rowW + jS];
        x = xi + (pE - pW) * inv2h;
        y = xj + (pN - pS) * inv2h;
        const float Aa = 1.0f + ((pE - 2.0f * phi) + pW) * invh2;
        const float Bb = 1.0f + ((pN - 2.0f * phi) + pS) * invh2;
        const float Cc = (((pEN - pES) - pWN) + pWS) * inv4h2;
        const float det = Aa * Bb - Cc * Cc;
        const float lam = 0.5f * ((Aa + Bb) - sqrtf((Aa - Bb) * (Aa - Bb) + 4.0f * (Cc * Cc)));
        float uxx = 0.0f, uyy = 0.0f, dxl = 0.0f, dyl = 0.0f, gl = 0.0f, u = 0.0f;
        for (int k = 0; k < ng; ++k) {
            const float4 g0 = *reinterpret_cast<const float4*>(gc + GAUSS_CONSTS * k);
            const float4 g1 = *reinterpret_cast<const float4*>(gc + GAUSS_CONSTS * k + 4);
            const float dx = x - g0.x, dy = y - g0.y;
            const float dx2 = dx * dx, dy2 = dy * dy;
            const float g = expf(-(dx2 * g0.z) - dy2 * g0.w);
            uxx = uxx + (g1.x * dx2 - g1.y) * g;
            uyy = uyy + (g1.z * dy2 - g1.w) * g;
            u = u + g;
            dxl = dx, dyl = dy, gl = g;                  // what is left after the loop is the last Gaussian's
        }
        const float uxy = (lds[SLOW_HEAD - 4] * (dxl * dyl)) * gl;
        const float Fn = sqrtf((uxx * uxx + 2.0f * (uxy * uxy)) + uyy * uyy);
        if (own) xs[c] = x, ys[c] = y, us[c] = u, fs[c] = -(uxx + uyy);
        const float s_f = wave_max(own ? Fn : -INFINITY);
        if (lane == 0 && wave < nw) red[4 * ROW + wave] = s_f;
        __syncthreads();                                 // the node arrays and the wave maxima of F are complete

        if (inner) {                                     // the six triangles of node (i, j), in the order of their cell numbers
            float* Arow = A + row * ld;
            for (int k = 0; k < ld; ++k) Arow[k] = 0.0f;
            float bacc = 0.0f;
            tri_terms(i - 1, j, false, 2, N, w, row, xs, ys, us, fs, Arow, bacc);
            tri_terms(i, j - 1, false, 1, N, w, row, xs, ys, us, fs, Arow, bacc);
            tri_terms(i, j, false, 0, N, w, row, xs, ys, us, fs, Arow, bacc);
            tri_terms(i - 1, j - 1, true, 1, N, w, row, xs, ys, us, fs, Arow, bacc);
            tri_terms(i - 1, j, true, 2, N, w, row, xs, ys, us, fs, Arow, bacc);
            tri_terms(i, j - 1, true, 0, N, w, row, xs, ys, us, fs, Arow, bacc);
            bv[row] = bacc;
        }
        __syncthreads();                                 // K_II and b are assembled

        bool ok = true;
        for (int k = 0; k < n; ++k) {                    // factor and forward substitution; n depends on N alone
            const float pv = A[k * ld];
            const bool pos = pv > 0.0f;
            ok = ok && pos;
            const float dk = pos ? sqrtf(pv) : NAN;
            const int below = min(w, n - 1 - k);
            if (sub && tid <= below) A[(k + tid) * ld + tid] = A[(k + tid) * ld + tid] / dk;
            if (tid == 0) bv[k] = bv[k] / dk;
            __syncthreads();
            if (tid == 0) A[k * ld] = dk;
            if (has_pair && pi <= below) A[(k + pi) * ld + (pi - pj)] = A[(k + pi) * ld + (pi - pj)] - A[(k + pi) * ld + pi] * A[(k + pj) * ld + pj];
            if (sub && tid <= below) bv[k + tid] = bv[k + tid] - A[(k + tid) * ld + tid] * bv[k];
            __syncthreads();
        }
        for (int k = n - 1; k >= 0; --k) {               // backward substitution; b[k] stays the numerator
            const float yk = bv[k] / A[k * ld];
            if (sub && tid <= k) bv[k - tid] = bv[k - tid] - A[k * ld + tid] * yk;
            __syncthreads();
        }
        const float e = inner ? bv[row] / A[row * ld] - u : 0.0f;
        const float En = e * e;
        const float s_e = wave_max(own ? En : -INFINITY);
        if (lane == 0 && wave < nw) red[5 * ROW + wave] = s_e;
        __syncthreads();                                 // the wave maxima of E are complete
        float fmx = red[4 * ROW], emx = red[5 * ROW];
        for (int v = 1; v < nw; ++v) {
            fmx = fmaxf(fmx, red[4 * ROW + v]);
            emx = fmaxf(emx, red[5 * ROW + v]);
        }
        // fmx, emx and ok came from LDS to all lanes alike: a constant term is a decision of the whole mesh
        m = (reg + (emx > 0.0f ? alpha * (En / emx) : 0.0f)) + (fmx > 0.0f ? beta * (Fn / fmx) : 0.0f);
        if (!ok) m = NAN;
        const float r = logf(m * det);

        const float s_wr = wave_sum(own ? wgt * r : 0.0f);
        const float s_mx = wave_max(own ? r : -INFINITY);
        const float s_mn = wave_min(own ? r : INFINITY);
        const float s_lm = wave_min(own ? lam : INFINITY);
        if (lane == 0 && wave < nw) {
            red[wave] = s_wr, red[ROW + wave] = s_mx, red[2 * ROW + wave] = s_mn, red[3 * ROW + wave] = s_lm;
        }
        __syncthreads();
        float sum = red[0], mx = red[ROW], mn = red[2 * ROW], lmin = red[3 * ROW];
        for (int v = 1; v < nw; ++v) {
            sum = sum + red[v];
            mx = fmaxf(mx, red[ROW + v]);
            mn = fminf(mn, red[2 * ROW + v]);
            lmin = fminf(lmin, red[3 * ROW + v]);
        }
        const float rbar = sum / invh2;                  // the weights add up to (N - 1)^2
        res = fmaxf(mx - rbar, rbar - mn);               // after a failed pivot every r, so rbar and both operands, are NaN
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
        if (mon_out) mon_out[noff + c] = m;
    }
    write_status(b, tid, steps, res, status, steps_out, res_out, status_out);
}

}  // namespace

extern "C" int gadapt_ma_m2n_slow_max_side(void) { return SLOW_MAX_SIDE; }

extern "C" int64_t gadapt_ma_m2n_slow_lds_bytes(int nodes) {
    int N = 3;
    while (N * N < nodes) ++N;
    if (nodes < 9 || nodes > SLOW_MAX_NODES || N * N != nodes)
        return mesh_fail(GADAPT_MESH_E_SIZE, "gadapt_ma_m2n_slow_lds_bytes: N x N nodes, 3 <= N <= 24");
    return slow_lds_bytes(N);
}

// Everything is checked on desc_host before the one launch: the checks and codes of gadapt_ma_m2n_batch with this route's side limit.
extern "C" int gadapt_ma_m2n_slow_batch(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* gauss, const float* mon3,
                                        double cfl, double tol, int max_steps, float* x, float* y, int32_t* steps, float* residual,
                                        int32_t* status, float* monitor_out, void* stream) {
    Geometry g;
    const int rc = check_batch("gadapt_ma_m2n_slow_batch", SLOW_MAX_SIDE, BAND_IN_LDS, false, n_mesh, desc_host, desc, gauss, mon3, cfl,
                               tol, max_steps, x, y, steps, residual, status, &g);
    if (rc != GADAPT_MESH_OK) return rc;
    const float tol_f = (float)tol;
    return launch(ma_m2n_slow_kernel, n_mesh, g.threads, slow_lds_bytes(g.side), stream, desc, gauss, mon3, cfl, tol_f,
                  (int)(tol_f == 0.0f), max_steps, x, y, steps, residual, status, monitor_out);
}
