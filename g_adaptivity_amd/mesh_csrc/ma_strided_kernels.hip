// ma_strided_kernels.hip - batched Monge-Ampere target meshes up to 81 x 81 with an fp64 potential (route='strided';
// include/gadapt_mesh.h has the arithmetic, ma_iteration.h the route: ownership, the fp64 image, the slot walk, the update and
// the epilogue, and why no lane decides an exit from its own value).
//
// ma_strided_kernel: two barriers a step.  Between the first and the second the image is only read: a lane walks its slots,
// forms r of each and keeps the K residuals r[k] in registers, and its partial sums go through the DPP wave reductions to LDS.
// After the second barrier every lane combines the wave partials in increasing wave order; then the exits and the update.
// 70 VGPRs, no AGPRs, 95 SGPRs, no scratch, no spills (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), one instance for
// every K; times and the parity table in docs/measurements.md.
//
// ma_m2n_strided_kernel is the same route with the reference's M2N 'fast' monitor, m = reg + beta F / Fmax with Fmax the maximum
// of F over the mesh's nodes at this step.  Three barriers a step:
//   first -> second   the image is complete and only read: the slot walk forms det, lambda and F of each slot.  F[k] and det[k]
//                     (det itself, not its logarithm: r = logf(m det) stays the header's operation) replace r[k] as the per-slot
//                     state across the second barrier; a lane folds min lambda and, from -inf, max F over its slots in
//                     increasing k.  The wave maxima of F go to row 4 of the partials.
//   second -> third   every lane combines row 4, then a second walk over its slots (again a real loop, one copy of the inlined
//                     logf: F[k] and det[k] are read and r[k] written through select chains; the walk unrolled seven times with
//                     a branch per slot spilled 16 SGPRs) forms m and r[k] and accumulates sum w r, max r and min r; with the min
//                     lambda folded before, they go through the wave
//                     reductions to rows 0..3.
//   after the third   the exits and the update of ma_strided_kernel; the image is written.
// The choice between beta F / Fmax and 0 is made on the Fmax read from LDS.
// ma_m2n_strided_kernel: 80 VGPRs, no AGPRs, 101 SGPRs, no scratch, no spills (the same report), one instance for every K.
#include "ma_iteration.h"                            // and through it ma_host.h, mesh_common.h, gadapt_mesh.h

#pragma clang fp contract(off)

using namespace gadapt_ma;

namespace {

__global__ __launch_bounds__(MAX_THREADS) void ma_strided_kernel(const int32_t* __restrict__ desc, const float* __restrict__ gauss,
                                                                const float* __restrict__ mon, double cfl, float tol, int tol_zero,
                                                                int max_steps, float* __restrict__ xo, float* __restrict__ yo,
                                                                int32_t* __restrict__ steps_out, float* __restrict__ res_out,
                                                                int32_t* __restrict__ status_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int b = blockIdx.x;
    const int32_t* d = desc + GADAPT_MA_DESC * b;
    const int N = d[GADAPT_MA_D_N], noff = d[GADAPT_MA_D_NODE_OFF], goff = d[GADAPT_MA_D_GAUSS_OFF], ng = d[GADAPT_MA_D_GAUSS_N];
    const int nodes = N * N, T = ma_threads(nodes), nw = T >> 6, K = (nodes + T - 1) / T;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* red = reinterpret_cast<float*>(lds);
    float* gc = red + 4 * ROW;
    double* img = reinterpret_cast<double*>(lds + 4 * MA_HEAD);

    const bool mine = tid < T;                           // a launch has the threads of its largest mesh
    const float n1 = (float)(N - 1), rN = 1.0f / (float)N;
    const double n1d = (double)(N - 1);
    const double inv2h = 0.5 * n1d, invh2 = n1d * n1d, inv4h2 = 0.25 * invh2;   // exact
    const float invh2f = n1 * n1;                                               // exact: n1 <= 80
    const float dt = (float)(cfl / invh2);
    const float reg = mon[2 * b], power = mon[2 * b + 1];

    if (tid < ng) {                                      // ng <= 8 <= the threads of any mesh
        const float* g = gauss + 4 * (int64_t)(goff + tid);
        const float q0 = g[2] * g[2], q1 = g[3] * g[3];
        float* o = gc + GAUSS_CONSTS * tid;
        o[0] = g[0], o[1] = g[1], o[2] = 1.0f / q0, o[3] = 1.0f / q1;
        o[4] = 4.0f / (q0 * q0), o[5] = 2.0f / q0, o[6] = 4.0f / (q1 * q1), o[7] = 2.0f / q1;
    }
    for (int k = 0; k < K; ++k) {
        const int idx = tid + k * T;
        if (mine && idx < nodes) img[idx] = 0.0;
    }
    float r[MAX_K];
#pragma unroll
    for (int q = 0; q < MAX_K; ++q) r[q] = 0.0f;
    float res = 0.0f;
    int steps = 0, status;

    for (;;) {
        __syncthreads();                                 // the image is complete (and, the first time, the constants)
        float a_wr = 0.0f, a_mx = -INFINITY, a_mn = INFINITY, a_lm = INFINITY;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const int idx = tid + k * T;
            const bool own = mine && idx < nodes;
            const Stencil s = stencil_of(own ? idx : 0, N, rN);
            const float wgt = ((s.i == 0 || s.i == N - 1) ? 0.5f : 1.0f) * ((s.j == 0 || s.j == N - 1) ? 0.5f : 1.0f);
            const double p0 = img[s.c];
            const double pE = img[s.rowE + s.j], pW = img[s.rowW + s.j], pN = img[s.row + s.jN], pS = img[s.row + s.jS];
            float x, y;
            moved_node(s, pE, pW, pN, pS, n1, inv2h, x, y);
            const double pEN = img[s.rowE + s.jN], pES = img[s.rowE + s.jS], pWN = img[s.rowW + s.jN], pWS = img[s.rowW + s.jS];
            const float A = (float)(1.0 + ((pE - 2.0 * p0) + pW) * invh2);
            const float B = (float)(1.0 + ((pN - 2.0 * p0) + pS) * invh2);
            const float Cc = (float)((((pEN - pES) - pWN) + pWS) * inv4h2);
            const float det = A * B - Cc * Cc;
            const float lam = 0.5f * ((A + B) - sqrtf((A - B) * (A - B) + 4.0f * (Cc * Cc)));
            float uxx = 0.0f, uyy = 0.0f;
#pragma unroll 1
            for (int g = 0; g < ng; ++g) {
                const float4 g0 = *reinterpret_cast<const float4*>(gc + GAUSS_CONSTS * g);
                const float4 g1 = *reinterpret_cast<const float4*>(gc + GAUSS_CONSTS * g + 4);
                const float dx = x - g0.x, dy = y - g0.y;
                const float dx2 = dx * dx, dy2 = dy * dy;
                const float e = expf(-(dx2 * g0.z) - dy2 * g0.w);
                uxx = uxx + (g1.x * dx2 - g1.y) * e;
                uyy = uyy + (g1.z * dy2 - g1.w) * e;
            }
            const float m = powf(reg + sqrtf(uxx * uxx + uyy * uyy), power);
            const float rv = logf(m * det);
            // a lane's own slots in increasing k; a slot without a node gives 0, -inf, +inf, +inf
            a_wr = a_wr + (own ? wgt * rv : 0.0f);
            a_mx = fmaxf(a_mx, own ? rv : -INFINITY);
            a_mn = fminf(a_mn, own ? rv : INFINITY);
            a_lm = fminf(a_lm, own ? lam : INFINITY);
#pragma unroll
            for (int q = 0; q < MAX_K; ++q) r[q] = q == k ? rv : r[q];
        }
        const float s_wr = wave_sum(a_wr);
        const float s_mx = wave_max(a_mx);
        const float s_mn = wave_min(a_mn);
        const float s_lm = wave_min(a_lm);
        if (lane == 0 && wave < nw) {
            red[wave] = s_wr, red[ROW + wave] = s_mx, red[2 * ROW + wave] = s_mn, red[3 * ROW + wave] = s_lm;
        }
        __syncthreads();
        float sum = red[0], mx = red[ROW], mn = red[2 * ROW], lmin = red[3 * ROW];
        for (int w = 1; w < nw; ++w) {
            sum = sum + red[w];
            mx = fmaxf(mx, red[ROW + w]);
            mn = fminf(mn, red[2 * ROW + w]);
            lmin = fminf(lmin, red[3 * ROW + w]);
        }
        const float rbar = sum / invh2f;                 // the weights add up to (N - 1)^2
        res = fmaxf(mx - rbar, rbar - mn);
        // every value below was read from LDS by all lanes alike; written so that a NaN ends the loop
        if (!(lmin > 0.0f) || !(res - res == 0.0f)) { status = GADAPT_MA_NONCONVEX; break; }
        if (!tol_zero && res <= tol) { status = GADAPT_MA_CONVERGED; break; }
        if (steps >= max_steps) { status = GADAPT_MA_CAP; break; }
        const float dtl = dt * fminf(1.0f, lmin);
#pragma unroll
        for (int q = 0; q < MAX_K; ++q) {                // own nodes only: nobody reads them before the next barrier
            const int idx = tid + q * T;
            if (q < K && mine && idx < nodes) img[idx] = img[idx] + (double)(dtl * (r[q] - rbar));
        }
        ++steps;
    }

    // the image was not written after the last evaluation: x and y of that phi, the evaluation's operations again
    for (int k = 0; k < K; ++k) {
        const int idx = tid + k * T;
        if (mine && idx < nodes) {
            const Stencil s = stencil_of(idx, N, rN);
            float x, y;
            moved_node(s, img[s.rowE + s.j], img[s.rowW + s.j], img[s.row + s.jN], img[s.row + s.jS], n1, inv2h, x, y);
            xo[noff + idx] = x;
            yo[noff + idx] = y;
        }
    }
    write_status(b, tid, steps, res, status, steps_out, res_out, status_out);
}

// The iteration of ma_strided_kernel with the M2N 'fast' monitor (include/gadapt_mesh.h): mon[b] = (mon_reg, beta), no powf.
__global__ __launch_bounds__(MAX_THREADS) void ma_m2n_strided_kernel(const int32_t* __restrict__ desc, const float* __restrict__ gauss,
                                                                    const float* __restrict__ mon, double cfl, float tol, int tol_zero,
                                                                    int max_steps, float* __restrict__ xo, float* __restrict__ yo,
                                                                    int32_t* __restrict__ steps_out, float* __restrict__ res_out,
                                                                    int32_t* __restrict__ status_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int b = blockIdx.x;
    const int32_t* d = desc + GADAPT_MA_DESC * b;
    const int N = d[GADAPT_MA_D_N], noff = d[GADAPT_MA_D_NODE_OFF], goff = d[GADAPT_MA_D_GAUSS_OFF], ng = d[GADAPT_MA_D_GAUSS_N];
    const int nodes = N * N, T = ma_threads(nodes), nw = T >> 6, K = (nodes + T - 1) / T;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* red = reinterpret_cast<float*>(lds);
    float* gc = red + 5 * ROW;
    double* img = reinterpret_cast<double*>(lds + 4 * M2N_HEAD);

    const bool mine = tid < T;                           // a launch has the threads of its largest mesh
    const float n1 = (float)(N - 1), rN = 1.0f / (float)N;
    const double n1d = (double)(N - 1);
    const double inv2h = 0.5 * n1d, invh2 = n1d * n1d, inv4h2 = 0.25 * invh2;   // exact
    const float invh2f = n1 * n1;                                               // exact: n1 <= 80
    const float dt = (float)(cfl / invh2);
    const float reg = mon[2 * b], beta = mon[2 * b + 1];

    if (tid < ng) {                                      // ng <= 8 <= the threads of any mesh
        const float* g = gauss + 4 * (int64_t)(goff + tid);
        const float q0 = g[2] * g[2], q1 = g[3] * g[3];
        float* o = gc + GAUSS_CONSTS * tid;
        o[0] = g[0], o[1] = g[1], o[2] = 1.0f / q0, o[3] = 1.0f / q1;
        o[4] = 4.0f / (q0 * q0), o[5] = 2.0f / q0, o[6] = 4.0f / (q1 * q1), o[7] = 2.0f / q1;
        if (tid == ng - 1) red[(M2N_HEAD - 4)] = (16.0f * o[2]) * o[3];   // u_xy is the LAST Gaussian's only, as in the reference
    }
    if (tid == 0 && ng == 0) red[(M2N_HEAD - 4)] = 0.0f;       // read below whatever ng is: never an unwritten word
    for (int k = 0; k < K; ++k) {
        const int idx = tid + k * T;
        if (mine && idx < nodes) img[idx] = 0.0;
    }
    float Fs[MAX_K], dets[MAX_K], r[MAX_K];
#pragma unroll
    for (int q = 0; q < MAX_K; ++q) Fs[q] = 0.0f, dets[q] = 1.0f, r[q] = 0.0f;
    float res = 0.0f;
    int steps = 0, status;

    for (;;) {
        __syncthreads();                                 // the image is complete (and, the first time, the constants)
        const float cxy = red[(M2N_HEAD - 4)];
        float a_f = -INFINITY, a_lm = INFINITY;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const int idx = tid + k * T;
            const bool own = mine && idx < nodes;
            const Stencil s = stencil_of(own ? idx : 0, N, rN);
            const double p0 = img[s.c];
            const double pE = img[s.rowE + s.j], pW = img[s.rowW + s.j], pN = img[s.row + s.jN], pS = img[s.row + s.jS];
            float x, y;
            moved_node(s, pE, pW, pN, pS, n1, inv2h, x, y);
            const double pEN = img[s.rowE + s.jN], pES = img[s.rowE + s.jS], pWN = img[s.rowW + s.jN], pWS = img[s.rowW + s.jS];
            const float A = (float)(1.0 + ((pE - 2.0 * p0) + pW) * invh2);
            const float B = (float)(1.0 + ((pN - 2.0 * p0) + pS) * invh2);
            const float Cc = (float)((((pEN - pES) - pWN) + pWS) * inv4h2);
            const float det = A * B - Cc * Cc;
            const float lam = 0.5f * ((A + B) - sqrtf((A - B) * (A - B) + 4.0f * (Cc * Cc)));
            float uxx = 0.0f, uyy = 0.0f, dxl = 0.0f, dyl = 0.0f, gl = 0.0f;
#pragma unroll 1
            for (int g = 0; g < ng; ++g) {
                const float4 g0 = *reinterpret_cast<const float4*>(gc + GAUSS_CONSTS * g);
                const float4 g1 = *reinterpret_cast<const float4*>(gc + GAUSS_CONSTS * g + 4);
                const float dx = x - g0.x, dy = y - g0.y;
                const float dx2 = dx * dx, dy2 = dy * dy;
                const float e = expf(-(dx2 * g0.z) - dy2 * g0.w);
                uxx = uxx + (g1.x * dx2 - g1.y) * e;
                uyy = uyy + (g1.z * dy2 - g1.w) * e;
                dxl = dx, dyl = dy, gl = e;              // what is left after the loop is the last Gaussian's
            }
            const float uxy = (cxy * (dxl * dyl)) * gl;
            const float Fn = sqrtf((uxx * uxx + 2.0f * (uxy * uxy)) + uyy * uyy);
            // a lane's own slots in increasing k; a slot without a node gives -inf, +inf
            a_f = fmaxf(a_f, own ? Fn : -INFINITY);
            a_lm = fminf(a_lm, own ? lam : INFINITY);
#pragma unroll
            for (int q = 0; q < MAX_K; ++q) Fs[q] = q == k ? Fn : Fs[q], dets[q] = q == k ? det : dets[q];
        }
        const float s_f = wave_max(a_f);
        if (lane == 0 && wave < nw) red[4 * ROW + wave] = s_f;
        __syncthreads();                                 // the wave maxima of F are complete
        float fmx = red[4 * ROW];
        for (int w = 1; w < nw; ++w) fmx = fmaxf(fmx, red[4 * ROW + w]);
        // fmx was read from LDS by all lanes alike: a constant monitor is a decision of the whole mesh
        const bool flat = !(fmx > 0.0f);
        float a_wr = 0.0f, a_mx = -INFINITY, a_mn = INFINITY;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {                    // one copy of the inlined logf; the slot's F and det by select chains
            const int idx = tid + k * T;
            const bool own = mine && idx < nodes;
            const float wgt = node_weight(stencil_of(own ? idx : 0, N, rN), N);
            float Fk = Fs[0], detk = dets[0];
#pragma unroll
            for (int q = 1; q < MAX_K; ++q) Fk = q == k ? Fs[q] : Fk, detk = q == k ? dets[q] : detk;
            const float m = reg + (flat ? 0.0f : beta * (Fk / fmx));
            const float rv = logf(m * detk);
            a_wr = a_wr + (own ? wgt * rv : 0.0f);
            a_mx = fmaxf(a_mx, own ? rv : -INFINITY);
            a_mn = fminf(a_mn, own ? rv : INFINITY);
#pragma unroll
            for (int q = 0; q < MAX_K; ++q) r[q] = q == k ? rv : r[q];
        }
        const float s_wr = wave_sum(a_wr);
        const float s_mx = wave_max(a_mx);
        const float s_mn = wave_min(a_mn);
        const float s_lm = wave_min(a_lm);
        if (lane == 0 && wave < nw) {
            red[wave] = s_wr, red[ROW + wave] = s_mx, red[2 * ROW + wave] = s_mn, red[3 * ROW + wave] = s_lm;
        }
        __syncthreads();
        float sum = red[0], mx = red[ROW], mn = red[2 * ROW], lmin = red[3 * ROW];
        for (int w = 1; w < nw; ++w) {
            sum = sum + red[w];
            mx = fmaxf(mx, red[ROW + w]);
            mn = fminf(mn, red[2 * ROW + w]);
            lmin = fminf(lmin, red[3 * ROW + w]);
        }
        const float rbar = sum / invh2f;                 // the weights add up to (N - 1)^2
        res = fmaxf(mx - rbar, rbar - mn);
        // every value below was read from LDS by all lanes alike; written so that a NaN ends the loop
        if (!(lmin > 0.0f) || !(res - res == 0.0f)) { status = GADAPT_MA_NONCONVEX; break; }
        if (!tol_zero && res <= tol) { status = GADAPT_MA_CONVERGED; break; }
        if (steps >= max_steps) { status = GADAPT_MA_CAP; break; }
        const float dtl = dt * fminf(1.0f, lmin);
#pragma unroll
        for (int q = 0; q < MAX_K; ++q) {                // own nodes only: nobody reads them before the next barrier
            const int idx = tid + q * T;
            if (q < K && mine && idx < nodes) img[idx] = img[idx] + (double)(dtl * (r[q] - rbar));
        }
        ++steps;
    }

    // the image was not written after the last evaluation: x and y of that phi, the evaluation's operations again
    for (int k = 0; k < K; ++k) {
        const int idx = tid + k * T;
        if (mine && idx < nodes) {
            const Stencil s = stencil_of(idx, N, rN);
            float x, y;
            moved_node(s, img[s.rowE + s.j], img[s.rowW + s.j], img[s.row + s.jN], img[s.row + s.jS], n1, inv2h, x, y);
            xo[noff + idx] = x;
            yo[noff + idx] = y;
        }
    }
    write_status(b, tid, steps, res, status, steps_out, res_out, status_out);
}

// The host side of both entry points: everything is checked on desc_host before the one launch.
int strided_launch(const char* who, bool m2n, int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* gauss,
                   const float* mon, double cfl, double tol, int max_steps, float* x, float* y, int32_t* steps, float* residual,
                   int32_t* status, void* stream) {
    Geometry g;
    const int rc = check_batch(who, STRIDED_MAX_SIDE, ONE_WORKGROUP, false, n_mesh, desc_host, desc, gauss, mon, cfl, tol, max_steps, x,
                               y, steps, residual, status, &g);
    if (rc != GADAPT_MESH_OK) return rc;
    const float tol_f = (float)tol;
    return launch(m2n ? ma_m2n_strided_kernel : ma_strided_kernel, n_mesh, g.threads,
                  strided_lds_bytes(m2n ? M2N_HEAD : MA_HEAD, g.side * g.side), stream, desc, gauss, mon, cfl, tol_f,
                  (int)(tol_f == 0.0f), max_steps, x, y, steps, residual, status);
}

}  // namespace

extern "C" int gadapt_ma_strided_max_side(void) { return STRIDED_MAX_SIDE; }

extern "C" int64_t gadapt_ma_strided_lds_bytes(int nodes) {
    if (nodes < 9 || nodes > STRIDED_MAX_NODES) return mesh_fail(GADAPT_MESH_E_SIZE, "gadapt_ma_strided_lds_bytes: 9..6561 nodes");
    return strided_lds_bytes(MA_HEAD, nodes);
}

extern "C" int64_t gadapt_ma_m2n_strided_lds_bytes(int nodes) {
    if (nodes < 9 || nodes > STRIDED_MAX_NODES) return mesh_fail(GADAPT_MESH_E_SIZE, "gadapt_ma_m2n_strided_lds_bytes: 9..6561 nodes");
    return strided_lds_bytes(M2N_HEAD, nodes);
}

extern "C" int gadapt_ma_batch_strided(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* gauss,
                                       const float* mon, double cfl, double tol, int max_steps, float* x, float* y, int32_t* steps,
                                       float* residual, int32_t* status, void* stream) {
    return strided_launch("gadapt_ma_batch_strided", false, n_mesh, desc_host, desc, gauss, mon, cfl, tol, max_steps, x, y, steps,
                          residual, status, stream);
}

extern "C" int gadapt_ma_m2n_batch_strided(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* gauss,
                                           const float* mon, double cfl, double tol, int max_steps, float* x, float* y,
                                           int32_t* steps, float* residual, int32_t* status, void* stream) {
    return strided_launch("gadapt_ma_m2n_batch_strided", true, n_mesh, desc_host, desc, gauss, mon, cfl, tol, max_steps, x, y, steps,
                          residual, status, stream);
}
