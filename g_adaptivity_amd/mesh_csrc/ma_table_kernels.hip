// ma_table_kernels.hip - batched Monge-Ampere target meshes from a TABULATED monitor, on both routes (include/gadapt_mesh.h has
// the iteration, ma_iteration.h its one statement).
//
// ma_table_kernel is ma_kernel and ma_table_strided_kernel is ma_strided_kernel with one change: the loop over the Gaussians and
// the powf are replaced by a bilinear read of the mesh's own table M [T, T] (table_monitor below), M[i, j] being the monitor at
// the physical point (i / (T-1), j / (T-1)).  Everything else is the siblings', operation for operation, two barriers a step.
//
// The table is read from global memory through the vector cache on both routes: four loads per node and update (two rows, two
// adjacent columns each), L1/L2-resident after the first touch.  The strided route's 53 000 bytes of LDS at 81 x 81 leave no
// room for a table, and a 1024 x 1024 table is 4 MB.  x and y are clamped to [0, 1] by comparisons that send a NaN to 0, so no
// index is ever formed from a NaN, and i0 <= T - 2: every index is within the table whatever phi holds.  A table entry that is
// <= 0 or not finite makes r not finite, which is the NONCONVEX exit as it stands.  Lanes and slots without a node read with
// node 0's coordinates.
//
// LDS: the 256 bytes of wave partials, then the siblings' images of phi (52 744 bytes at 81 x 81 on the strided route).
//
// ma_table_kernel: 74 VGPRs, no AGPRs, 71 SGPRs, no scratch, no spills (hipcc -Rpass-analysis=kernel-resource-usage, gfx950).
// ma_table_strided_kernel: 71 VGPRs, no AGPRs, 90 SGPRs, no scratch, no spills (the same report), one instance for every K.
#include "ma_iteration.h"                            // and through it ma_host.h, mesh_common.h, gadapt_mesh.h

#pragma clang fp contract(off)

using namespace gadapt_ma;

namespace {

// The monitor at (x, y): bilinear in the table's cell, continuous across cells, exact for tables linear in x and y.
// 0 <= i0, j0 <= T - 2, so the four reads are M[i0 T + j0 (+ 1) (+ T)] <= M[T^2 - 1].
__device__ inline float table_monitor(const float* __restrict__ M, int T, float t1, float x, float y) {
    const float xc = x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f;          // a NaN maps to 0
    const float yc = y > 0.0f ? (y < 1.0f ? y : 1.0f) : 0.0f;
    const float fx = xc * t1, fy = yc * t1;
    const int i0 = min((int)fx, T - 2), j0 = min((int)fy, T - 2);
    const float ax = fx - (float)i0, ay = fy - (float)j0;
    const float* q = M + (i0 * T + j0);                                // T <= 1024: below 2^20
    const float m00 = q[0], m01 = q[1], m10 = q[T], m11 = q[T + 1];
    const float m0 = m00 + ax * (m10 - m00);
    const float m1 = m01 + ax * (m11 - m01);
    return m0 + ay * (m1 - m0);
}

__global__ __launch_bounds__(LANE_MAX_NODES) void ma_table_kernel(const int32_t* __restrict__ desc, const float* __restrict__ tables,
                                                                 double cfl, float tol, int tol_zero, int max_steps,
                                                                 float* __restrict__ xo, float* __restrict__ yo,
                                                                 int32_t* __restrict__ steps_out, float* __restrict__ res_out,
                                                                 int32_t* __restrict__ status_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x;
    const int32_t* d = desc + GADAPT_MA_DESC * b;
    const int N = d[GADAPT_MA_D_N], noff = d[GADAPT_MA_D_NODE_OFF], T = d[GADAPT_MA_D_TABLE_T];
    const float* M = tables + d[GADAPT_MA_D_TABLE_OFF];
    const int nodes = N * N, nw = (nodes + 63) >> 6;     // whole waves: N <= 32 is within ma_threads' cap
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* red = lds;
    float* img[2] = {lds + TABLE_HEAD, lds + TABLE_HEAD + nodes};

    const bool own = tid < nodes;
    const int c = own ? tid : 0;
    const int i = c / N, j = c - i * N;
    // even reflection: the neighbour beyond an edge is the one inside it
    const int rowE = (i == N - 1 ? N - 2 : i + 1) * N, rowW = (i == 0 ? 1 : i - 1) * N;
    const int jN = j == N - 1 ? N - 2 : j + 1, jS = j == 0 ? 1 : j - 1;
    const float n1 = (float)(N - 1), t1 = (float)(T - 1);
    const float xi = (float)i / n1, xj = (float)j / n1;
    const float inv2h = 0.5f * n1, invh2 = n1 * n1, inv4h2 = 0.25f * invh2;   // exact: n1 <= 31
    const float wgt = ((i == 0 || i == N - 1) ? 0.5f : 1.0f) * ((j == 0 || j == N - 1) ? 0.5f : 1.0f);
    const float dt = (float)(cfl / ((double)(N - 1) * (double)(N - 1)));

    float phi = 0.0f, x = xi, y = xj, res = 0.0f;
    if (own) img[0][c] = phi;
    int steps = 0, cur = 0, status;

    for (;;) {
        __syncthreads();                                 // image `cur` is complete
        const float* p = img[cur];
        const float pE = p[rowE + j], pW = p[rowW + j], pN = p[i * N + jN], pS = p[i * N + jS];
        const float pEN = p[rowE + jN], pES = p[rowE + jS], pWN = p[rowW + jN], pWS = p[rowW + jS];
        x = xi + (pE - pW) * inv2h;
        y = xj + (pN - pS) * inv2h;
        const float A = 1.0f + ((pE - 2.0f * phi) + pW) * invh2;
        const float B = 1.0f + ((pN - 2.0f * phi) + pS) * invh2;
        const float Cc = (((pEN - pES) - pWN) + pWS) * inv4h2;
        const float det = A * B - Cc * Cc;
        const float lam = 0.5f * ((A + B) - sqrtf((A - B) * (A - B) + 4.0f * (Cc * Cc)));
        const float m = table_monitor(M, T, t1, x, y);
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
        for (int w = 1; w < nw; ++w) {
            sum = sum + red[w];
            mx = fmaxf(mx, red[ROW + w]);
            mn = fminf(mn, red[2 * ROW + w]);
            lmin = fminf(lmin, red[3 * ROW + w]);
        }
        const float rbar = sum / invh2;                  // the weights add up to (N - 1)^2
        res = fmaxf(mx - rbar, rbar - mn);
        // every value below was read from LDS by all lanes alike; written so that a NaN ends the loop
        if (!(lmin > 0.0f) || !(res - res == 0.0f)) { status = GADAPT_MA_NONCONVEX; break; }
        if (!tol_zero && res <= tol) { status = GADAPT_MA_CONVERGED; break; }
        if (steps >= max_steps) { status = GADAPT_MA_CAP; break; }
        phi = phi + (dt * fminf(1.0f, lmin)) * (r - rbar);
        ++steps;
        cur ^= 1;
        if (own) img[cur][c] = phi;                      // this image was last read before the barrier above
    }

    if (own) {
        xo[noff + c] = x;
        yo[noff + c] = y;
    }
    write_status(b, tid, steps, res, status, steps_out, res_out, status_out);
}

__global__ __launch_bounds__(MAX_THREADS) void ma_table_strided_kernel(const int32_t* __restrict__ desc,
                                                                      const float* __restrict__ tables, double cfl, float tol,
                                                                      int tol_zero, int max_steps, float* __restrict__ xo,
                                                                      float* __restrict__ yo, int32_t* __restrict__ steps_out,
                                                                      float* __restrict__ res_out, int32_t* __restrict__ status_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_bytes[];
    const int b = blockIdx.x;
    const int32_t* d = desc + GADAPT_MA_DESC * b;
    const int N = d[GADAPT_MA_D_N], noff = d[GADAPT_MA_D_NODE_OFF], TS = d[GADAPT_MA_D_TABLE_T];
    const float* M = tables + d[GADAPT_MA_D_TABLE_OFF];
    const int nodes = N * N, T = ma_threads(nodes), nw = T >> 6, K = (nodes + T - 1) / T;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* red = reinterpret_cast<float*>(lds_bytes);
    double* img = reinterpret_cast<double*>(lds_bytes + 4 * TABLE_HEAD);

    const bool mine = tid < T;                           // a launch has the threads of its largest mesh
    const float n1 = (float)(N - 1), rN = 1.0f / (float)N, t1 = (float)(TS - 1);
    const double n1d = (double)(N - 1);
    const double inv2h = 0.5 * n1d, invh2 = n1d * n1d, inv4h2 = 0.25 * invh2;   // exact
    const float invh2f = n1 * n1;                                               // exact: n1 <= 80
    const float dt = (float)(cfl / invh2);

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
        __syncthreads();                                 // the image is complete
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
            const float m = table_monitor(M, TS, t1, x, y);
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

// The host side of both entry points: everything is checked on desc_host before the one launch.
int table_launch(const char* who, bool strided, int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* tables,
                 double cfl, double tol, int max_steps, float* x, float* y, int32_t* steps, float* residual, int32_t* status,
                 void* stream) {
    Geometry g;
    const int rc = check_batch(who, strided ? STRIDED_MAX_SIDE : LANE_MAX_SIDE, ONE_WORKGROUP, true, n_mesh, desc_host, desc, tables,
                               nullptr, cfl, tol, max_steps, x, y, steps, residual, status, &g);
    if (rc != GADAPT_MESH_OK) return rc;
    const float tol_f = (float)tol;
    const int most = g.side * g.side;
    return launch(strided ? ma_table_strided_kernel : ma_table_kernel, n_mesh, g.threads,
                  strided ? strided_lds_bytes(TABLE_HEAD, most) : lane_lds_bytes(TABLE_HEAD, most), stream, desc, tables, cfl, tol_f,
                  (int)(tol_f == 0.0f), max_steps, x, y, steps, residual, status);
}

}  // namespace

extern "C" int gadapt_ma_table_max_side(void) { return MAX_TABLE_SIDE; }

extern "C" int gadapt_ma_table_batch(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* tables, double cfl,
                                     double tol, int max_steps, float* x, float* y, int32_t* steps, float* residual, int32_t* status,
                                     void* stream) {
    return table_launch("gadapt_ma_table_batch", false, n_mesh, desc_host, desc, tables, cfl, tol, max_steps, x, y, steps, residual,
                        status, stream);
}

extern "C" int gadapt_ma_table_batch_strided(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* tables,
                                             double cfl, double tol, int max_steps, float* x, float* y, int32_t* steps,
                                             float* residual, int32_t* status, void* stream) {
    return table_launch("gadapt_ma_table_batch_strided", true, n_mesh, desc_host, desc, tables, cfl, tol, max_steps, x, y, steps,
                        residual, status, stream);
}
