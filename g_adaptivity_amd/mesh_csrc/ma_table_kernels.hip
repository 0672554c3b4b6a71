// ma_table_kernels.hip - batched Monge-Ampere target meshes from a TABULATED monitor, on both routes (include/gadapt_mesh.h has
// the iteration; ma_kernels.hip and ma_strided_kernels.hip are the kernels these two are derived from).
//
// ma_table_kernel is ma_kernel and ma_table_strided_kernel is ma_strided_kernel with one change: the loop over the Gaussians and
// the powf are replaced by a bilinear read of the mesh's own table M [T, T] (table_monitor below), M[i, j] being the monitor at
// the physical point (i / (T-1), j / (T-1)).  px, py, a, b, c, x, y, det, lambda, the reductions and their order, the exit tests
// and their order, the update, and the rule that every lane reads exit-deciding values back from LDS are the siblings',
// operation for operation; on the strided route so are the fp64 phi, the five stencil expressions rounded once to fp32 and the
// ownership t + k T.  The barriers and what is written between them are the siblings' too (two a step).
//
// The table is read from global memory through the vector cache on both routes: four loads per node and update (two rows, two
// adjacent columns each), L1/L2-resident after the first touch.  The strided route's 53 000 bytes of LDS at 81 x 81 leave no
// room for a table, and a 1024 x 1024 table is 4 MB.  x and y are clamped to [0, 1] by comparisons that send a NaN to 0, so no
// index is ever formed from a NaN, and i0 <= T - 2: every index is within the table whatever phi holds.  A table entry that is
// <= 0 or not finite makes r not finite, which is the NONCONVEX exit as it stands.  Lanes and slots without a node read with
// node 0's coordinates and contribute 0, -inf, +inf, +inf.
//
// LDS: the 256 bytes of wave partials, then the siblings' images of phi (two fp32 images on the lane route, one fp64 image on
// the strided one: 52 744 bytes at 81 x 81).  logf / sqrtf are the accurate ones; no FMA contraction (Makefile and the pragma).
//
// ma_table_kernel: 74 VGPRs, no AGPRs, 71 SGPRs, no scratch, no spills (hipcc -Rpass-analysis=kernel-resource-usage, gfx950).
// ma_table_strided_kernel: 71 VGPRs, no AGPRs, 90 SGPRs, no scratch, no spills (the same report), one instance for every K.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "gadapt_mesh.h"
#include "mesh_common.h"

#pragma clang fp contract(off)

using namespace gadapt_mesh_shared;                      // g_err, mesh_fail, dpp_move, wave_sum, wave_max, wave_min

namespace {

constexpr int MAX_TABLE_SIDE = 1024;
constexpr int MAX_WAVES = 16;                            // 1024 lanes on both routes
constexpr int RED_FLOATS = 4 * MAX_WAVES;                // red[4][MAX_WAVES]

// the lane route: ma_kernels.hip
constexpr int LANE_MAX_SIDE = 32;
constexpr int LANE_MAX_NODES = LANE_MAX_SIDE * LANE_MAX_SIDE;
static_assert(LANE_MAX_NODES == GADAPT_MMPDE5_MAX_NODES, "one lane per node, one workgroup per mesh");
__host__ __device__ inline int lane_threads(int nodes) { return (nodes + 63) & ~63; }
__host__ __device__ inline int64_t lane_lds_bytes(int nodes) { return 4 * (RED_FLOATS + 2 * (int64_t)nodes); }

// the strided route: ma_strided_kernels.hip
constexpr int STRIDED_MAX_SIDE = 81;
constexpr int MAX_THREADS = 1024;
constexpr int MAX_K = (STRIDED_MAX_SIDE * STRIDED_MAX_SIDE + MAX_THREADS - 1) / MAX_THREADS;
static_assert(MAX_K == 7, "ma_table_strided_kernel keeps seven residuals per lane");
static_assert((4 * RED_FLOATS) % 16 == 0, "the image is read with 8-byte loads");
__host__ __device__ inline int64_t strided_lds_bytes(int nodes) { return 4 * RED_FLOATS + 8 * (int64_t)nodes; }
__host__ __device__ inline int strided_threads(int nodes) {
    const int t = (nodes + 63) & ~63;
    return t < MAX_THREADS ? t : MAX_THREADS;
}

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
    const int nodes = N * N, nw = lane_threads(nodes) >> 6;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* red = lds;
    float* img[2] = {lds + RED_FLOATS, lds + RED_FLOATS + nodes};

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
            red[wave] = s_wr, red[MAX_WAVES + wave] = s_mx, red[2 * MAX_WAVES + wave] = s_mn, red[3 * MAX_WAVES + wave] = s_lm;
        }
        __syncthreads();
        float sum = red[0], mx = red[MAX_WAVES], mn = red[2 * MAX_WAVES], lmin = red[3 * MAX_WAVES];
        for (int w = 1; w < nw; ++w) {
            sum = sum + red[w];
            mx = fmaxf(mx, red[MAX_WAVES + w]);
            mn = fminf(mn, red[2 * MAX_WAVES + w]);
            lmin = fminf(lmin, red[3 * MAX_WAVES + w]);
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
    if (tid == 0) {
        steps_out[b] = steps;
        res_out[b] = res;
        status_out[b] = status;
    }
}

// floor(c / N) for 0 <= c < N^2, 3 <= N <= 81: (c + 0.5) is exact, rN = 1 / N and the product are each within 2^-24 relative,
// so the product is within 81 * 2^-23 < 1e-5 of (c + 0.5) / N, which is at least 0.5 / 81 > 6e-3 away from every integer.
__device__ inline int node_row(int c, float rN) { return (int)(((float)c + 0.5f) * rN); }

struct Stencil {
    int c, i, j, row, rowE, rowW, jN, jS;
};

// even reflection: the neighbour beyond an edge is the one inside it
__device__ inline Stencil stencil_of(int c, int N, float rN) {
    Stencil s;
    const int i = node_row(c, rN);
    s.c = c, s.i = i, s.j = c - i * N, s.row = i * N;
    s.rowE = (i == N - 1 ? N - 2 : i + 1) * N, s.rowW = (i == 0 ? 1 : i - 1) * N;
    s.jN = s.j == N - 1 ? N - 2 : s.j + 1, s.jS = s.j == 0 ? 1 : s.j - 1;
    return s;
}

// x = xi + (float)((pE - pW) (n1 / 2)), y likewise: the evaluation and the epilogue share these operations
__device__ inline void moved_node(const Stencil& s, double pE, double pW, double pN, double pS, float n1, double inv2h, float& x,
                                  float& y) {
    x = (float)s.i / n1 + (float)((pE - pW) * inv2h);
    y = (float)s.j / n1 + (float)((pN - pS) * inv2h);
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
    const int nodes = N * N, T = strided_threads(nodes), nw = T >> 6, K = (nodes + T - 1) / T;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* red = reinterpret_cast<float*>(lds_bytes);
    double* img = reinterpret_cast<double*>(lds_bytes + 4 * RED_FLOATS);

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
            red[wave] = s_wr, red[MAX_WAVES + wave] = s_mx, red[2 * MAX_WAVES + wave] = s_mn, red[3 * MAX_WAVES + wave] = s_lm;
        }
        __syncthreads();
        float sum = red[0], mx = red[MAX_WAVES], mn = red[2 * MAX_WAVES], lmin = red[3 * MAX_WAVES];
        for (int w = 1; w < nw; ++w) {
            sum = sum + red[w];
            mx = fmaxf(mx, red[MAX_WAVES + w]);
            mn = fminf(mn, red[2 * MAX_WAVES + w]);
            lmin = fminf(lmin, red[3 * MAX_WAVES + w]);
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
    if (tid == 0) {
        steps_out[b] = steps;
        res_out[b] = res;
        status_out[b] = status;
    }
}

#ifdef GADAPT_MA_TABLE_NO_LAUNCH
}  // namespace
int g_sweep_threads = 0;                                 // what the launch would have been given
int64_t g_sweep_lds = 0;
namespace {
#endif

// The host side of both entry points: everything is checked on desc_host before the one launch.
int table_launch(const char* who, bool strided, int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* tables,
                 double cfl, double tol, int max_steps, float* x, float* y, int32_t* steps, float* residual, int32_t* status,
                 void* stream) {
    char msg[240];
    const int max_side = strided ? STRIDED_MAX_SIDE : LANE_MAX_SIDE;
    if (n_mesh < 1 || !desc_host || !desc || !tables || !x || !y || !steps || !residual || !status) {
        snprintf(msg, sizeof msg, "%s: empty batch or null pointer", who);
        return mesh_fail(GADAPT_MESH_E_BADARG, msg);
    }
    if (!(cfl > 0.0) || !(tol >= 0.0) || !isfinite(cfl) || !isfinite(tol)) {
        snprintf(msg, sizeof msg, "%s: need cfl > 0 and tol >= 0, both finite", who);
        return mesh_fail(GADAPT_MESH_E_BADARG, msg);
    }
    if (max_steps < 0 || max_steps > GADAPT_MMPDE5_MAX_STEPS) {
        snprintf(msg, sizeof msg, "%s: max_steps %d; 0..%d supported (the loop must end)", who, max_steps, GADAPT_MMPDE5_MAX_STEPS);
        return mesh_fail(GADAPT_MESH_E_SIZE, msg);
    }
    int threads = 64, most = 0;
    for (int b = 0; b < n_mesh; ++b) {
        const int32_t* d = desc_host + GADAPT_MA_DESC * b;
        const int N = d[GADAPT_MA_D_N], T = d[GADAPT_MA_D_TABLE_T];
        if (N < 3 || d[GADAPT_MA_D_NODE_OFF] < 0 || d[GADAPT_MA_D_TABLE_OFF] < 0) {
            snprintf(msg, sizeof msg, "%s: mesh %d: N %d, offsets %d / %d", who, b, N, d[GADAPT_MA_D_NODE_OFF], d[GADAPT_MA_D_TABLE_OFF]);
            return mesh_fail(GADAPT_MESH_E_BADARG, msg);
        }
        if (N > max_side || T < 2 || T > MAX_TABLE_SIDE) {
            snprintf(msg, sizeof msg, "%s: mesh %d: N = %d with a table of T = %d; N <= %d a side (one workgroup holds a mesh) and "
                     "2 <= T <= %d", who, b, N, T, max_side, MAX_TABLE_SIDE);
            return mesh_fail(GADAPT_MESH_E_SIZE, msg);
        }
        if ((int64_t)d[GADAPT_MA_D_NODE_OFF] + N * N > INT32_MAX || (int64_t)d[GADAPT_MA_D_TABLE_OFF] + T * T > INT32_MAX) {
            snprintf(msg, sizeof msg, "%s: more than 2^31 nodes or table entries in one batch", who);
            return mesh_fail(GADAPT_MESH_E_SIZE, msg);
        }
        const int t = strided ? strided_threads(N * N) : lane_threads(N * N);
        threads = t > threads ? t : threads;
        most = N * N > most ? N * N : most;
    }
#ifdef GADAPT_MA_TABLE_NO_LAUNCH                          // tools/ma_table_entry_sweep.cpp: the checks above alone, on the host
    g_sweep_threads = threads, g_sweep_lds = strided ? strided_lds_bytes(most) : lane_lds_bytes(most);
    return GADAPT_MESH_OK;
#endif
    const float tol_f = (float)tol;
    if (strided)
        ma_table_strided_kernel<<<n_mesh, threads, (size_t)strided_lds_bytes(most), (hipStream_t)stream>>>(
            desc, tables, cfl, tol_f, tol_f == 0.0f, max_steps, x, y, steps, residual, status);
    else
        ma_table_kernel<<<n_mesh, threads, (size_t)lane_lds_bytes(most), (hipStream_t)stream>>>(
            desc, tables, cfl, tol_f, tol_f == 0.0f, max_steps, x, y, steps, residual, status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mesh_fail(GADAPT_MESH_E_LAUNCH, hipGetErrorString(e));
    return GADAPT_MESH_OK;
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
