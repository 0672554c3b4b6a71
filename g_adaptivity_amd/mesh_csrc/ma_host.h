// ma_host.h - what the host side of the nine Monge-Ampere entry points shares (ma_kernels.hip, ma_strided_kernels.hip,
// ma_m2n_slow_kernels.hip, ma_table_kernels.hip): the limits, the launch geometry (threads and LDS layout of the seven kernels)
// the one batch check and the one launch.  No kernel: tools/ma_host_sweep.cpp builds from this header alone.
#ifndef GADAPT_MA_HOST_H
#define GADAPT_MA_HOST_H

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "gadapt_mesh.h"
#include "mesh_common.h"

namespace gadapt_ma {

constexpr int LANE_MAX_SIDE = 32, LANE_MAX_NODES = 32 * 32;          // one lane per node: gadapt_ma_max_side()
constexpr int SLOW_MAX_SIDE = 24, SLOW_MAX_NODES = 24 * 24;          // 576 lanes, 9 waves: gadapt_ma_m2n_slow_max_side()
constexpr int STRIDED_MAX_SIDE = 81, STRIDED_MAX_NODES = 81 * 81;    // gadapt_ma_strided_max_side()
constexpr int MAX_THREADS = 1024;
constexpr int MAX_K = (STRIDED_MAX_NODES + MAX_THREADS - 1) / MAX_THREADS;
constexpr int MAX_GAUSS = 8;                             // gadapt_ma_max_gauss(): every route takes the same Gaussians
constexpr int GAUSS_CONSTS = 8;                          // c0, c1, 1/q0, 1/q1, A0, B0, A1, B1
constexpr int MAX_TABLE_SIDE = 1024;                     // gadapt_ma_table_max_side()
constexpr int ROW = MAX_THREADS / 64;                    // a row of wave partials
static_assert(LANE_MAX_NODES == GADAPT_MMPDE5_MAX_NODES, "one lane per node, one workgroup per mesh");
static_assert(MAX_THREADS == GADAPT_MMPDE5_MAX_NODES, "the ownership of mmpde5_strided_kernel");
static_assert(MAX_K == 7, "the strided kernels keep seven residuals per lane");

// Whole waves, at most 1024 lanes: the lane route's one lane per node (N <= 32) and the strided route's T.
__host__ __device__ inline int ma_threads(int nodes) {
    const int t = (nodes + 63) & ~63;
    return t < MAX_THREADS ? t : MAX_THREADS;
}

// The head of every kernel's LDS, in floats: `rows` rows of wave partials, then the Gaussians' constants, then Cxy in a 16-byte
// slot of its own.  After it the lane route has two fp32 images of phi, each as long as the launch's largest mesh, the strided
// route one fp64 image; the slow kernel adds four node arrays, the band (row r holds K[r][r-d] at r (w+1) + d, w = N - 2) and the
// right-hand side.
constexpr int head_floats(int rows, bool gaussians, bool cxy) {
    return rows * ROW + (gaussians ? MAX_GAUSS * GAUSS_CONSTS : 0) + (cxy ? 4 : 0);
}
constexpr int MA_HEAD = head_floats(4, true, false);     // ma_kernel, ma_strided_kernel: 512 bytes
constexpr int M2N_HEAD = head_floats(5, true, true);     // row 4 is Fmax's: 592 bytes
constexpr int SLOW_HEAD = head_floats(6, true, true);    // rows 4 and 5 are Fmax's and Emax's
constexpr int TABLE_HEAD = head_floats(4, false, false); // 256 bytes
static_assert((4 * MA_HEAD) % 16 == 0 && (4 * M2N_HEAD) % 16 == 0 && (4 * TABLE_HEAD) % 16 == 0, "the fp64 image is read with 8-byte loads");

inline int64_t lane_lds_bytes(int head, int nodes) { return 4 * (head + 2 * (int64_t)nodes); }
// 52 488 + 512 = 53 000 bytes at 81 x 81 (53 080 under M2N, 52 744 with a table), below the 64 KB that need no raised limit
inline int64_t strided_lds_bytes(int head, int nodes) { return 4 * head + 8 * (int64_t)nodes; }
// 60 944 bytes at 24 x 24; 25 x 25 would take 68 556
inline int64_t slow_lds_bytes(int N) {
    const int64_t w = N - 2, n = w * w;
    return 4 * (SLOW_HEAD + 6 * (int64_t)N * N + n * (w + 1) + n);
}

struct Geometry {
    int threads, side;                                   // of the launch: its largest mesh's
};

// Everything an entry point checks on desc_host before its one launch, in the order the codes have precedence.  `side_reason`
// words the side limit; descriptor words 2 and 3 are a Gaussian offset and count (`field` may then be null if no mesh has a
// Gaussian, and `mon` is required) or, with `table`, a table offset and side (`field` is required, `mon` is not read).
inline int check_batch(const char* who, int max_side, const char* side_reason, bool table, int n_mesh, const int32_t* desc_host,
                       const int32_t* desc, const void* field, const void* mon, double cfl, double tol, int max_steps, const float* x,
                       const float* y, const int32_t* steps, const float* residual, const int32_t* status, Geometry* out) {
    using gadapt_mesh_shared::mesh_fail;
    char msg[240];
    if (n_mesh < 1 || !desc_host || !desc || !(table ? field : mon) || !x || !y || !steps || !residual || !status) {
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
    Geometry g = {64, 3};
    for (int b = 0; b < n_mesh; ++b) {
        const int32_t* d = desc_host + GADAPT_MA_DESC * b;
        const int N = d[GADAPT_MA_D_N], noff = d[GADAPT_MA_D_NODE_OFF], off = d[2], cnt = d[3];   // Gaussians or a table
        if (table) {
            if (N < 3 || noff < 0 || off < 0) {
                snprintf(msg, sizeof msg, "%s: mesh %d: N %d, offsets %d / %d", who, b, N, noff, off);
                return mesh_fail(GADAPT_MESH_E_BADARG, msg);
            }
            if (N > max_side || cnt < 2 || cnt > MAX_TABLE_SIDE) {
                snprintf(msg, sizeof msg, "%s: mesh %d: N = %d with a table of T = %d; N <= %d a side (%s) and 2 <= T <= %d", who, b, N,
                         cnt, max_side, side_reason, MAX_TABLE_SIDE);
                return mesh_fail(GADAPT_MESH_E_SIZE, msg);
            }
            if ((int64_t)noff + N * N > INT32_MAX || (int64_t)off + cnt * cnt > INT32_MAX) {
                snprintf(msg, sizeof msg, "%s: more than 2^31 nodes or table entries in one batch", who);
                return mesh_fail(GADAPT_MESH_E_SIZE, msg);
            }
        } else {
            if (N < 3 || noff < 0 || off < 0 || cnt < 0 || (cnt > 0 && !field)) {
                snprintf(msg, sizeof msg, "%s: mesh %d: N %d, offsets %d / %d, %d Gaussians", who, b, N, noff, off, cnt);
                return mesh_fail(GADAPT_MESH_E_BADARG, msg);
            }
            if (N > max_side || cnt > MAX_GAUSS) {
                snprintf(msg, sizeof msg, "%s: mesh %d: N = %d with %d Gaussians; N <= %d a side (%s) and at most %d Gaussians", who, b,
                         N, cnt, max_side, side_reason, MAX_GAUSS);
                return mesh_fail(GADAPT_MESH_E_SIZE, msg);
            }
            if ((int64_t)noff + N * N > INT32_MAX) {
                snprintf(msg, sizeof msg, "%s: more than 2^31 nodes in one batch", who);
                return mesh_fail(GADAPT_MESH_E_SIZE, msg);
            }
        }
        const int t = ma_threads(N * N);
        g.threads = t > g.threads ? t : g.threads;
        g.side = N > g.side ? N : g.side;
    }
    *out = g;
    return GADAPT_MESH_OK;
}

constexpr const char* ONE_WORKGROUP = "one workgroup holds a mesh";
constexpr const char* BAND_IN_LDS = "the band of the P1 solve stays in LDS";

// The one launch of an entry point, one workgroup per mesh, and its error test
template <class Kernel, class... Args>
inline int launch(Kernel kernel, int n_mesh, int threads, int64_t lds_bytes, void* stream, Args... args) {
    kernel<<<n_mesh, threads, (size_t)lds_bytes, (hipStream_t)stream>>>(args...);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GADAPT_MESH_OK : gadapt_mesh_shared::mesh_fail(GADAPT_MESH_E_LAUNCH, hipGetErrorString(e));
}

}  // namespace gadapt_ma

#endif
