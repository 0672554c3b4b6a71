// gadapt_block_plan.h - tile plan of the narrow route's one-launch forward (wide::fwd_narrow_block_kernel, gadapt_narrow_fwd.inc): one
// definition for the kernel, its launcher and the host copy that the CPU tests call (gadapt_narrow_block_range_host, csr_build.cpp).
//
// A workgroup owns GADAPT_NARROW_TILE consecutive nodes and runs K consecutive layers for them.  Layer k + 1 of node i needs layer k of
// i's in-neighbours, and on an eligible graph (halo h: gadapt_narrow_block_halo_host) those lie within h nodes of i's aligned 32-node
// group, so layer k is computed on the owned range widened by (K - 1 - k) h on each side and the layer-0 input is loaded one h wider
// still.  Every range is clamped to [0, ceil32(N)) and stays 32-aligned: a half-wave is one aligned 32-node group at every layer.
#ifndef GADAPT_BLOCK_PLAN_H
#define GADAPT_BLOCK_PLAN_H

#include <stdint.h>

#define GADAPT_NARROW_TILE 512          /* nodes a workgroup owns */
#define GADAPT_NARROW_BLOCK_LAYERS 4    /* layers of one launch, at most */

#ifdef __HIPCC__
#define GADAPT_PLAN_FN __host__ __device__ static inline
#else
#define GADAPT_PLAN_FN static inline
#endif

// [lo, hi) of layer k (0 <= k < K) of tile t in a group of K layers; k = -1: the load range
GADAPT_PLAN_FN void gadapt_block_range(int64_t n_nodes, int halo, int K, int64_t t, int k, int64_t* lo, int64_t* hi) {
    const int64_t w = (int64_t)(K - 1 - k) * halo, n32 = (n_nodes + 31) / 32 * 32;
    const int64_t a = GADAPT_NARROW_TILE * t - w, b = GADAPT_NARROW_TILE * (t + 1) + w;
    *lo = a < 0 ? 0 : a;
    *hi = b > n32 ? n32 : b;
}
// First node of the workgroup's LDS frame (row r of the frame holds node frame0 + r) and its row count: the load range, rounded out to
// whole 64-node wave blocks so that the owned range starts on a wave boundary of the frame.  At most 1024 rows (K = 4, halo 64).
GADAPT_PLAN_FN int gadapt_block_frame_margin(int halo, int K) { return (K * halo + 63) / 64 * 64; }

#endif  // GADAPT_BLOCK_PLAN_H
