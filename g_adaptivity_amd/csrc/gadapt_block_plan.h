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

// The top layer's backward target pass inside the block launch (fwd_narrow_block_kernel<., ., TOP>): the packed slab rows a tile owes.
// Slab row r holds the sums over nodes 256 r .. 256 r + 255 (the workgroup of grand_bwd_target_narrow_kernel that visits them): the
// wave sums of its four 64-node blocks as (b0 + b1) + (b2 + b3), blocks in node order.  A tile's eight waves own its eight 64-node
// blocks in ROTATED order - wave w owns frame block w or w + 8, whichever starts the owned range (margin / 64 waves in) - so:
//   gadapt_block_owned_block   the owned block (0..7, node order within the tile) of wave w;
//   gadapt_block_slab_plan     of tile t of n_tiles: rows[j] = 2 t + j (j = 0, 1), fed by the waves waves[j][0..3] in that order, and the
//                              rows beyond the last tile's that it fills with zeros: zero_first, zero_first + zero_step, ... < n_rows
//                              (every target launch of the step accumulates onto all n_rows = gadapt_backward_slab_rows rows and the
//                              tail sums them all, so each is written by exactly one tile).  A row index >= n_rows is not written.
GADAPT_PLAN_FN int gadapt_block_owned_block(int margin, int wave) { return (wave + 8 - margin / 64) & 7; }
struct gadapt_block_slab { int rows[2]; int waves[2][4]; int zero_first, zero_step; };
GADAPT_PLAN_FN struct gadapt_block_slab gadapt_block_slab_plan(int64_t n_nodes, int margin, int64_t t) {
    const int n_tiles = (int)((n_nodes + GADAPT_NARROW_TILE - 1) / GADAPT_NARROW_TILE);
    struct gadapt_block_slab s;
    for (int j = 0; j < 2; ++j) {
        s.rows[j] = 2 * (int)t + j;
        for (int b = 0; b < 4; ++b) s.waves[j][b] = (4 * j + b + margin / 64) & 7;     // the wave whose owned block is 4 j + b
    }
    s.zero_first = 2 * n_tiles + (int)t;
    s.zero_step = n_tiles;
    return s;
}

// The backward layers below the top in one launch (grand_bwd_narrow_block_kernel, gadapt_narrow_bwd_block.inc): K <= 3 consecutive fused
// stages [S_l + T_{l-1}], l descending, on the same 512-node tiles.  S_l of node j reads the g rows and {alpha dt, ds} pairs stage s - 1
// left for j's OUT-neighbours, which lie within h (the halo of the source-ordered CSR) of j's aligned 32-node group: stage s runs on the
// owned range widened by (K - 1 - s) h - gadapt_block_range with the stage for the layer.  There is no load range beyond stage 0's (it
// reads what the launch above left in global memory), so the frame margin is that of K - 1 halos: at most 128 rows, 768 frame rows.
//   gadapt_bwd_block_margin     rows of the frame in front of the owned range (a multiple of 64: the owned range starts on a wave block);
//   gadapt_bwd_block_pair_cap   {alpha dt, ds} pairs the LDS buffer holds that stage s - 1 fills for stage s (s >= 1): the pairs whose
//                               source lies in stage s's range, at most 8 per row - stage 1 of three has 512 + 2 * 64 rows at most, every
//                               later stage (and stage 1 of two) the 512 owned ones;
//   gadapt_bwd_block_groups     the launches of n_stages = L - 1 fused stages: groups of three, a remainder of one avoided (4 = 2 + 2), so
//                               that every launch has at least one stage boundary to save.  Returns the size of the group that starts at
//                               stage `done` (0 when none is left).
#define GADAPT_NARROW_BWD_BLOCK_STAGES 3
GADAPT_PLAN_FN int gadapt_bwd_block_margin(int halo, int K) { return gadapt_block_frame_margin(halo, K - 1); }
GADAPT_PLAN_FN int gadapt_bwd_block_pair_cap(int K, int s) { return 8 * (GADAPT_NARROW_TILE + ((K == 3 && s == 1) ? 128 : 0)); }
GADAPT_PLAN_FN int gadapt_bwd_block_groups(int n_stages, int done) {
    const int left = n_stages - done;
    if (left <= 0) return 0;
    if (left <= GADAPT_NARROW_BWD_BLOCK_STAGES) return left;
    return left == GADAPT_NARROW_BWD_BLOCK_STAGES + 1 ? 2 : GADAPT_NARROW_BWD_BLOCK_STAGES;
}

#endif  // GADAPT_BLOCK_PLAN_H
