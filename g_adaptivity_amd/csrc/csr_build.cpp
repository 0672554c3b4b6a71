// csr_build.cpp - one-time host build of the two CSR orientations of a batched mesh graph.
//
// Replaces the per-call gather/scatter index handling of PyG's MessagePassing.propagate
// (/root/reference/src/GRAND_plus.py:233-234) - see include/gadapt_hip.h.  Stable counting
// sorts: edges keep their input order inside a row, so the summation order of every
// kernel is a pure function of the caller's edge list.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "gadapt_hip.h"
#include "gadapt_block_plan.h"
#include "gadapt_narrow_plan.h"
#include "gadapt_tail_plan.h"

extern "C" int gadapt_csr_build_host(const int64_t* src, const int64_t* dst, int64_t n_edges, int64_t n_nodes,
                                     int32_t* rowptr_t, int32_t* col_t, int32_t* eid_t,
                                     int32_t* rowptr_s, int32_t* col_s, int32_t* perm_s, int32_t* tpos_s) {
    if (!src || !dst || n_edges < 0 || n_nodes <= 0 || n_nodes > INT32_MAX || n_edges > INT32_MAX ||
        !rowptr_t || !col_t || !eid_t || !rowptr_s || !col_s || !perm_s || !tpos_s)
        return GADAPT_E_BADARG;
    const int64_t N = n_nodes, E = n_edges;
    for (int64_t i = 0; i <= N; ++i) rowptr_t[i] = rowptr_s[i] = 0;
    for (int64_t e = 0; e < E; ++e) {
        if (src[e] < 0 || src[e] >= N || dst[e] < 0 || dst[e] >= N) return GADAPT_E_RANGE;
        rowptr_t[dst[e] + 1]++;
        rowptr_s[src[e] + 1]++;
    }
    for (int64_t i = 0; i < N; ++i) { rowptr_t[i + 1] += rowptr_t[i]; rowptr_s[i + 1] += rowptr_s[i]; }
    std::vector<int32_t> fill_t(rowptr_t, rowptr_t + N), fill_s(rowptr_s, rowptr_s + N);
    // by target, stable in input order
    for (int64_t e = 0; e < E; ++e) {
        const int32_t slot = fill_t[dst[e]]++;
        col_t[slot] = (int32_t)src[e];
        eid_t[slot] = (int32_t)e;
    }
    // by source, stable in TARGET-SLOT order (so perm_s is monotone inside a row where possible)
    for (int32_t slot = 0; slot < (int32_t)E; ++slot) {
        const int64_t e = eid_t[slot];
        const int32_t s = fill_s[src[e]]++;
        col_s[s] = (int32_t)dst[e];
        perm_s[s] = slot;
        tpos_s[slot] = s;
    }
    return GADAPT_OK;
}

// Per-tile staging metadata (see include/gadapt_hip.h): 4 ints per tile of `tile_rows` consecutive rows.
extern "C" int gadapt_tile_meta_host(const int32_t* rowptr, const int32_t* col, int64_t n_nodes, int tile_rows, int32_t* meta_out) {
    if (!rowptr || !col || !meta_out || n_nodes <= 0 || tile_rows <= 0) return GADAPT_E_BADARG;
    const int64_t n_tiles = (n_nodes + tile_rows - 1) / tile_rows;
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int64_t lo = t * tile_rows, hi = (lo + tile_rows < n_nodes) ? lo + tile_rows : n_nodes;
        int32_t longest = 0;
        for (int64_t i = lo; i < hi; ++i) { const int32_t d = rowptr[i + 1] - rowptr[i]; if (d > longest) longest = d; }
        // windowed: every neighbour of the tile's rows lies in the slabs t-1, t, t+1
        const int64_t wlo = (t - 1) * tile_rows, whi = (t + 2) * tile_rows;
        int32_t windowed = 1;
        for (int32_t e = rowptr[lo]; e < rowptr[hi]; ++e)
            if (col[e] < wlo || col[e] >= whi) { windowed = 0; break; }
        meta_out[4 * t + 0] = rowptr[lo];
        meta_out[4 * t + 1] = rowptr[hi] - rowptr[lo];
        meta_out[4 * t + 2] = longest;
        meta_out[4 * t + 3] = windowed;
    }
    return GADAPT_OK;
}

// ELL-8 copy of one CSR orientation for the wide kernels (see include/gadapt_hip.h): row i -> ell[8i..8i+7], unused
// entries -1, rows padded to a multiple of 256 (rows longer than 8 are cut: such a graph never qualifies).  *max_deg_out = the
// longest row if the orientation qualifies for the 384-row window (every row <= 8 entries and every neighbour of node i
// inside rows [256*(i/256) - 64, 256*(i/256) + 320)), else 0.
extern "C" int gadapt_ell_build_host(const int32_t* rowptr, const int32_t* col, int64_t n_nodes, int32_t* ell_out, int32_t* max_deg_out) {
    if (!rowptr || !col || !ell_out || !max_deg_out || n_nodes <= 0) return GADAPT_E_BADARG;
    const int64_t n_pad = (n_nodes + 255) / 256 * 256;
    for (int64_t k = 0; k < n_pad * 8; ++k) ell_out[k] = -1;
    for (int64_t i = 0; i < n_nodes; ++i) {
        const int32_t e0 = rowptr[i], d = rowptr[i + 1] - e0;
        for (int32_t k = 0; k < d && k < 8; ++k) ell_out[8 * i + k] = col[e0 + k];
    }
    return gadapt_wide_window_host(rowptr, col, n_nodes, 256, 64, 8, max_deg_out);
}

// The wide kernels' locality test for steps of `step` nodes and a window of step + 2 * halo rows: *max_deg_out = the longest row if every
// row has at most max_row entries and every neighbour of node i lies in rows [step*(i/step) - halo, step*(i/step) + step + halo), else 0.
extern "C" int gadapt_wide_window_host(const int32_t* rowptr, const int32_t* col, int64_t n_nodes, int step, int halo, int max_row, int32_t* max_deg_out) {
    if (!rowptr || !col || !max_deg_out || n_nodes <= 0 || step <= 0 || halo < 0 || max_row <= 0) return GADAPT_E_BADARG;
    int32_t longest = 0;
    bool ok = true;
    for (int64_t i = 0; i < n_nodes && ok; ++i) {
        const int32_t e0 = rowptr[i], d = rowptr[i + 1] - e0;
        if (d > max_row) { ok = false; break; }
        if (d > longest) longest = d;
        const int64_t lo = i / step * step - halo, hi = lo + step + 2 * (int64_t)halo;
        for (int32_t k = 0; k < d; ++k) {
            const int32_t j = col[e0 + k];
            if (j < lo || j >= hi) { ok = false; break; }
        }
    }
    *max_deg_out = ok ? longest : 0;
    return GADAPT_OK;
}

// Halo of the narrow route's one-launch forward (gadapt_block_plan.h): the smallest h in {32, 64} such that every row of the
// target-ordered CSR has at most 8 entries and every in-neighbour of node i lies in [32*(i/32) - h, 32*(i/32) + 32 + h); 0 when neither
// does (the graph keeps the per-layer launches).  Row-major meshes up to 32 nodes wide give 32, up to 64 wide 64.
extern "C" int gadapt_narrow_block_halo_host(const int32_t* rowptr, const int32_t* col, int64_t n_nodes, int32_t* halo_out) {
    if (!rowptr || !col || !halo_out || n_nodes <= 0) return GADAPT_E_BADARG;
    *halo_out = 0;
    for (int h = 32; h <= 64; h += 32) {
        int32_t md = 0;
        if (int rc = gadapt_wide_window_host(rowptr, col, n_nodes, 32, h, 8, &md)) return rc;
        if (md > 0) { *halo_out = h; break; }
    }
    return GADAPT_OK;
}

// Compute range [*lo_out, *hi_out) of layer `layer` of tile `tile` in a group of n_layers layers (layer = -1: the load range):
// gadapt_block_range, the arithmetic the kernel uses.
extern "C" int gadapt_narrow_block_range_host(int64_t n_nodes, int halo, int n_layers, int64_t tile, int layer, int64_t* lo_out, int64_t* hi_out) {
    if (n_nodes <= 0 || (halo != 32 && halo != 64) || n_layers < 1 || n_layers > GADAPT_NARROW_BLOCK_LAYERS || layer < -1 || layer >= n_layers ||
        tile < 0 || tile * GADAPT_NARROW_TILE >= n_nodes || !lo_out || !hi_out)
        return GADAPT_E_BADARG;
    gadapt_block_range(n_nodes, halo, n_layers, tile, layer, lo_out, hi_out);
    return GADAPT_OK;
}

// The slab rows tile `tile` owes when the top layer's target pass runs in the launch: gadapt_block_slab_plan / gadapt_block_owned_block,
// the arithmetic the kernel uses.  plan_out: rows[2], waves[2][4], zero_first, zero_step.
extern "C" int gadapt_narrow_block_slab_plan_host(int64_t n_nodes, int halo, int n_layers, int64_t tile, int32_t* plan_out) {
    if (n_nodes <= 0 || (halo != 32 && halo != 64) || n_layers < 1 || n_layers > GADAPT_NARROW_BLOCK_LAYERS || tile < 0 ||
        tile * GADAPT_NARROW_TILE >= n_nodes || !plan_out)
        return GADAPT_E_BADARG;
    const gadapt_block_slab s = gadapt_block_slab_plan(n_nodes, gadapt_block_frame_margin(halo, n_layers), tile);
    for (int j = 0; j < 2; ++j) {
        plan_out[j] = s.rows[j];
        for (int b = 0; b < 4; ++b) plan_out[2 + 4 * j + b] = s.waves[j][b];
    }
    plan_out[10] = s.zero_first; plan_out[11] = s.zero_step;
    return GADAPT_OK;
}
extern "C" int gadapt_narrow_block_owned_block_host(int halo, int n_layers, int wave) {
    if ((halo != 32 && halo != 64) || n_layers < 1 || n_layers > GADAPT_NARROW_BLOCK_LAYERS || wave < 0 || wave >= GADAPT_NARROW_TILE / 64) return -1;
    return gadapt_block_owned_block(gadapt_block_frame_margin(halo, n_layers), wave);
}

// The backward block launch (gadapt_narrow_bwd_block.inc): compute range [*lo_out, *hi_out) of fused stage `stage` of tile `tile` in a launch
// of n_stages stages (gadapt_block_range on the halo of the source-ordered CSR), and - pair_cap_out, nullable - the {alpha dt, ds} pairs the
// LDS buffer holds that the stage before fills for this one (0 for stage 0, which reads global memory): the arithmetic the kernel uses.
extern "C" int gadapt_narrow_bwd_block_range_host(int64_t n_nodes, int halo, int n_stages, int64_t tile, int stage, int64_t* lo_out, int64_t* hi_out,
                                                  int32_t* pair_cap_out) {
    if (n_nodes <= 0 || (halo != 32 && halo != 64) || n_stages < 2 || n_stages > GADAPT_NARROW_BWD_BLOCK_STAGES || stage < 0 || stage >= n_stages ||
        tile < 0 || tile * GADAPT_NARROW_TILE >= n_nodes || !lo_out || !hi_out)
        return GADAPT_E_BADARG;
    gadapt_block_range(n_nodes, halo, n_stages, tile, stage, lo_out, hi_out);
    if (pair_cap_out) *pair_cap_out = stage ? gadapt_bwd_block_pair_cap(n_stages, stage) : 0;
    return GADAPT_OK;
}
// ... the rows of its frame in front of the owned range (-1: bad argument), and the stages of the launch that starts at fused stage `done`
// of n_stages = L - 1 (0: none left)
extern "C" int gadapt_narrow_bwd_block_margin_host(int halo, int n_stages) {
    if ((halo != 32 && halo != 64) || n_stages < 2 || n_stages > GADAPT_NARROW_BWD_BLOCK_STAGES) return -1;
    return gadapt_bwd_block_margin(halo, n_stages);
}
extern "C" int gadapt_narrow_bwd_block_groups_host(int n_stages, int done) {
    if (n_stages < 2 || done < 0) return -1;
    return gadapt_bwd_block_groups(n_stages, done);
}

// The launch sequence of a narrow step (gadapt_narrow_plan.h), the pure function: facts [GADAPT_NARROW_FACTS] and switches [4] in the
// order of the structs' members -> the plan as int32 words (layout: include/gadapt_hip.h).  Returns the words written.
extern "C" int gadapt_narrow_step_plan_host(const int64_t* facts, const int32_t* switches, int32_t* plan_out, int cap) {
    if (!facts || !switches || !plan_out || cap < 0) return GADAPT_E_BADARG;
    const int64_t* v = facts;
    if (v[3] < 1 || v[3] > INT32_MAX || !gadapt_narrow_sizes_ok(v[0], v[1], (int)v[2])) return GADAPT_E_BADARG;
    for (int k = 2; k < GADAPT_NARROW_FACTS; ++k) if (v[k] < 0 || v[k] > INT32_MAX) return GADAPT_E_BADARG;
    if ((v[5] != 0 && v[5] != 32 && v[5] != 64) || (v[6] != 0 && v[6] != 32 && v[6] != 64)) return GADAPT_E_BADARG;
    const gadapt_narrow_facts f = {v[0], v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6], (int)v[7], (int)v[8], (int)v[9], (int)v[10], (int)v[11],
                                   (int)v[12], (int)v[13], (int)v[14], (int)v[15], (int)v[16], (int)v[17], (int)v[18], (int)v[19], (int)v[20], (int)v[21]};
    const gadapt_narrow_switches s = {switches[0], switches[1] != 0, switches[2] != 0, switches[3] != 0};
    if (s.fwd < 0 || s.fwd > 2) return GADAPT_E_BADARG;
    const gadapt_narrow_plan p = gadapt_narrow_plan_of(&f, &s);
    const int n = gadapt_narrow_plan_write(&p, plan_out, cap);
    return n < 0 ? GADAPT_E_BADARG : n;
}

// The spread step tail of the narrow route (gadapt_tail_plan.h; step_tail_narrow_spread_kernel): the arithmetic the kernel and its launcher
// use.  plan_out: rows per parameter workgroup, threads per workgroup, parameter workgroups, slots per thread, workgroups of the launch
// and tickets taken with (has_loss != 0) or without loss partials.
extern "C" int gadapt_narrow_tail_plan_host(int has_loss, int32_t* plan_out) {
    if (!plan_out) return GADAPT_E_BADARG;
    plan_out[0] = GADAPT_NARROW_TAIL_ROWS; plan_out[1] = GADAPT_NARROW_TAIL_THREADS; plan_out[2] = gadapt_narrow_tail_wgs();
    plan_out[3] = gadapt_narrow_tail_slots(); plan_out[4] = gadapt_narrow_tail_grid(has_loss); plan_out[5] = gadapt_narrow_tail_tickets(has_loss);
    return GADAPT_OK;
}
// rows of parameter workgroup wg (-1: no such workgroup)
extern "C" int gadapt_narrow_tail_rows_host(int wg) {
    if (wg < 0 || wg >= gadapt_narrow_tail_wgs()) return -1;
    return gadapt_narrow_tail_rows_of(wg);
}
// out3 = {entry of the flat bucket or -1, row within the workgroup, place in the row} of (wg, thread, slot); {wg, thread, slot} of entry e
extern "C" int gadapt_narrow_tail_entry_host(int wg, int thread, int slot, int32_t* out3) {
    if (wg < 0 || wg >= gadapt_narrow_tail_wgs() || thread < 0 || thread >= GADAPT_NARROW_TAIL_THREADS || slot < 0 ||
        slot >= gadapt_narrow_tail_slots() || !out3)
        return GADAPT_E_BADARG;
    const gadapt_tail_entry t = gadapt_narrow_tail_entry(wg, thread, slot);
    out3[0] = t.e; out3[1] = t.ri; out3[2] = t.k;
    return GADAPT_OK;
}
extern "C" int gadapt_narrow_tail_owner_host(int e, int32_t* out3) {
    if (e < 0 || e >= GADAPT_NARROW_TAIL_C * GADAPT_NARROW_TAIL_ROW_ENTRIES || !out3) return GADAPT_E_BADARG;
    const gadapt_tail_owner o = gadapt_narrow_tail_owner(e);
    out3[0] = o.wg; out3[1] = o.thread; out3[2] = o.slot;
    return GADAPT_OK;
}
