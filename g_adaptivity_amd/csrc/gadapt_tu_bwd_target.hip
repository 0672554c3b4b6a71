// gadapt_tu_bwd_target.hip - backward target pass launches (autograd of src/GRAND_plus.py:225-343: softmax backward, dP,
// weight-gradient partials, dxd): the tiled kernel and the compact layer-0 kernel (gadapt_bwd_target.inc).  One translation
// unit of libgadapt_hip.so (see gadapt_internal.h).
#include "gadapt_internal.h"
#include "gadapt_bwd_target.inc"
#include "gadapt_narrow_bwd.inc"
#include "gadapt_narrow_bwd_block.inc"

// The slab holds one row per workgroup of a target pass: every target launch of a block at hidden size C uses this grid, so every
// row is visited (gadapt_slab_rows_c)
template <int C> static int target_grid(int64_t n_nodes) { return grid_for(tiles_for<C>(n_nodes), resident_blocks_bwd_t<C>(GADAPT_BWD_T_MAX_BLOCKS)); }
int gadapt_slab_rows_c(int64_t n_nodes, int c) { GADAPT_DISPATCH_C(c, target_grid<CC>(n_nodes)); }

// The kernel arguments of a target pass of layer b at hidden size C.  The tiled kernels read the tile metadata (meta) and, compact,
// a g_in of row pitch b.g_stride (0 = C); the one-node-per-lane kernels (compact layer 0, narrow route) read the ELL table.
template <int C> static BwdTArgs target_args(const gadapt_graph* g, const LayerBwd& b, int n_tiles, bool tiled) {
    BwdTArgs pt{b.x_in, b.g_in, b.alpha, b.a, b.lp, g->rowptr_t, g->col_t, g->tpos_s, tiled ? meta_for<Cfg<C>::TM>(g->meta_t) : nullptr,
                reinterpret_cast<float2*>(b.edge_ws), b.dxd, b.slab, b.sums_out, g->n_nodes, n_tiles, b.accumulate, b.residual_only, g->n_edges, nullptr, b.g_cols};
    pt.sums_sc_out = b.sums_sc_out;
    pt.c = C;
    pt.g_stride = b.g_stride ? b.g_stride : C;
    pt.sums_partials = b.sums_partials;
    pt.slab_packed = b.slab_packed ? 1 : 0;
    return pt;
}

template <int C> static int launch_bwd_target(const gadapt_graph* g, const LayerBwd& b, hipStream_t st) {
    using K = Cfg<C>;
    const int g_cols = b.g_cols, x_cols = b.x_cols, out4 = b.out4, want_source = b.g_out != nullptr;
    float* const sums_out = b.sums_out;
    if (g_cols < 0 || g_cols > 4) return fail(GADAPT_E_BADARG, "compact upstream gradient: 1..4 columns");
    if ((x_cols != 0 && x_cols != 4) || (x_cols && (g_cols || want_source)))
        return fail(GADAPT_E_BADARG, "compact layer input: 4 columns, layer 0 of a block of >= 2 layers, no d x0");
    if (x_cols && b.residual_only) return fail(GADAPT_E_BADARG, "compact layer input: Euler-step layers only");
    if (b.slab_packed && (!x_cols || sums_out)) return fail(GADAPT_E_BADARG, "packed slab rows: the compact layer-0 launch with fixed steps and temperature");
    if (out4 && (!want_source || x_cols || b.residual_only || C < 8 || (g_cols && sums_out)))
        return fail(GADAPT_E_BADARG, "4-column backward: a layer with a gradient to pass on, hidden >= 8, not compact-g with d dt / d scale");
    BwdTArgs pt = target_args<C>(g, b, tiles_for<C>(g->n_nodes), true);
#ifdef GADAPT_STAMPS
    pt.stamps = g_stamp_buf ? g_stamp_buf + 1024 * 32 : nullptr;
#endif
    const dim3 grid(target_grid<C>(g->n_nodes));
    if (x_cols) {                                                // layer 0 on the compact [N,4] input: one node per lane
        ProfScope prof(1, st, 2);
        pt.ell = g->ell_t;
        if (sums_out && pt.sums_sc_out) hipLaunchKernelGGL((grand_bwd_target_compact_kernel<2>), grid, dim3(256), 0, st, pt);
        else if (sums_out) hipLaunchKernelGGL((grand_bwd_target_compact_kernel<1>), grid, dim3(256), 0, st, pt);
        else if (pt.ell) hipLaunchKernelGGL((grand_bwd_target_compact_kernel<0, true>), grid, dim3(256), 0, st, pt);
        else hipLaunchKernelGGL((grand_bwd_target_compact_kernel<0>), grid, dim3(256), 0, st, pt);
        return check_launch("grand_bwd_target_compact_kernel");
    }
    constexpr int lds_t = K::lds_bytes(1, K::RING_T + 1, 1);
    ProfScope prof(1, st, (g_cols ? 1 : 0) | (out4 ? 8 : 0));
    // instantiations: SUMS 0 / 1 (d dt: learn_step) / 2 (d dt and d score_scale), each plain, with the compact upstream
    // gradient (GC) and - hidden >= 8 - with the 4-column dxd (D4)
    auto go = [&](auto kern) { allow_lds(kern, lds_t); hipLaunchKernelGGL(kern, grid, dim3(K::NT), lds_t, st, pt); };
    auto pick = [&](auto sums_tag) {
        constexpr int S = decltype(sums_tag)::value;
        if (out4) {
            if constexpr (C >= 8) {
                if (!g_cols) go(grand_bwd_target_kernel<C, S, false, true>);
                else if constexpr (S == 0) go(grand_bwd_target_kernel<C, 0, true, true>);   // GC + D4 + SUMS: not built (gadapt_block_backward)
            }
        } else if (g_cols) {
            go(grand_bwd_target_kernel<C, S, true>);
        } else {
            go(grand_bwd_target_kernel<C, S>);
        }
    };
    if (sums_out && pt.sums_sc_out) pick(IntTag<2>{}); else if (sums_out) pick(IntTag<1>{}); else pick(IntTag<0>{});
    return check_launch("grand_bwd_target_kernel");
}

int gadapt_launch_bwd_target_c(int c, const gadapt_graph* g, const LayerBwd& b, hipStream_t st) { GADAPT_DISPATCH_C(c, launch_bwd_target<CC>(g, b, st)); }

template <int C> static int occupancy_bwd_target() {
    int n = -1;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, grand_bwd_target_kernel<C, 0>, Cfg<C>::NT, Cfg<C>::lds_bytes(1, Cfg<C>::RING_T + 1, 1));
    return n;
}
int gadapt_occupancy_bwd_target_c(int c) { GADAPT_DISPATCH_C(c, occupancy_bwd_target<CC>()); }

// The narrow route's arguments of a target pass: [N,4] rows of pitch 4, no d dt / d scale, Euler-step layers, the ELL table
static BwdTArgs narrow_target_args(const gadapt_graph* g, const LayerBwd& b) {
    LayerBwd n = b;
    n.sums_out = n.sums_sc_out = nullptr; n.residual_only = 0; n.g_stride = 4; n.sums_partials = 0;
    BwdTArgs pt = target_args<64>(g, n, tiles_for<64>(g->n_nodes), false);
    pt.ell = g->ell_t;
    return pt;
}

// narrow route, layers 1..L-1 (grand_bwd_target_narrow_kernel): x_in, dxd [N,4]; g_in [N,4] or the compact [N,g_cols] top gradient.  The
// slab row layout and grid of every other target-pass launch of the block (hidden c), so the layer-0 launch accumulates onto these rows.
int gadapt_launch_bwd_target_narrow_c(int c, const gadapt_graph* g, const LayerBwd& b, hipStream_t st) {
    if (c != 64 || !g->ell_t || !g->tpos_s || b.g_cols < 0 || b.g_cols > 4) return fail(GADAPT_E_BADARG, "narrow target pass: hidden 64, ELL graph, 0..4 g columns");
    const BwdTArgs pt = narrow_target_args(g, b);
    ProfScope prof(1, st, b.g_cols ? 3 : 2);                   // compact input (and compact upstream gradient at the top layer)
    hipLaunchKernelGGL(grand_bwd_target_narrow_kernel, dim3(target_grid<64>(g->n_nodes)), dim3(256), 0, st, pt);
    return check_launch("grand_bwd_target_narrow_kernel");
}

// narrow route, fused launch (grand_bwd_target_fused_narrow_kernel, gadapt_narrow_bwd.inc): the source pass of layer l (src: x_in, g_in [N,4]
// or - g_cols > 0 - the compact [N,g_cols] top gradient, a / p0, g_out; the pairs in edge_in; its dxd row is read from tgt.dxd) and, in the
// same lane, the target pass of layer l-1 (tgt: x_in, alpha, a, lp, dxd, slab) on the result.  layer0 = 0: g_out [N,4], dxd and the pairs of
// layer l-1 (edge_out, NOT edge_in: lanes of one launch read one and scatter into the other) are written; layer0 = 1 (l-1 = 0): slab
// partials only.  Grid and slab rows of every target launch.
int gadapt_launch_bwd_fused_narrow_c(int c, const gadapt_graph* g, const LayerBwd& src, const LayerBwd& tgt, const float* edge_in, float* edge_out,
                                     int layer0, hipStream_t st) {
    if (c != 64 || !g->ell_t || !g->tpos_s || !g->ell_s || !g->rowptr_s || !g->col_s || src.g_cols < 0 || src.g_cols > 4)
        return fail(GADAPT_E_BADARG, "fused narrow backward: hidden 64, ELL graph, 0..4 g columns");
    if (!layer0 && (!src.g_out || !edge_out || edge_out == edge_in)) return fail(GADAPT_E_BADARG, "fused narrow backward: a second edge buffer and g_out above layer 0");
    LayerBwd t = tgt;
    t.g_in = nullptr; t.edge_ws = edge_out; t.g_cols = 0;
    BwdFusedNarrowArgs pf{};
    pf.t = narrow_target_args(g, t);
    pf.x_src = src.x_in; pf.g_in = src.g_in; pf.edge_in = edge_in; pf.A_src = src.a; pf.p0_src = src.p0;
    pf.rowptr_s = g->rowptr_s; pf.col_s = g->col_s; pf.ell_s = g->ell_s;
    pf.g_out = src.g_out; pf.g_cols = src.g_cols;
    ProfScope prof(1, st, 2);                                   // a target-pass launch on compact input (the source pass rides in it)
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(target_grid<64>(g->n_nodes)), dim3(256), 0, st, pf); };
    if (layer0) { if (src.g_cols) go(grand_bwd_target_fused_narrow_kernel<true, true>); else go(grand_bwd_target_fused_narrow_kernel<true, false>); }
    else { if (src.g_cols) go(grand_bwd_target_fused_narrow_kernel<false, true>); else go(grand_bwd_target_fused_narrow_kernel<false, false>); }
    return check_launch("grand_bwd_target_fused_narrow_kernel");
}

// narrow route, K = 2 or 3 consecutive fused stages [S_l + T_{l-1}] in one launch (grand_bwd_narrow_block_kernel, gadapt_narrow_bwd_block.inc):
// one 512-thread workgroup per 512-node tile, halo of the source-ordered CSR (32 or 64; the caller has it from the graph's registration).
// Everything is checked before the launch.  layer0 = 1: the last stage's target half is layer 0, the launch writes slab rows only;
// layer0 = 0: its last stage also stores g_out, dxd_out and the pairs into edge_out for the nodes a tile owns - three buffers other than
// the ones stage 0 reads.
int gadapt_launch_bwd_narrow_block_c(int c, const gadapt_graph* g, const BwdBlockLaunch& b, hipStream_t st) {
    if (c != 64 || !g || !g->ell_t || !g->tpos_s || !g->ell_s || !g->rowptr_s || !g->rowptr_t || g->n_edges <= 0 || g->n_nodes <= 0 ||
        (b.halo != 32 && b.halo != 64) || b.K < 2 || b.K > GADAPT_NARROW_BWD_BLOCK_STAGES || b.g_cols < 0 || b.g_cols > 4)
        return fail(GADAPT_E_BADARG, "narrow block backward: hidden 64, ELL graph with edges, halo 32 or 64, 2..3 stages, 0..4 g columns");
    if (!b.x_src0 || !b.alpha0 || !b.lp0 || !b.a || !b.p0 || !b.g_in || !b.edge_in || !b.dxd_in || !b.slab ||
        b.slot_stride < 4 * (int64_t)g->n_nodes || b.alpha_stride < g->n_edges)
        return fail(GADAPT_E_BADARG, "narrow block backward: layer slots, alpha, {dt, scale}, coefficients, the buffers of the launch above, the slab");
    if (!b.layer0 && (!b.g_out || !b.edge_out || !b.dxd_out || b.g_out == b.g_in || b.edge_out == b.edge_in || b.dxd_out == b.dxd_in))
        return fail(GADAPT_E_BADARG, "narrow block backward: above layer 0 the last stage stores g, dxd and pairs to buffers other than the ones read");
    if (b.slab_rows != gadapt_slab_rows_c(g->n_nodes, c) || !gadapt_narrow_row_is_one_range(g->n_nodes, b.slab_rows))
        return fail(GADAPT_E_BADARG, "narrow block backward: the slab of the target launches, one 256-node range per row");
    BwdBlockArgs q{};
    q.x_src0 = b.x_src0; q.slot_stride = b.slot_stride; q.alpha0 = b.alpha0; q.alpha_stride = b.alpha_stride; q.lp0 = b.lp0;
    q.A = b.a; q.p0 = b.p0; q.g_in = b.g_in; q.edge_in = reinterpret_cast<const float2*>(b.edge_in); q.dxd_in = b.dxd_in;
    q.g_out = b.g_out; q.edge_out = reinterpret_cast<float2*>(b.edge_out); q.dxd_out = b.dxd_out;
    q.rowptr_t = g->rowptr_t; q.ell_t = g->ell_t; q.tpos = g->tpos_s; q.rowptr_s = g->rowptr_s; q.ell_s = g->ell_s;
    q.slab = b.slab;
    q.n_nodes = g->n_nodes; q.n_edges = g->n_edges; q.K = b.K; q.halo = b.halo; q.c = c; q.g_cols = b.g_cols; q.slab_rows = b.slab_rows;
    const int grid = (g->n_nodes + GADAPT_NARROW_TILE - 1) / GADAPT_NARROW_TILE;
    ProfScope prof(1, st, 2 | 32);                              // a target-pass launch on compact input, bit 5: several layers in the launch
    auto go = [&](auto kern) { allow_lds(kern, NBB_LDS_BYTES); hipLaunchKernelGGL(kern, dim3(grid), dim3(NBB_NT), NBB_LDS_BYTES, st, q); };
    if (b.layer0) { if (b.g_cols) go(grand_bwd_narrow_block_kernel<true, true>); else go(grand_bwd_narrow_block_kernel<true, false>); }
    else { if (b.g_cols) go(grand_bwd_narrow_block_kernel<false, true>); else go(grand_bwd_narrow_block_kernel<false, false>); }
    return check_launch("grand_bwd_narrow_block_kernel");
}
