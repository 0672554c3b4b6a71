// gadapt_tu_fwd.hip - forward layer launches: x' = x + dt (sum_j alpha_ij x_j - x) (src/GRAND_plus.py:225-343 + src/GNN.py:288-291),
// tiled kernel for every hidden size and graph (gadapt_fwd.inc), wide kernel for hidden 64 on row-major mesh batches
// (gadapt_wide.inc).  One translation unit of libgadapt_hip.so (see gadapt_internal.h).
#include "gadapt_internal.h"
#include "gadapt_fwd.inc"
#include "gadapt_wide.inc"
#include "gadapt_narrow_fwd.inc"

// The wide kernels take over for hidden size 64 when the graph qualifies; GADAPT_WIDE=0 in the environment keeps the tiled
// kernels (A/B runs and the tests of the tiled path).
static bool wide_enabled() {
    static const bool on = [] { const char* e = getenv("GADAPT_WIDE"); return !(e && e[0] == '0'); }();
    return on;
}
static inline int wide_grid(int n_steps) {
    int g = (n_steps + 7) & ~7;
    if (g > 256) g = 256;                                       // one 512-thread workgroup per CU
    return g;
}
// Four-wave workgroups on steps of 128 nodes (wide::W<false, 4>): when the 256-node steps would leave half of the CUs without a
// workgroup and the graph qualifies for the narrower window (gadapt_graph::wide_half_deg_t)
static bool wide_half(const gadapt_graph* g) {
    return g->wide_deg_t > 0 && g->wide_half_deg_t > 0 && (g->n_nodes + wide::STEP - 1) / wide::STEP <= 128;
}
// The kernel arguments of a wide or narrow forward launch over n_steps steps; kmax: the longest in-row of the geometry the wide launch
// picks (512-row window / four-wave workgroups / default)
static wide::FwdArgs wide_fwd_args(const gadapt_graph* g, const LayerFwd& f, int n_steps) {
    const bool big = g->wide_deg_t <= 0, half = !big && wide_half(g);
    return wide::FwdArgs{f.x_in, f.x_out, f.a, f.p0, f.lp, g->ell_t, g->rowptr_t, f.alpha_out, g->n_nodes, n_steps, f.residual_only,
                         big ? g->wide_big_deg_t : (half ? g->wide_half_deg_t : g->wide_deg_t), nullptr, f.x_top4};
}
// The extras of a fused step into a launch's arguments.  Which parts a launch takes is its caller's condition: the node fields, the
// in-kernel coefficients (wide::FwdArgs only), the loss - and then the number of loss partials the launch writes.
template <typename Args> static void put_extra(Args& p, const FwdExtra& ex, bool fields, bool coeffs, bool loss, int n_partials) {
    if (fields) { p.fs = ex.fs; p.x0c = ex.x0c; }
    if constexpr (std::is_same<Args, wide::FwdArgs>::value) {
        if (coeffs) { p.cw = ex.cw; p.a_out = ex.a_out; p.p0_out = ex.p0_out; }
    }
    if (loss) { p.loss = ex.loss; if (ex.n_partials_out) *ex.n_partials_out = n_partials; }
}

static int launch_wide_fwd(const gadapt_graph* g, const LayerFwd& f, hipStream_t st) {
    const bool big = g->wide_deg_t <= 0;                        // 512-row window (meshes with up to 128 nodes per row)
    const bool half = !big && wide_half(g);
    const int step = half ? wide::STEP_HALF : wide::STEP, nwv = half ? 4 : 8;
    const int n_steps = (g->n_nodes + step - 1) / step;
    const int x_cols = f.x_cols;
    wide::FwdArgs p = wide_fwd_args(g, f, n_steps);
#ifdef GADAPT_STAMPS
    p.stamps = g_stamp_buf;
#endif
    if (const FwdExtra* ex = f.extra) {
        if (x_cols && half && ex->cw) return fail(GADAPT_E_BADARG, "wide forward on four-wave workgroups: the coefficients are given (gadapt_forward_computes_coeffs)");
        put_extra(p, *ex, x_cols != 0, x_cols && !half, !f.x_out && ex->loss.target, nwv * wide_grid(n_steps));
    }
    ProfScope prof(0, st, (x_cols ? 2 : 0) | (f.x_out ? 0 : 4));
    auto go = [&](auto kern, int lds) { allow_lds(kern, lds); hipLaunchKernelGGL(kern, dim3(wide_grid(n_steps)), dim3(64 * nwv), lds, st, p); };
    const bool head = !f.x_out && !x_cols;                      // head-only output: its own instantiation (aggregates one chunk)
    // narrow route (compact input AND compact output, gadapt_block_forward_narrow): the last layer's launch also seeds the loss
    const bool xloss = x_cols && !f.x_out && p.loss.target;
    auto pick = [&](auto big_tag, auto nwv_tag) {               // one geometry: its four instantiations
        constexpr bool BIG = decltype(big_tag)::value != 0;
        constexpr int NWV = decltype(nwv_tag)::value, lds = wide::fwd_lds_bytes<BIG, NWV>();
        if (xloss) go(wide::fwd_kernel<true, BIG, true, NWV>, lds);
        else if (x_cols) go(wide::fwd_kernel<true, BIG, false, NWV>, lds);
        else if (head) go(wide::fwd_kernel<false, BIG, true, NWV>, lds);
        else go(wide::fwd_kernel<false, BIG, false, NWV>, lds);
    };
    if (big) pick(IntTag<1>{}, IntTag<8>{}); else if (half) pick(IntTag<0>{}, IntTag<4>{}); else pick(IntTag<0>{}, IntTag<8>{});
    return check_launch("wide::fwd_kernel");
}

static bool wide_takes(const gadapt_graph* g) {
    return g->ell_t && (g->wide_deg_t > 0 || (g->wide_big_deg_t > 0 && g->wide_big_deg_t <= 7)) && wide_enabled();
}
// 1: the layer-0 launch of a fused training step on this graph at this hidden size is the wide kernel, which computes the composite
// coefficients itself (FwdExtra::cw); 0: they must be given (a coefficient launch ends the step)
int gadapt_forward_computes_coeffs_c(const gadapt_graph* g, int c) { return (c == 64 && g && wide_takes(g) && !wide_half(g)) ? 1 : 0; }
// 1: the narrow route (every layer on [N,4] slots, gadapt_block_forward_narrow) runs on this graph at this hidden size - the graphs whose
// forward is the wide kernel, which reproduces the dense flow's arithmetic on channels 0..3 bit for bit
int gadapt_narrow_takes_c(const gadapt_graph* g, int c) { return (c == 64 && g && wide_takes(g)) ? 1 : 0; }

// Narrow route (gadapt_block_forward_narrow): compact [N,4] input, compact [N,4] output in x_top4, hidden 64 on a graph the wide forward
// takes (gadapt_narrow_takes_c).  wide::fwd_narrow_kernel reproduces wide::fwd_kernel<true, ...> on channels 0..3 bit for bit, with the
// same kmax (the longest in-row of the geometry the wide launch would pick).  gadapt_debug_set_narrow_forward(0) keeps the wide kernel.
int gadapt_launch_fwd_narrow_c(int c, const gadapt_graph* g, const LayerFwd& f, hipStream_t st) {
    if (c != 64 || !g || !f.x_top4 || !gadapt_narrow_takes_c(g, c)) return fail(GADAPT_E_BADARG, "narrow forward: hidden 64, head rows, a graph the wide forward takes");
    const int n_steps = (g->n_nodes + wide::NRW_NT - 1) / wide::NRW_NT;
    const int grid = n_steps < GADAPT_LOSS_PARTIALS_MAX / 4 ? n_steps : GADAPT_LOSS_PARTIALS_MAX / 4;   // one loss partial per wave
    wide::FwdArgs p = wide_fwd_args(g, f, n_steps);
    p.x_out = nullptr;
    if (const FwdExtra* ex = f.extra) {
        if (ex->cw && !gadapt_forward_computes_coeffs_c(g, c)) return fail(GADAPT_E_BADARG, "narrow forward: the coefficients are given on this graph (gadapt_forward_computes_coeffs)");
        put_extra(p, *ex, true, ex->cw != nullptr, ex->loss.target != nullptr, 4 * grid);
    }
    if (p.cw && grid < GADAPT_NARROW_COEFF_WGS) return fail(GADAPT_E_BADARG, "narrow forward: in-kernel coefficients need 64 workgroups (one row of A each)");
    ProfScope prof(0, st, 6);                                   // compact input, head-only output (the variant of the wide launch it replaces)
    const bool fld = p.fs.x_comp != nullptr, head = p.loss.target != nullptr;
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(grid), dim3(wide::NRW_NT), 0, st, p); };
    if (head) { if (fld) go(wide::fwd_narrow_kernel<true, true>); else go(wide::fwd_narrow_kernel<true, false>); }
    else { if (fld) go(wide::fwd_narrow_kernel<false, true>); else go(wide::fwd_narrow_kernel<false, false>); }
    return check_launch("wide::fwd_narrow_kernel");
}

// The same for n_layers <= 4 consecutive layers in one launch (wide::fwd_narrow_block_kernel): one 512-thread workgroup per 512-node
// tile, halo from gadapt_narrow_block_halo_host (32 or 64; the caller has it from the graph's registration).  first.x_in: the group's [N,4]
// input slot; the rows of layer k go to first.x_top4 + k * slot_stride, those of the last layer to x_last where given (head rows); lp and
// alpha_out (nullable) are the first layer's, the next layers' follow at + 2 and + alpha_stride.  extra: layer-0 fields / coefficients
// (a group that starts the block), loss (a group that ends it) and, with the loss, extra->top: the top layer's backward target pass in the
// same launch (the TOP instantiations; profiled as this forward launch only).  Everything is checked before the launch.
// gadapt_narrow_kmax_c: the longest in-row the narrow launches walk on this graph.
int gadapt_narrow_kmax_c(const gadapt_graph* g) { return wide_fwd_args(g, LayerFwd{}, 0).kmax; }
int gadapt_narrow_block_tiles_ok_c(const gadapt_graph* g) {
    const int64_t tiles = ((int64_t)g->n_nodes + GADAPT_NARROW_TILE - 1) / GADAPT_NARROW_TILE;
    return tiles >= 1 && tiles * (wide::NRB_NT / 64) <= GADAPT_LOSS_PARTIALS_MAX;      // one loss partial per wave
}
int gadapt_launch_fwd_narrow_block_c(int c, const gadapt_graph* g, const LayerFwd& first, int halo, int n_layers, int64_t slot_stride,
                                     int64_t alpha_stride, float* x_last, hipStream_t st) {
    float* const x_out0 = first.x_top4;
    if (c != 64 || !g || !gadapt_narrow_takes_c(g, c) || (halo != 32 && halo != 64) || n_layers < 1 || n_layers > GADAPT_NARROW_BLOCK_LAYERS ||
        !first.x_in || !first.lp || (!x_out0 && !(x_last && n_layers == 1)) || slot_stride < 4 * (int64_t)g->n_nodes ||
        (first.alpha_out && alpha_stride < g->n_edges))
        return fail(GADAPT_E_BADARG, "narrow block forward: hidden 64, halo 32 or 64, 1..4 layers, output slots, a graph the wide forward takes");
    if (!gadapt_narrow_block_tiles_ok_c(g))
        return fail(GADAPT_E_BADARG, "narrow block forward: more loss partials than GADAPT_LOSS_PARTIALS_MAX (8 per 512-node tile)");
    const int grid = (g->n_nodes + GADAPT_NARROW_TILE - 1) / GADAPT_NARROW_TILE;
    wide::BlockArgs q{};
    q.f = wide_fwd_args(g, first, grid);
    q.f.x_out = nullptr; q.f.residual_only = 0;
    q.K = n_layers; q.halo = halo; q.slot_stride = slot_stride; q.alpha_stride = alpha_stride; q.x_last = x_last;
    wide::FwdArgs& p = q.f;
    if (const FwdExtra* ex = first.extra) {
        if (ex->cw) {
            if (!gadapt_forward_computes_coeffs_c(g, c)) return fail(GADAPT_E_BADARG, "narrow block forward: the coefficients are given on this graph (gadapt_forward_computes_coeffs)");
            if (!ex->a_out || !ex->p0_out) return fail(GADAPT_E_BADARG, "narrow block forward: in-kernel coefficients without their destination");
        }
        if (ex->loss.target && (!x_last || !ex->loss.seed || !ex->loss.partials))
            return fail(GADAPT_E_BADARG, "narrow block forward: a loss needs the head rows, the seed and the partials");
        put_extra(p, *ex, true, ex->cw != nullptr, ex->loss.target != nullptr, (wide::NRB_NT / 64) * grid);
    }
    if (!p.cw && (!first.a || !first.p0)) return fail(GADAPT_E_BADARG, "narrow block forward: no coefficients");
    if (p.cw && grid < GADAPT_NARROW_COEFF_WGS) return fail(GADAPT_E_BADARG, "narrow block forward: in-kernel coefficients need 64 workgroups (one row of A each)");
    // the top layer's backward target pass in this launch (the C-ABI unit's plan decides): one node per lane of the slab grid
    const NarrowTop* top = first.extra ? first.extra->top : nullptr;
    if (top) {
        if (!p.loss.target || !top->dxd || !top->edge_out || !top->slab || !g->tpos_s || g->n_edges <= 0 || p.kmax > GADAPT_NARROW_ROW_MAX ||
            top->slab_rows != gadapt_slab_rows_c(g->n_nodes, c) || !gadapt_narrow_row_is_one_range(g->n_nodes, top->slab_rows))
            return fail(GADAPT_E_BADARG, "narrow block forward (top target pass): a loss, dxd / edge / slab buffers, edges, in-rows of at most 8, one node per lane of the slab grid");
        q.tpos = g->tpos_s; q.edge_out = reinterpret_cast<float2*>(top->edge_out); q.dxd = top->dxd; q.slab = top->slab;
        q.slab_rows = top->slab_rows; q.n_edges = g->n_edges;
    }
    ProfScope prof(0, st, 6 | 32);                              // compact input, head-only output, bit 5: several layers in the launch
    const bool fld = p.fs.x_comp != nullptr, head = p.loss.target != nullptr;
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(grid), dim3(wide::NRB_NT), 0, st, q); };
    if (top) { if (fld) go(wide::fwd_narrow_block_kernel<true, true, true>); else go(wide::fwd_narrow_block_kernel<true, false, true>); }
    else if (head) { if (fld) go(wide::fwd_narrow_block_kernel<true, true>); else go(wide::fwd_narrow_block_kernel<true, false>); }
    else { if (fld) go(wide::fwd_narrow_block_kernel<false, true>); else go(wide::fwd_narrow_block_kernel<false, false>); }
    return check_launch("wide::fwd_narrow_block_kernel");
}

template <int C> static int launch_fwd(const gadapt_graph* g, const LayerFwd& f, hipStream_t st) {
    using K = Cfg<C>;
    if (f.x_cols != 0 && f.x_cols != 4) return fail(GADAPT_E_BADARG, "compact layer input: 4 columns");
    if constexpr (C == 64) {
        if (wide_takes(g)) return launch_wide_fwd(g, f, st);
    }
    FwdArgs p{f.x_in, f.x_out, f.a, f.p0, f.lp, g->rowptr_t, g->col_t, meta_for<K::TM>(g->meta_t), f.alpha_out, g->n_nodes,
              (g->n_nodes + K::TM - 1) / K::TM, f.residual_only, g->n_edges, nullptr, f.x_top4};
#ifdef GADAPT_STAMPS
    p.stamps = g_stamp_buf;
#endif
    const dim3 grid(grid_for(p.n_tiles, resident_blocks<C>(GADAPT_FWD_MAX_BLOCKS)));
    if (f.extra) put_extra(p, *f.extra, f.x_cols != 0, false, !f.x_out && f.x_top4 && f.extra->loss.target, (int)grid.x * K::NW);
    ProfScope prof(0, st, (f.x_cols ? 2 : 0) | (f.x_out ? 0 : 4));
    constexpr int lds = K::lds_bytes(0, K::RING + 1);
    auto go = [&](auto kern) { allow_lds(kern, lds); hipLaunchKernelGGL(kern, grid, dim3(K::NT), lds, st, p); };
    if (f.x_cols) go(grand_fwd_kernel<C, true>); else go(grand_fwd_kernel<C>);
    return check_launch("grand_fwd_kernel");
}

int gadapt_launch_fwd_c(int c, const gadapt_graph* g, const LayerFwd& f, hipStream_t st) { GADAPT_DISPATCH_C(c, launch_fwd<CC>(g, f, st)); }

template <int C> static int occupancy_fwd() {
    int n = -1;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, grand_fwd_kernel<C>, Cfg<C>::NT, Cfg<C>::lds_bytes(0, Cfg<C>::RING + 1));
    return n;
}
int gadapt_occupancy_fwd_c(int c) { GADAPT_DISPATCH_C(c, occupancy_fwd<CC>()); }
