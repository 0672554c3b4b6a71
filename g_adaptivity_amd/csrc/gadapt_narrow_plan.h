// gadapt_narrow_plan.h - the launch sequence of one step of the narrow route (hidden 64, every layer on [N,4] rows), decided in one
// place: what is known about the step (gadapt_narrow_facts), the launch-sequence switches (gadapt_narrow_switches), and ONE pure
// function of the two, gadapt_narrow_plan_of.  The C-ABI unit gathers the facts once per entry-point call and walks the plan
// (gadapt_kernels.hip: block_forward, block_forward_loss, block_backward_narrow); the host copy (gadapt_narrow_step_plan_host,
// csr_build.cpp) is what the CPU tests call.  Plain host code: no HIP header.  The contract it restates is include/gadapt_hip.h.
//
// A plan is walked by index - gadapt_narrow_fwd_launch(plan, i), i < n_fwd, and gadapt_narrow_bwd_launch(plan, i), i < n_bwd - so the
// number of layers has no cap of its own.  A launch record names buffers, not addresses: layer slots come from the entry point's
// Block, work buffers from gadapt_narrow_layout_of.
#ifndef GADAPT_NARROW_PLAN_H
#define GADAPT_NARROW_PLAN_H

#include <stdint.h>
#include "gadapt_block_plan.h"

#define GADAPT_NARROW_ROW_MAX 8         /* in- and out-rows the one-node-per-lane kernels take from registers (GADAPT_MAXD) */
#define GADAPT_NARROW_COEFF_WGS 64      /* workgroups the in-kernel coefficients need: one row of A each */

// ---- what is known about a step when an entry point is called
struct gadapt_narrow_facts {
    int64_t n_nodes, n_edges;
    int c, n_layers;
    int takes;                          // the route runs on this graph at this hidden size (gadapt_narrow_route)
    int halo_t, halo_s;                 // registered halo of the target-ordered / source-ordered CSR (0: none)
    int kmax;                           // the longest in-row the narrow forward walks
    int slab_rows;                      // gadapt_backward_slab_rows
    int tiles_ok;                       // the 512-node tiles keep the loss partials within their maximum
    int ell_t, ell_s, tpos_s, rowptr_s, col_s;   // which tables the graph has
    int shared;                         // one shared conv (a_stride = p0_stride = 0), else one per layer
    int packed;                         // packed slab rows, else full rows
    int target;                         // a loss target is given
    int buffers;                        // the forward call was given the backward's dxd, edge and slab buffers
    int coeffs;                         // the in-kernel coefficients were asked for (param given)
    int top_done;                       // backward: the forward call already ran the top layer's target pass
    int may_block;                      // backward: the entry point may run block groups (it reports *block_ran)
};
#define GADAPT_NARROW_FACTS 22          /* members of gadapt_narrow_facts (gadapt_narrow_step_plan_host takes them as int64 words) */
// ---- the launch-sequence switches (gadapt_debug_set_narrow_forward / _backward_fused / _top_in_forward / _backward_block)
struct gadapt_narrow_switches { int fwd, bwd_fused, top_fwd, bwd_block; };

// ---- predicates with more than one user
// a slab row is the sum over ONE 256-node range: every lane of a 256-thread target-pass workgroup has at most one node
static inline int gadapt_narrow_row_is_one_range(int64_t n_nodes, int slab_rows) { return slab_rows > 0 && n_nodes <= 256 * (int64_t)slab_rows; }
// of the caller's dxd_ws (N c floats) the route uses [0, 4N): a second edge buffer (2E floats) fits behind that ...
static inline int gadapt_narrow_edge2_fits(int64_t n_nodes, int64_t n_edges, int c) { return 2 * n_edges <= (int64_t)(c - 4) * n_nodes; }
// ... and a second dxd [N,4] behind the second edge buffer
static inline int gadapt_narrow_dxd2_fits(int64_t n_nodes, int64_t n_edges, int c) { return 2 * n_edges <= (int64_t)(c - 8) * n_nodes; }

// ---- work buffers: float offsets of the members of each buffer pair.  g[k]: in g_ws (2 N c floats), 4N floats each; dxd[k]: in dxd_ws
// (N c floats), 4N each; edge[0]: in edge_ws (2E floats), edge[1]: in dxd_ws, 2E each.  edge[1] lies inside dxd_ws where
// gadapt_narrow_edge2_fits, dxd[1] where gadapt_narrow_dxd2_fits; a plan names a member only where it fits.
struct gadapt_narrow_layout { int64_t g[2], dxd[2], edge[2]; };
static inline struct gadapt_narrow_layout gadapt_narrow_layout_of(int64_t n_nodes, int64_t n_edges, int c) {
    struct gadapt_narrow_layout y;
    y.g[0] = 0; y.g[1] = n_nodes * c;
    y.dxd[0] = 0; y.dxd[1] = 4 * n_nodes + 2 * n_edges;
    y.edge[0] = 0; y.edge[1] = 4 * n_nodes;
    return y;
}

// sizes whose offsets fit 32 bits: row offsets in bytes as the kernels take them (n_nodes * c * 4 < 4 GiB), and the end of the second dxd
static inline int gadapt_narrow_sizes_ok(int64_t n_nodes, int64_t n_edges, int c) {
    return n_nodes > 0 && n_edges >= 0 && c > 0 && n_nodes * c * 4 < ((int64_t)1 << 32) && 8 * n_nodes + 2 * n_edges < ((int64_t)1 << 31);
}

// ---- the plan
enum { GADAPT_NARROW_FWD_WIDE = 0, GADAPT_NARROW_FWD_NODE = 1, GADAPT_NARROW_FWD_GROUPS = 2 };     // forward: per layer (two kernels), groups
enum { GADAPT_NARROW_BWD_PAIRS = 0, GADAPT_NARROW_BWD_FUSED = 1, GADAPT_NARROW_BWD_GROUPS = 2 };   // backward
struct gadapt_narrow_plan {
    int route;                          // 0: the route does not take the step - no launches
    int n_layers, shared;
    int fwd_kind, fwd_halo, n_fwd;      // forward launches (the coefficient launch not counted)
    int coeffs_first;                   // gadapt_coeffs_forward comes first and the layers take the coefficients as given
    int top_in_fwd;                     // the last forward launch also runs the top layer's target pass (*top_ran)
    int bwd_kind, bwd_halo, n_bwd;
    int top_done;                       // the backward starts below the top layer's target pass
    int block_ran;                      // *block_ran of gadapt_block_backward_narrow_packed_block
    struct gadapt_narrow_layout at;     // where the launches' work buffers lie
};
// One launch.  kind: which launcher; layer: forward - the first layer of the launch, backward - the layer whose target pass (TARGET,
// TARGET0) or source pass (SOURCE, FUSED, GROUP: the first stage's) it runs; count: layers or fused stages in it.  Buffers by pair
// member (gadapt_narrow_layout), -1: none; g_in = -1 with first = 1: the top gradient.  first: forward - starts at layer 0 (node fields,
// in-kernel coefficients), backward - reads the top gradient.  last: forward - ends the block (head rows, loss), backward - its target
// half is layer 0 (slab partials only).  top: forward - the top layer's target pass rides in it (edge_out, dxd_out, slab).
// accumulate: onto the slab rows (0: the launch writes them).
enum { GADAPT_NARROW_L_FWD_WIDE = 0, GADAPT_NARROW_L_FWD_NODE, GADAPT_NARROW_L_FWD_GROUP, GADAPT_NARROW_L_TARGET, GADAPT_NARROW_L_SOURCE,
       GADAPT_NARROW_L_TARGET0, GADAPT_NARROW_L_FUSED, GADAPT_NARROW_L_GROUP };
struct gadapt_narrow_launch { int kind, layer, count, g_in, g_out, edge_in, edge_out, dxd_in, dxd_out, accumulate, first, last, top; };
#define GADAPT_NARROW_PLAN_HEAD 18      /* int32 words of a serialised plan before its records */
#define GADAPT_NARROW_LAUNCH_WORDS 13   /* ... and of one record */

// launches of the fused stages below the top as block groups (gadapt_bwd_block_groups)
static inline int gadapt_narrow_bwd_group_count(int n_layers) {
    int n = 0;
    for (int done = 0, k; (k = gadapt_bwd_block_groups(n_layers - 1, done)) > 0; done += k) ++n;
    return n;
}

static inline struct gadapt_narrow_plan gadapt_narrow_plan_of(const struct gadapt_narrow_facts* f, const struct gadapt_narrow_switches* s) {
    struct gadapt_narrow_plan p = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, gadapt_narrow_layout_of(f->n_nodes, f->n_edges, f->c)};
    if (!f->takes || f->c != 64 || f->n_layers < 1 || f->n_nodes < 1) return p;
    p.route = 1; p.n_layers = f->n_layers; p.shared = f->shared ? 1 : 0;
    const int L = f->n_layers;
    const int one_range = gadapt_narrow_row_is_one_range(f->n_nodes, f->slab_rows);
    // forward: groups of up to GADAPT_NARROW_BLOCK_LAYERS layers where the target side has a registered halo and the conv is shared
    // (default choice only), else one launch per layer
    p.fwd_halo = (s->fwd == 1 && f->shared && f->tiles_ok) ? f->halo_t : 0;
    p.fwd_kind = p.fwd_halo ? GADAPT_NARROW_FWD_GROUPS : (s->fwd != 0 ? GADAPT_NARROW_FWD_NODE : GADAPT_NARROW_FWD_WIDE);
    p.n_fwd = p.fwd_halo ? (L + GADAPT_NARROW_BLOCK_LAYERS - 1) / GADAPT_NARROW_BLOCK_LAYERS : L;
    // the layer-0 launch has one workgroup per 512-node tile (groups) or per 256-node step, and leaves one row of A per workgroup
    const int64_t wgs = p.fwd_halo ? (f->n_nodes + GADAPT_NARROW_TILE - 1) / GADAPT_NARROW_TILE : (f->n_nodes + 255) / 256;
    p.coeffs_first = (f->coeffs && wgs < GADAPT_NARROW_COEFF_WGS) ? 1 : 0;
    p.top_in_fwd = (s->top_fwd && p.fwd_halo && f->target && f->buffers && L >= 2 && f->ell_t && f->tpos_s && f->n_edges > 0 &&
                    f->kmax <= GADAPT_NARROW_ROW_MAX && one_range) ? 1 : 0;
    // backward
    p.top_done = f->top_done ? 1 : 0;
    if (L < 2) return p;
    const int tops = p.top_done ? 0 : 1;                        // T_{L-1} is part of the sequence
    const int groups = f->may_block && s->bwd_block && s->bwd_fused && f->packed && f->shared && L >= 3 && f->n_edges > 0 && f->ell_t &&
                       f->ell_s && f->tpos_s && f->rowptr_s && f->kmax <= GADAPT_NARROW_ROW_MAX && one_range &&
                       (L > GADAPT_NARROW_BWD_BLOCK_STAGES + 1 ? gadapt_narrow_dxd2_fits(f->n_nodes, f->n_edges, f->c)
                                                               : gadapt_narrow_edge2_fits(f->n_nodes, f->n_edges, f->c));
    if (groups && f->halo_s) {
        p.bwd_kind = GADAPT_NARROW_BWD_GROUPS; p.bwd_halo = f->halo_s; p.block_ran = 1;
        p.n_bwd = tops + gadapt_narrow_bwd_group_count(L);
    } else if (s->bwd_fused && f->ell_s && f->rowptr_s && f->col_s && gadapt_narrow_edge2_fits(f->n_nodes, f->n_edges, f->c)) {
        p.bwd_kind = GADAPT_NARROW_BWD_FUSED;
        p.n_bwd = tops + L - 1;
    } else {
        p.bwd_kind = GADAPT_NARROW_BWD_PAIRS;
        p.n_bwd = tops + 2 * (L - 1);
    }
    return p;
}

static inline struct gadapt_narrow_launch gadapt_narrow_no_launch(int kind, int layer) {
    struct gadapt_narrow_launch r = {kind, layer, 1, -1, -1, -1, -1, -1, -1, 0, 0, 0, 0};
    return r;
}
static inline struct gadapt_narrow_launch gadapt_narrow_fwd_launch(const struct gadapt_narrow_plan* p, int i) {
    const int per = p->fwd_kind == GADAPT_NARROW_FWD_GROUPS ? GADAPT_NARROW_BLOCK_LAYERS : 1, l = i * per;
    struct gadapt_narrow_launch r = gadapt_narrow_no_launch(p->fwd_kind == GADAPT_NARROW_FWD_GROUPS ? GADAPT_NARROW_L_FWD_GROUP :
                                                            (p->fwd_kind == GADAPT_NARROW_FWD_NODE ? GADAPT_NARROW_L_FWD_NODE : GADAPT_NARROW_L_FWD_WIDE), l);
    r.count = p->n_layers - l < per ? p->n_layers - l : per;
    r.first = l == 0; r.last = l + r.count == p->n_layers;
    if (r.last && p->top_in_fwd) { r.top = 1; r.edge_out = 0; r.dxd_out = 0; }      // T_{L-1} with accumulate = 0, as the backward's
    return r;
}
// T_{L-1}: reads the top gradient, leaves dxd and the pairs in the first member of each pair and writes every slab row
static inline struct gadapt_narrow_launch gadapt_narrow_top_target(int L) {
    struct gadapt_narrow_launch r = gadapt_narrow_no_launch(GADAPT_NARROW_L_TARGET, L - 1);
    r.edge_out = 0; r.dxd_out = 0; r.first = 1;
    return r;
}
static inline struct gadapt_narrow_launch gadapt_narrow_bwd_launch(const struct gadapt_narrow_plan* p, int i) {
    const int L = p->n_layers;
    if (p->bwd_kind == GADAPT_NARROW_BWD_PAIRS) {
        // T_{L-1}, S_{L-1}, T_{L-2}, S_{L-2}, .., S_1, T_0: one edge buffer, one dxd, the halves of g_ws in turn
        const int at = i + p->top_done, l = L - 1 - at / 2;
        if (at == 0) return gadapt_narrow_top_target(L);
        struct gadapt_narrow_launch r = gadapt_narrow_no_launch(l == 0 ? GADAPT_NARROW_L_TARGET0 : ((at & 1) ? GADAPT_NARROW_L_SOURCE : GADAPT_NARROW_L_TARGET), l);
        r.first = l == L - 1; r.g_in = r.first ? -1 : ((L - 2 - l) & 1);
        if (r.kind == GADAPT_NARROW_L_SOURCE) { r.edge_in = 0; r.dxd_in = 0; r.g_out = (L - 1 - l) & 1; return r; }
        r.accumulate = p->shared;                                // (below the top: the top layer's launch wrote the rows)
        if (l == 0) r.last = 1; else { r.edge_out = 0; r.dxd_out = 0; }
        return r;
    }
    if (!p->top_done && i == 0) return gadapt_narrow_top_target(L);
    const int m = i - (p->top_done ? 0 : 1);                     // launch number below T_{L-1}
    int done = m, count = 1;                                    // fused stages above this launch, and in it
    if (p->bwd_kind == GADAPT_NARROW_BWD_GROUPS) {
        done = 0; count = gadapt_bwd_block_groups(L - 1, 0);
        for (int k = 0; k < m; ++k) { done += count; count = gadapt_bwd_block_groups(L - 1, done); }
    }
    // [S_l + T_{l-1}] (count of them): reads what the launch above left in member m & 1 of the edge pair and writes the other; g rows go
    // to the halves of g_ws in turn.  dxd: a FUSED launch reads and writes row j of ONE buffer in the lane that owns node j; a GROUP
    // reads halo rows other workgroups own, so its last stage stores to the other member.
    struct gadapt_narrow_launch r = gadapt_narrow_no_launch(p->bwd_kind == GADAPT_NARROW_BWD_GROUPS ? GADAPT_NARROW_L_GROUP : GADAPT_NARROW_L_FUSED, L - 1 - done);
    const int both = p->bwd_kind == GADAPT_NARROW_BWD_GROUPS;
    r.count = count; r.first = m == 0; r.last = done + count == L - 1;
    r.g_in = m == 0 ? -1 : ((m - 1) & 1); r.edge_in = m & 1; r.dxd_in = both ? (m & 1) : 0;
    r.accumulate = both ? 1 : p->shared;
    if (!r.last) { r.g_out = m & 1; r.edge_out = (m + 1) & 1; r.dxd_out = both ? ((m + 1) & 1) : 0; }
    return r;
}

// ---- a plan as int32 words (gadapt_narrow_step_plan, gadapt_narrow_step_plan_host; layout: include/gadapt_hip.h).  Returns the words
// written, or -1 when cap is too small.  (The offsets fit a word: the callers refuse sizes beyond gadapt_narrow_sizes_ok.)
static inline int gadapt_narrow_plan_words(const struct gadapt_narrow_plan* p) {
    return GADAPT_NARROW_PLAN_HEAD + GADAPT_NARROW_LAUNCH_WORDS * (p->n_fwd + p->n_bwd);
}
static inline int gadapt_narrow_plan_write(const struct gadapt_narrow_plan* p, int32_t* out, int cap) {
    if (cap < gadapt_narrow_plan_words(p)) return -1;
    const int head[GADAPT_NARROW_PLAN_HEAD] = {p->route, p->n_fwd, p->n_bwd, p->fwd_kind, p->fwd_halo, p->coeffs_first, p->top_in_fwd, p->bwd_kind,
                                               p->bwd_halo, p->top_done, p->block_ran, GADAPT_NARROW_LAUNCH_WORDS,
                                               (int)p->at.g[0], (int)p->at.g[1], (int)p->at.dxd[0], (int)p->at.dxd[1], (int)p->at.edge[0], (int)p->at.edge[1]};
    for (int k = 0; k < GADAPT_NARROW_PLAN_HEAD; ++k) out[k] = head[k];
    int32_t* o = out + GADAPT_NARROW_PLAN_HEAD;
    for (int i = 0; i < p->n_fwd + p->n_bwd; ++i, o += GADAPT_NARROW_LAUNCH_WORDS) {
        const struct gadapt_narrow_launch r = i < p->n_fwd ? gadapt_narrow_fwd_launch(p, i) : gadapt_narrow_bwd_launch(p, i - p->n_fwd);
        const int w[GADAPT_NARROW_LAUNCH_WORDS] = {r.kind, r.layer, r.count, r.g_in, r.g_out, r.edge_in, r.edge_out, r.dxd_in, r.dxd_out,
                                                   r.accumulate, r.first, r.last, r.top};
        for (int k = 0; k < GADAPT_NARROW_LAUNCH_WORDS; ++k) o[k] = w[k];
    }
    return gadapt_narrow_plan_words(p);
}

#endif  // GADAPT_NARROW_PLAN_H
