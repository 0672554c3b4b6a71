/*
 * gadapt_hip.h - C-ABI of the MI355X-native g-adaptivity message-passing path.
 *
 * Plain pointers and sizes only: no torch types cross this boundary.  Every device
 * pointer is fp32 / int32 HBM memory owned by the caller; `stream` is a hipStream_t
 * passed as void*.  All entry points return 0 on success or a negative GADAPT_E_*
 * code and never abort; `gadapt_last_error()` gives the message.  Nothing here
 * allocates, frees or synchronises (graph-capture safe) except the *_host helpers.
 *
 * The reference (/root/reference, 100 % Python) has no FFI; each entry point cites
 * the reference code whose arithmetic it replaces.  INTEGRATION.md shows the
 * ctypes binding a maintainer adds on the reference side.
 *
 * Formulation.  One GRAND layer of the reference is
 *     Q = x Wq^T + bq,  K = x Wk^T + bk,  s_ij = <Q_i,K_j>/sqrt(C)   (GRAND_plus.py:225-226,279)
 *     alpha_ij = softmax_j(s_ij / T)  over edges j->i                 (GRAND_plus.py:326-333)
 *     x'_i = x_i + dt * (sum_j alpha_ij x_j - x_i)                    (GRAND_plus.py:338-343,267; GNN.py:288-291)
 * <Q_i,K_j> = P_i . x_j + <Q_i,bk>  with  P_i = A x_i + p0,  A = Wk^T Wq,  p0 = Wk^T bq;
 * the second term does not depend on j and cancels in the softmax, so the kernels
 * work from (A, p0): one [C,C] projection per node instead of two, and the edge walk
 * gathers x_j only.
 *
 * Arithmetic.  Everything is fp32 in and out.  At hidden sizes >= 32 the [nodes,C] x [C,C] products (P = x A^T, dP A, A y and
 * the dA partial) run on the 16-bit matrix cores from operands split into pieces that restore fp32 accuracy: three bf16
 * pieces (x = h + m + l exactly, six piece products, the dropped ones below 2^-23 |x y|) or, where the operand tile is prepared
 * once per tile, two f16 pieces after an exact power-of-two scaling per row / column group (hh + hl + lh, dropped term below
 * 2^-22 |x y|); piece products are exact in the fp32 accumulators.  The softmax uses expf and a true
 * division.  Measured against an fp64 evaluation: coordinates 1e-7 relative, parameter gradients at the fp32 reference
 * path's own rounding level (tests/test_gpu_parity.py, full BASELINE sizes included).
 */
#ifndef GADAPT_HIP_H
#define GADAPT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GADAPT_OK            0
#define GADAPT_E_BADARG     -1   /* null pointer, negative size, unsupported hidden_dim ... */
#define GADAPT_E_LAUNCH     -2   /* hipGetLastError() after a launch */
#define GADAPT_E_RANGE      -3   /* edge endpoint outside [0, n_nodes) */
#define GADAPT_E_RUNTIME    -4   /* a run-time dependency is missing or failed (gadapt_allreduce_flat: RCCL) */

/* Hidden sizes the fused kernels are built for; others -> GADAPT_E_BADARG. */
int  gadapt_supported_hidden_dim(int c);
const char* gadapt_last_error(void);
int  gadapt_abi_version(void);
/* Forget a pending error of the calling thread: the message of gadapt_last_error() and HIP's own sticky per-thread last error
 * (hipGetLastError).  For callers that recover from a failure that did not come through this library - e.g. a hipGraph capture
 * that was invalidated: every later launch check would otherwise report that stale error once.  Returns the HIP error code that
 * was pending (0: none). */
int  gadapt_clear_error(void);

/* ------------------------------------------------------------------ graph
 * Replaces the per-forward edge bookkeeping of PyG's MessagePassing.propagate
 * (called at GRAND_plus.py:233-234) with a one-time CSR build.  Input is the
 * edge list AFTER GNN.py:206-223 surgery, host memory, int64 as PyG holds it:
 * src[e] -> dst[e].  Outputs (host, int32, caller-allocated):
 *   rowptr_t[N+1], col_t[E] : in-edges grouped by target, col_t = source;
 *   eid_t[E]                : original edge id of each target-ordered slot
 *                             (alpha_out[slot] belongs to edge eid_t[slot]);
 *   rowptr_s[N+1], col_s[E] : out-edges grouped by source, col_s = target;
 *   perm_s[E]               : target-ordered slot of each source-ordered slot;
 *   tpos_s[E]               : its inverse - source-ordered slot of each target-ordered slot.
 * Order inside a row is the input order (stable), so results are reproducible. */
int gadapt_csr_build_host(const int64_t* src, const int64_t* dst, int64_t n_edges, int64_t n_nodes,
                          int32_t* rowptr_t, int32_t* col_t, int32_t* eid_t,
                          int32_t* rowptr_s, int32_t* col_s, int32_t* perm_s, int32_t* tpos_s);

/* Per-tile staging metadata for the kernels: for tiles of `tile_rows` consecutive rows of one CSR orientation,
 * meta[4t+0] = first entry of the tile's slice, [4t+1] = its length, [4t+2] = the longest row,
 * [4t+3] = 1 if every neighbour of the tile's rows lies in tiles t-1..t+1 (the kernels then gather from an LDS
 * window instead of L2), else 0.  The kernels use tile heights 64, 128 and 256 (by hidden size): build all three
 * for both orientations (host pointers). */
int gadapt_tile_meta_host(const int32_t* rowptr, const int32_t* col, int64_t n_nodes, int tile_rows, int32_t* meta_out);

typedef struct gadapt_graph {
    int32_t n_nodes;
    int32_t n_edges;
    const int32_t* rowptr_t;  /* device */
    const int32_t* col_t;
    const int32_t* rowptr_s;
    const int32_t* col_s;
    const int32_t* perm_s;
    const int32_t* tpos_s;
    const int32_t* meta_t[3];  /* device: tile metadata of the target CSR for tile heights 64, 128, 256 */
    const int32_t* meta_s[3];  /* device: same for the source CSR */
    /* optional (NULL / 0 = absent): ELL-8 copies for the wide kernels (gadapt_ell_build_host) */
    const int32_t* ell_t;      /* device [round_up(N,256)][8]: in-neighbours of node i, -1 = unused */
    const int32_t* ell_s;      /* device: out-neighbours (targets), same layout */
    int32_t wide_deg_t;        /* longest in-row if the target orientation qualifies for the wide kernels, else 0 */
    int32_t wide_deg_s;        /* same for the source orientation */
    int32_t wide_big_deg_t;    /* longest in-row if the target orientation qualifies for the 512-row window of the wide forward
                                  (gadapt_wide_window_host(step 256, halo 128, rows <= 7): meshes with up to 128 nodes per row), else 0 */
    int32_t wide_half_deg_t;   /* ABI 9: longest in-row if the target orientation also qualifies for steps of 128 nodes with a 64-row halo
                                  (gadapt_wide_window_host(step 128, halo 64, rows <= 8)), else 0: batches of at most 32 768 nodes then run
                                  the wide forward on four-wave workgroups, twice as many of them */
} gadapt_graph;

/* ELL-8 copy of one CSR orientation (host pointers).  The wide kernels (hidden size 64: one wave owns 32 consecutive
 * nodes, two lanes per node, a 256-node workgroup step gathers from a 384-row LDS window) run when every row has at
 * most 8 entries and every neighbour of node i lies in rows [256*(i/256) - 64, 256*(i/256) + 320): row-major mesh
 * batches do; any other graph takes the tiled kernels.  ell_out: round_up(N,256)*8 int32; *max_deg_out = longest
 * row when the orientation qualifies, else 0. */
int gadapt_ell_build_host(const int32_t* rowptr, const int32_t* col, int64_t n_nodes, int32_t* ell_out, int32_t* max_deg_out);
/* The same locality test for steps of `step` nodes, a window of step + 2*halo rows and rows of at most max_row entries: *max_deg_out =
 * longest row when every neighbour of node i lies in rows [step*(i/step) - halo, step*(i/step) + step + halo), else 0.  step 256 / halo
 * 128 / max_row 7 is what the wide forward's 512-row window takes (row-major meshes with up to 128 nodes per mesh row: BASELINE config
 * 5); step 128 / halo 64 / max_row 8 what its four-wave form takes (gadapt_graph::wide_half_deg_t). */
int gadapt_wide_window_host(const int32_t* rowptr, const int32_t* col, int64_t n_nodes, int step, int halo, int max_row, int32_t* max_deg_out);

/* One launch for up to 4 consecutive forward layers of the narrow route (gadapt_block_forward_narrow / _loss_narrow), by halo recompute:
 * a workgroup owns 512 consecutive nodes and computes layer k on them widened by (K - 1 - k) * halo on each side, so no workgroup waits
 * for another.  *halo_out = the smallest h in {32, 64} such that every row of the target-ordered CSR has at most 8 entries and every
 * in-neighbour of node i lies in [32*(i/32) - h, 32*(i/32) + 32 + h) (gadapt_wide_window_host(step 32, h, max_row 8)); 0: neither, the
 * graph keeps one launch per layer.  Row-major meshes up to 32 nodes wide give 32, up to 64 wide 64.  Host pointers. */
int gadapt_narrow_block_halo_host(const int32_t* rowptr, const int32_t* col, int64_t n_nodes, int32_t* halo_out);
/* The plan the kernel follows, for checking it on the host: [*lo_out, *hi_out) = the nodes tile `tile` (512 nodes each) computes at
 * layer `layer` (0 .. n_layers-1) of a group of n_layers <= 4 layers - its owned range widened by (n_layers - 1 - layer) * halo, clamped
 * to [0, round_up(n_nodes, 32)); layer = -1: the range of input rows it loads, one halo wider than layer 0's. */
int gadapt_narrow_block_range_host(int64_t n_nodes, int halo, int n_layers, int64_t tile, int layer, int64_t* lo_out, int64_t* hi_out);
/* ... and the packed slab rows a tile owes when the top layer's backward target pass runs in the launch (see
 * gadapt_block_forward_loss_narrow_top below).  Slab row r sums nodes 256 r .. 256 r + 255 as (b0 + b1) + (b2 + b3) over its 64-node
 * blocks in node order; the eight waves of a tile own its eight blocks in rotated order.  plan_out (12 ints): the two rows 2 tile and
 * 2 tile + 1; the four waves that feed the first row, in summation order, then the four of the second; then zero_first and zero_step:
 * the tile also writes zeros to rows zero_first, zero_first + zero_step, ... below the slab's row count - the rows beyond the last
 * tile's - so that every row is written by exactly one tile.  owned_block_host: the block (0..7, node order within the tile) wave
 * `wave` (0..7) owns, or -1 for a bad argument. */
int gadapt_narrow_block_slab_plan_host(int64_t n_nodes, int halo, int n_layers, int64_t tile, int32_t* plan_out);
int gadapt_narrow_block_owned_block_host(int halo, int n_layers, int wave);
/* gadapt_graph holds device arrays, so the library cannot find the halo itself: the caller tells it once per graph, after filling the
 * structure (halo = gadapt_narrow_block_halo_host's result; 0 = forget the graph - call it before the arrays are freed or reused for
 * another graph).  The entry is keyed by (rowptr_t, ell_t, n_nodes, n_edges).  A graph that was never registered runs one launch per
 * layer; results are bit-identical either way. */
int gadapt_narrow_block_register(const gadapt_graph* g, int halo);
/* The halo the narrow route's forward would run its one-launch groups with on this graph at hidden size c right now (the registered
 * halo, the forward choice of gadapt_debug_set_narrow_forward, at most 512 tiles), or 0: one launch per layer.  Per-layer convs
 * (a_stride != 0) keep one launch per layer as well. */
int gadapt_narrow_block_halo(const gadapt_graph* g, int c);

/* The backward layers below the top in one launch (gadapt_block_backward_narrow_packed_block below): the same tiles, K = 2 or 3 fused
 * stages [S_l + T_{l-1}] per launch, stage s on the owned range widened by (K - 1 - s) * halo, where halo is that of the SOURCE-ordered
 * CSR: gadapt_narrow_block_halo_host(rowptr_s, col_s, ...).  gadapt_narrow_block_register_source tells the library (0 = forget), keyed by
 * (rowptr_s, ell_s, n_nodes, n_edges); gadapt_narrow_block_register and its meaning are unchanged.  The host copies of the plan:
 * range_host = the nodes of stage `stage` (0 .. n_stages-1) of a launch of n_stages stages, and (pair_cap_out, nullable) how many
 * {alpha dt, ds} pairs the LDS buffer holds that the stage before fills for it (0 for stage 0); margin_host = the frame rows in front of
 * the owned range; groups_host = the stages of the launch that starts at fused stage `done` of n_stages = L - 1 (groups of three, a
 * remainder of one avoided: 5 = 3 + 2, 4 = 2 + 2; 0 = none left). */
int gadapt_narrow_block_register_source(const gadapt_graph* g, int halo);
int gadapt_narrow_bwd_block_range_host(int64_t n_nodes, int halo, int n_stages, int64_t tile, int stage, int64_t* lo_out, int64_t* hi_out,
                                       int32_t* pair_cap_out);
int gadapt_narrow_bwd_block_margin_host(int halo, int n_stages);
int gadapt_narrow_bwd_block_groups_host(int n_stages, int done);

/* ------------------------------------------------------------------ weights
 * A[o][c] = sum_r Wk[r][o] Wq[r][c],  p0[o] = sum_r Wk[r][o] bq[r].
 * Wq,Wk are torch Linear weights [out,in] (GRAND_plus.py:146-147). */
int gadapt_coeffs_forward(const float* wq, const float* bq, const float* wk,
                          float* a_out, float* p0_out, int c, void* stream);
/* Chain rule back to the Linear parameters.  dbk is written as exact zeros:
 * d/dbk vanishes because softmax is shift-invariant per target. */
int gadapt_coeffs_backward(const float* wq, const float* bq, const float* wk,
                           const float* d_a, const float* d_p0,
                           float* d_wq, float* d_bq, float* d_wk, float* d_bk, int c, void* stream);

/* ------------------------------------------------------------------ encoder
 * x0 = feats @ W^T (+ b): get_enc (GNN.py:72-98, call :270).  feats [N,F], W [C,F]. */
int gadapt_encode_linear(const float* feats, const float* w, const float* b /*nullable*/,
                         float* x0, int64_t n_nodes, int f, int c, void* stream);
/* Same with the feature assembly of GNN.py:225-239 folded in: the node feature vector is
 * [x_comp[i, 0..dim), f_tensor[i] (if given), uu_tensor[i] (if given)], W [C, dim + extras]. */
int gadapt_encode_features(const float* x_comp, int dim, const float* f_tensor /*nullable*/,
                           const float* uu_tensor /*nullable*/, const float* w, const float* b /*nullable*/,
                           float* x0, int64_t n_nodes, int c, void* stream);

/* gadapt_encode_features and gadapt_coeffs_forward (of ONE conv: the weight-shared layer of GNN.py:131-140) in a single
 * launch: both precede layer 0 and are independent of each other.  c = encoder output width, c_conv = conv width. */
int gadapt_encode_features_coeffs(const float* x_comp, int dim, const float* f_tensor /*nullable*/,
                                  const float* uu_tensor /*nullable*/, const float* w, const float* b /*nullable*/,
                                  float* x0, int64_t n_nodes, int c,
                                  const float* wq, const float* bq, const float* wk, float* a_out, float* p0_out, int c_conv,
                                  void* stream);

/* ------------------------------------------------------------------ one layer
 * layer_params (device, 2 floats): {dt, score_scale} with score_scale = 1/(sqrt(C)*T).
 * alpha_out (nullable) [E] in target order.  x_out must not alias x_in.
 * residual_only = 0: x_out = x + dt*(A(x)x - x)   (conv + Euler update, GNN.py:288-291)
 * residual_only = 1: x_out = A(x)x - x            (what GRAND_plusConv.forward returns,
 *                                                  GRAND_plus.py:267; dt is ignored)   */
int gadapt_layer_forward(const gadapt_graph* g, const float* x_in, float* x_out,
                         const float* a, const float* p0, const float* layer_params,
                         float* alpha_out, int residual_only, int c, void* stream);

/* Workspace sizing for the backward: the target pass leaves one partial-sum row of
 * (C*C + C) floats per workgroup ("slab"); rows depends on the node count only. */
int     gadapt_backward_slab_rows(int64_t n_nodes, int c);
int64_t gadapt_backward_slab_floats(int64_t n_nodes, int c);   /* rows * (C*C + C) */

/* Backward of one layer, split in two launches:
 *   target pass: per in-edge d(score), per node dP, weight-gradient partials, and
 *                dxd = (1-dt) g + A^T dP;
 *   source pass: g_out = dxd + sum over out-edges (alpha dt g_i + dscore A x_i ...) .
 * g_in = dL/dx_out [N,C]; x_in = the layer's input; alpha = forward's alpha_out.
 * edge_ws [E] float2 (filled in source order through tpos_s), dxd_ws [N,C] scratch.  slab accumulates (accumulate!=0) or is
 * overwritten.  sums_out (nullable, 2 floats per call, atomically accumulated):
 * {d dt, d score_scale}.  Pass g_out = NULL to skip the source pass (layer 0 with a
 * frozen encoder: GNN.py:82). */
int gadapt_layer_backward(const gadapt_graph* g, const float* x_in, const float* g_in,
                          const float* alpha, const float* a, const float* p0,
                          const float* layer_params,
                          float* edge_ws, float* dxd_ws, float* slab, int accumulate,
                          float* sums_out, float* g_out, int residual_only, int c, void* stream);

/* slab [n_rows][C*C+C] -> d_a [C*C], d_p0 [C].  scratch: 32*(C*C+C) floats. */
int gadapt_slab_reduce(const float* slab, int n_rows, float* scratch, float* d_a, float* d_p0, int c, void* stream);

/* gadapt_slab_reduce followed by gadapt_coeffs_backward in two launches instead of three: the second-level sums and the
 * chain rule share a kernel (d_a / d_p0 only ever exist in LDS).  Same results bit for bit. */
int gadapt_slab_reduce_coeffs_backward(const float* slab, int n_rows, float* scratch,
                                       const float* wq, const float* bq, const float* wk,
                                       float* d_wq, float* d_bq, float* d_wk, float* d_bk, int c, void* stream,
                                       const float* lp_partials /*nullable*/, int n_layers, int want_d_scale,
                                       float* d_layer_params /*nullable*/);
/* lp_partials (nullable): the [2][L][n_rows] workspace gadapt_block_backward filled - the first launch then also does what
 * gadapt_layer_params_reduce does (a few extra workgroups instead of a launch of its own). */

/* ------------------------------------------------------------------ L-step Euler block
 * The loop of GNN.py:273-291 with weight sharing (GNN.py:131-141): x_all is
 * [(L+1),N,C] with x_all[0] = encoder output on entry; layer l reads x_all[l],
 * writes x_all[l+1].  a/p0/layer_params advance by *_stride floats per layer
 * (0 = shared).  alpha_all (nullable) [L,E].
 * x0_cols = 0: slot 0 holds the dense [N,C] encoder output.  x0_cols = 4: slot 0 holds, at its start, the COMPACT
 * [N,4] output of the identity encoder (zero-pad to C columns, GNN.py:75-82: columns 4.. are zero by construction);
 * layer 0 reads it without the padded matrix ever being written (needs >= 2 layers, hidden >= 8). */
int gadapt_block_forward(const gadapt_graph* g, float* x_all, int x0_cols, int n_layers,
                         const float* a, int64_t a_stride, const float* p0, int64_t p0_stride,
                         const float* layer_params, float* alpha_all, float* x_top4, int c, void* stream);
/* x_top4 (nullable) [N,4]: when given, the last layer writes ONLY columns 0..3 of its output rows, to x_top4, and slot L
 * of x_all is left unwritten: the caller wants x_phys = x[:, :dim] (GNN.py:299) and nothing downstream reads the rest. */

/* Backward of the block.  g_top = dL/dx_all[L] (not modified): [N,C] when g_top_cols = 0, or the compact [N,g_top_cols]
 * (1..4 columns, zero beyond: the backward of x_phys = x[:, :dim], GNN.py:299, without materialising the padded
 * matrix).  x0_cols as in gadapt_block_forward (then d_x0 must be NULL).  g_ws: 2*N*C floats,
 * dxd_ws: N*C, edge_ws: 2*E, slab: n_slots*gadapt_backward_slab_floats(N,c) with
 * n_slots = 1 (shared weights) or L.  d_layer_params (nullable): WORKSPACE of 2 * L * gadapt_backward_slab_rows(N,c) floats -
 * every target-pass workgroup writes its partial of d dt_l (learn_step, GNN.py:179-180,288-289) and, when want_d_scale != 0, of
 * d score_scale_l into its own slot; gadapt_layer_params_reduce then sums them in a fixed order (no float atomics: the step and
 * temperature gradients are bit-reproducible).  want_d_scale = 0: the per-edge log terms of d score_scale are not computed.
 * d_x0 (nullable) [N,C] receives dL/dx_all[0]. */
int gadapt_block_backward(const gadapt_graph* g, const float* x_all, int x0_cols, const float* alpha_all,
                          const float* g_top, int g_top_cols, int n_layers,
                          const float* a, int64_t a_stride, const float* p0, int64_t p0_stride,
                          const float* layer_params,
                          float* g_ws, float* dxd_ws, float* edge_ws, float* slab,
                          float* d_layer_params, int want_d_scale, float* d_x0, int c, void* stream);
/* ------------------------------------------------------------------ fused training step (ABI 8)
 * The reference's iteration - zero_grad, model(data), F.mse_loss / F.l1_loss(out, data.x_phys), backward, Adam step
 * (run_GNN.py:99-131; loss :80-84,106; Adam :88,128-131) - for a weight-shared GRAND / GRAND_plus block behind the identity
 * encoder, as 14 launches instead of 16 (and without the two that cost most: the loss and the encoder): gadapt_block_forward_loss, gadapt_block_backward (g_top = seed, g_top_cols = d),
 * gadapt_step_tail.
 *
 * gadapt_block_forward_loss = gadapt_block_forward(x0_cols = 4, x_top4) with two things folded into its launches:
 *   - layer 0 assembles its compact [N,4] input [x_comp | f | uu | 0] from the caller's node fields (the feature concatenation of
 *     GNN.py:225-239 through the zero-pad encoder GNN.py:75-82; f_tensor / uu_tensor nullable, dim + extras <= 4) and writes it to
 *     the start of x_all's slot 0, where the layer-0 backward reads it: no encoder launch;
 *   - the last layer's head-only launch also writes seed [N,d] = d loss / d x_top4[:, :d] (same arithmetic as gadapt_loss_forward)
 *     and one partial of sum |x_top4[:, :d] - target|^p per wave to loss_partials (gadapt_loss_partials_max() floats): no loss
 *     launch.  Returns the number of partials written (> 0) or a negative error code.  target == NULL (seed, loss_partials unused): no
 *     loss, returns 0 - the evaluation forward on the node fields as one call (the layer-0 launch reads them, x_top4 is the result).
 * (a, p0): the composite coefficients of the shared conv.  param == NULL: INPUTS - from gadapt_coeffs_forward before the first
 * step, from the previous step's gadapt_step_tail afterwards.  param != NULL (only where gadapt_forward_computes_coeffs(g, c) = 1:
 * hidden 64 on a graph the wide forward kernel takes): the flat bucket [Wq | bq | Wk | bk] the step trains - the layer-0 launch
 * computes A = Wk^T Wq, p0 = Wk^T bq itself (gadapt_coeffs_forward's arithmetic; every workgroup for its own operand fragments,
 * while its window of node rows is in flight) and writes them to a / p0 for the launches that follow: OUTPUTS, and no coefficient
 * launch anywhere in the step. */
int gadapt_loss_partials_max(void);
int gadapt_forward_computes_coeffs(const gadapt_graph* g, int c);
int gadapt_block_forward_loss(const gadapt_graph* g, float* x_all, const float* x_comp, int dim, const float* f_tensor /*nullable*/,
                              const float* uu_tensor /*nullable*/, int n_layers, float* a, float* p0, const float* param /*nullable*/,
                              const float* layer_params, float* alpha_all, float* x_top4,
                              const float* target, int d, int l1, float* seed, float* loss_partials, int c, void* stream);
/* ------------------------------------------------------------------ narrow route (ABI 9; resolved by name: a library without them fails to load)
 * GRAND_plus behind the zero-pad identity encoder keeps columns 4.. of every layer's x at exactly zero (lin_value = Identity,
 * root_weight = False: x' = x + dt (sum_j alpha_ij x_j - x) maps zero columns to zero columns), so the whole block can run on the
 * four live columns.  gadapt_narrow_route(g, c) = 1 where it does: hidden 64 on a graph the wide forward kernel takes (its XC
 * instantiation reproduces the dense flow's arithmetic on channels 0..3 bit for bit).  The three calls below have the signatures and
 * buffers of their dense-slot namesakes; what differs:
 *   - every slot of x_all holds [N,4] rows at its start (slot 0 as with x0_cols = 4; layer l < L-1 writes slot l+1, the last layer
 *     x_top4): x0_cols must be 4 and x_top4 given;
 *   - gadapt_block_backward_narrow: g_top compact (1 <= g_top_cols <= 4), d_layer_params and d_x0 NULL (fixed steps and temperature);
 *     layers L-1 .. 1 run the narrow target and source passes on [N,4] rows (dxd_ws, g_ws used at their start), layer 0 the compact
 *     target pass - by default with each source pass inside the next target pass (gadapt_debug_set_narrow_backward_fused), which
 *     uses floats 4N .. 4N + 2E of dxd_ws (N c floats, as for gadapt_block_backward) as a second edge buffer.  Weight gradients land in the 4 x 4 corner of dA and entries 0..3 of dp0 of the slab rows; the rest of each row is
 *     written zero, so the slab reduction and gadapt_step_tail are the dense route's;
 *   - gadapt_block_forward_loss_narrow with param != NULL: the layer-0 launch spreads the rows of A / p0 over its first 64 workgroups
 *     (one per 256-node step, or per 512-node tile of a group launch), so on a graph of fewer than 64 of them the call issues
 *     gadapt_coeffs_forward first and the layers take (a, p0) as given - the same values, one launch more.
 * Which launches a step runs, rule by rule, and where their work buffers lie: gadapt_narrow_step_plan below. */
int gadapt_narrow_route(const gadapt_graph* g, int c);
int gadapt_block_forward_narrow(const gadapt_graph* g, float* x_all, int x0_cols, int n_layers,
                                const float* a, int64_t a_stride, const float* p0, int64_t p0_stride,
                                const float* layer_params, float* alpha_all, float* x_top4, int c, void* stream);
int gadapt_block_forward_loss_narrow(const gadapt_graph* g, float* x_all, const float* x_comp, int dim, const float* f_tensor /*nullable*/,
                                     const float* uu_tensor /*nullable*/, int n_layers, float* a, float* p0, const float* param /*nullable*/,
                                     const float* layer_params, float* alpha_all, float* x_top4,
                                     const float* target, int d, int l1, float* seed, float* loss_partials, int c, void* stream);
int gadapt_block_backward_narrow(const gadapt_graph* g, const float* x_all, int x0_cols, const float* alpha_all,
                                 const float* g_top, int g_top_cols, int n_layers,
                                 const float* a, int64_t a_stride, const float* p0, int64_t p0_stride,
                                 const float* layer_params,
                                 float* g_ws, float* dxd_ws, float* edge_ws, float* slab,
                                 float* d_layer_params, int want_d_scale, float* d_x0, int c, void* stream);
/* Tail of the step.  slab != NULL (one GPU): the first-level slab sums (as gadapt_slab_reduce_coeffs_backward's first launch; one
 * extra workgroup advances the optimizer's device step count and sums the loss partials in a fixed order: loss_out[0] = sum /
 * loss_count); ONE launch that finishes the sums, applies the chain rule to the flat gradient grad = [dWq | dbq | dWk | dbk]
 * (gadapt_slab_reduce_coeffs_backward's arithmetic) and runs Adam on the flat bucket param = [Wq | bq | Wk | bk]
 * (gadapt_adam_step_dev's arithmetic and state; a workgroup owns whole rows r of Wq / Wk with bq[r], bk[r] - the chain rule of those
 * entries reads only entries the same workgroup owns, so the launch needs no exchange between workgroups); and, when a_out / p0_out
 * are given, gadapt_coeffs_forward of the UPDATED weights -> (a_out, p0_out) for the next step (NULL where the next forward computes
 * them itself: gadapt_forward_computes_coeffs) - 14 or 13 launches per step.  slab == NULL (data parallel): grad is given - the
 * caller all-reduced it - and the launches are step count, Adam (+ coefficients); its first half is the same call with slab given and
 * exp_avg = exp_avg_sq = NULL: the two sum launches (loss included), stopping at the flat gradient.
 * state = int32[2] {steps taken, 0} as for gadapt_adam_step_dev.
 * Bit-identical parameters, moments and coefficients to the separate launches (tests/test_gpu_training.py). */
int gadapt_step_tail(const float* slab /*nullable*/, int n_rows, float* scratch, float* param, float* grad, float* exp_avg,
                     float* exp_avg_sq, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t* state,
                     float grad_scale, float* a_out, float* p0_out,
                     const float* loss_partials /*nullable*/, int n_loss_partials, float* loss_out, int64_t loss_count,
                     int c, void* stream);
/* Narrow route with PACKED slab rows: a target-pass workgroup of the narrow backward owes 20 numbers, so a row is 32 floats instead of
 * c*c + c - entry 4*o + k = dA[o][k], entry 16 + o = dp0[o] (o, k < 4), entries 20..31 zero: one 128-byte line per workgroup.
 * gadapt_narrow_slab_floats = 32 * gadapt_backward_slab_rows at hidden 64.  gadapt_block_backward_narrow_packed: arguments, launches
 * and sums of gadapt_block_backward_narrow - the 20 live entries of every row carry the same bits - for ONE shared conv
 * (a_stride = p0_stride = 0); every float of the slab is written.  gadapt_step_tail_narrow: arguments of gadapt_step_tail, hidden 64,
 * slab = the packed slab (required, like scratch - unused, kept for the common argument list): ONE launch that sums the rows in the
 * order of gadapt_step_tail's first-level and second-level sums, keeps the chain-rule terms whose dA / dp0 factor can be non-zero,
 * runs Adam on the whole bucket, advances the step count and sums the loss partials; exp_avg = exp_avg_sq = NULL stops at the flat
 * gradient (state untouched).  Bit-identical to gadapt_step_tail on the full-width slab with the same live entries
 * (tests/test_gpu_narrow_tail.py).  The gradient-given form (no slab) stays with gadapt_step_tail. */
int64_t gadapt_narrow_slab_floats(int64_t n_nodes);
int gadapt_block_backward_narrow_packed(const gadapt_graph* g, const float* x_all, int x0_cols, const float* alpha_all,
                                        const float* g_top, int g_top_cols, int n_layers,
                                        const float* a, int64_t a_stride, const float* p0, int64_t p0_stride,
                                        const float* layer_params,
                                        float* g_ws, float* dxd_ws, float* edge_ws, float* slab,
                                        float* d_layer_params, int want_d_scale, float* d_x0, int c, void* stream);
int gadapt_step_tail_narrow(const float* slab, int n_rows, float* scratch, float* param, float* grad, float* exp_avg,
                            float* exp_avg_sq, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t* state,
                            float grad_scale, float* a_out, float* p0_out,
                            const float* loss_partials /*nullable*/, int n_loss_partials, float* loss_out, int64_t loss_count,
                            int c, void* stream);
/* gadapt_step_tail_narrow spread over row-owning workgroups (step_tail_narrow_spread_kernel; csrc/gadapt_tail_plan.h): a parameter
 * workgroup owns whole rows r of the bucket - Wq[r][:], bq[r], Wk[r][:], bk[r] - so the chain rule of its entries reads only parameters
 * it owns; every such workgroup sums the whole packed slab itself, in the one-workgroup kernel's order (bit-identical sums, nothing
 * exchanged), and runs Adam on its one or two entries per thread; with loss partials the loss workgroup is one more, the last.  The step
 * count, state = int32[2] {steps taken, 0}: every parameter workgroup reads state[0] with its first loads and uses state[0] + 1; one thread
 * then takes a ticket in state[1] (as gadapt_adam_step_dev does) and the workgroup whose ticket is the last stores state[1] = 0 and
 * state[0] = the new count.  No workgroup waits for another.  Gradient only: neither word is touched.  The host copies of the plan:
 * plan_host: plan_out[6] = {rows per parameter workgroup, threads per workgroup, parameter workgroups, slots per thread, workgroups of
 * the launch, tickets taken} with (has_loss != 0) or without loss partials; rows_host: rows of workgroup wg (the last may be short; -1: no
 * such workgroup); entry_host: out3 = {entry of the flat bucket or -1, row within the workgroup, place in the row: 0..63 Wq, 64 bq,
 * 65..128 Wk, 129 bk} of (wg, thread, slot); owner_host: out3 = {wg, thread, slot} of entry e. */
int gadapt_narrow_tail_plan_host(int has_loss, int32_t* plan_out);
int gadapt_narrow_tail_rows_host(int wg);
int gadapt_narrow_tail_entry_host(int wg, int thread, int slot, int32_t* out3);
int gadapt_narrow_tail_owner_host(int e, int32_t* out3);
/* The top layer's backward target pass inside the forward launch.  T_{L-1}, the first launch of gadapt_block_backward_narrow_packed, needs
 * nothing from another workgroup: its g row is the loss seed, and the last layer's forward holds its x rows, alpha, {dt, scale} and A.
 * gadapt_block_forward_loss_narrow_top is gadapt_block_forward_loss_narrow given the backward's dxd_ws, edge_ws and packed slab.  Where
 * the step is eligible the last forward launch also writes what T_{L-1} writes - dxd_ws [N,4], the {alpha dt, ds} pairs in edge_ws, all
 * gadapt_backward_slab_rows rows of the slab (rows without nodes: 32 zeros), the same bits - and *top_ran = 1; then
 * gadapt_block_backward_narrow_packed_below_top (the arguments of gadapt_block_backward_narrow_packed) runs the remaining launches, its
 * edge buffers alternating as if T_{L-1} had just written edge_ws.  Eligible: a block launch covers the top layer (a registered halo,
 * see gadapt_narrow_block_halo), a target, n_layers >= 2, the three buffers given, rows of at most 8 in-neighbours, n_edges > 0,
 * n_nodes <= 256 * gadapt_backward_slab_rows (one node per lane of T_{L-1}: n_nodes <= 131072), and the switch
 * gadapt_debug_set_narrow_top_in_forward on.  Otherwise *top_ran = 0, nothing but gadapt_block_forward_loss_narrow's results is written
 * and the backward is gadapt_block_backward_narrow_packed.  Returns the number of loss partials, like its namesake. */
int gadapt_block_forward_loss_narrow_top(const gadapt_graph* g, float* x_all, const float* x_comp, int dim, const float* f_tensor /*nullable*/,
                                         const float* uu_tensor /*nullable*/, int n_layers, float* a, float* p0, const float* param /*nullable*/,
                                         const float* layer_params, float* alpha_all, float* x_top4,
                                         const float* target, int d, int l1, float* seed, float* loss_partials,
                                         float* dxd_ws /*nullable*/, float* edge_ws /*nullable*/, float* slab /*nullable*/, int* top_ran,
                                         int c, void* stream);
int gadapt_block_backward_narrow_packed_below_top(const gadapt_graph* g, const float* x_all, int x0_cols, const float* alpha_all,
                                                  const float* g_top, int g_top_cols, int n_layers,
                                                  const float* a, int64_t a_stride, const float* p0, int64_t p0_stride,
                                                  const float* layer_params,
                                                  float* g_ws, float* dxd_ws, float* edge_ws, float* slab,
                                                  float* d_layer_params, int want_d_scale, float* d_x0, int c, void* stream);

/* The layers below the top in one launch.  gadapt_block_backward_narrow_packed_block takes the arguments of
 * gadapt_block_backward_narrow_packed, runs T_{L-1} itself when top_done = 0 (top_done = 1: behind gadapt_block_forward_loss_narrow_top with
 * *top_ran = 1) and then the fused stages [S_l + T_{l-1}], l = L-1 .. 1, as ONE launch per group of up to three stages (L = 3: one launch of
 * two, L = 4: one of three, L = 6: 3 + 2; gadapt_narrow_bwd_block_groups_host), stages separated by workgroup barriers, and sets
 * *block_ran = 1.  Eligible: the switches gadapt_debug_set_narrow_backward_block and gadapt_debug_set_narrow_backward_fused on; a source halo of 32 or 64 registered
 * (gadapt_narrow_block_register_source); one shared conv; n_edges > 0; ell_t, ell_s and tpos_s present, rows of at most 8 in both tables;
 * n_nodes <= 256 * gadapt_backward_slab_rows; n_layers >= 3; 2 E <= (c - 4) N (n_layers > 4: 2 E <= (c - 8) N).  Otherwise it runs exactly
 * the launches of gadapt_block_backward_narrow_packed / _below_top and sets *block_ran = 0.
 * Contract when *block_ran = 1 - the SLAB: entries 0..19 of rows 0 .. min(2 ceil(N / 512), rows) - 1 carry the bits those launches leave;
 * every other entry of the slab is not written by the block launches (the rows beyond hold the zeros of T_{L-1}, to which those launches
 * add +0).  Work buffers: each of g, dxd and the pairs has two members, laid out in csrc/gadapt_narrow_plan.h by gadapt_narrow_layout_of
 * - words 12..17 of a serialised plan, below - and the launches write exactly what their records in gadapt_narrow_step_plan name:
 *   top_done = 0: T_{L-1} writes member 0 of dxd and of the pairs, and every slab row;
 *   n_layers <= 4: nothing else - g_ws is not written at all, and with top_done = 1 neither are dxd_ws and edge_ws;
 *   n_layers > 4: launch number m = 0, 1, .. below T_{L-1} that is not the last stores, for every node, what the next one reads: g rows
 *     to member m & 1, dxd rows and the pairs to member (m + 1) & 1 - never a member it reads.  Nothing else. */
int gadapt_block_backward_narrow_packed_block(const gadapt_graph* g, const float* x_all, int x0_cols, const float* alpha_all,
                                              const float* g_top, int g_top_cols, int n_layers,
                                              const float* a, int64_t a_stride, const float* p0, int64_t p0_stride,
                                              const float* layer_params,
                                              float* g_ws, float* dxd_ws, float* edge_ws, float* slab,
                                              float* d_layer_params, int want_d_scale, float* d_x0, int c, void* stream,
                                              int top_done, int* block_ran);

/* The launch sequence of a narrow step, as the entry points above run it (csrc/gadapt_narrow_plan.h: one pure function of the facts of a
 * step and the four launch-sequence switches; read-only queries, nothing is launched; resolved by name, ABI 9).
 * The rules, all of them.  A step has launches only where gadapt_narrow_route = 1 and n_layers >= 1.  `One range`: n_nodes <= 256 *
 * gadapt_backward_slab_rows.  `Short rows`: the longest in-row the narrow forward walks is at most 8.
 *   FORWARD.  Groups of up to 4 consecutive layers, one launch each (L = 4: one, L = 6: 4 + 2), where gadapt_debug_set_narrow_forward is
 *   1, the conv is shared, the target side has a registered halo and the 512-node tiles keep the loss partials within
 *   gadapt_loss_partials_max; else one launch per layer - the one-node-per-lane kernel, or the wide kernel where the switch is 0.
 *   COEFFICIENTS FIRST.  With param given (flag COEFFS) gadapt_coeffs_forward comes first where the layer-0 launch has fewer than 64
 *   workgroups: one per 512-node tile of a group launch, one per 256-node step of a per-layer launch.
 *   TOP IN FORWARD.  The last forward launch also runs T_{L-1} where gadapt_debug_set_narrow_top_in_forward is on, the forward runs in
 *   groups, a target and the three backward buffers are given, n_layers >= 2, ell_t and tpos_s are present, n_edges > 0, short rows, one
 *   range.
 *   BACKWARD (n_layers >= 2), first T_{L-1} unless top_done, then one of:
 *     groups - the fused stages [S_l + T_{l-1}], l = L-1 .. 1, in launches of gadapt_narrow_bwd_block_groups_host stages - where the entry
 *       point reports *block_ran (flag MAY_BLOCK), gadapt_debug_set_narrow_backward_block and _backward_fused are on, the source side has a
 *       registered halo, packed slab, shared conv, n_layers >= 3, n_edges > 0, ell_t, ell_s, tpos_s and rowptr_s present, short rows, one
 *       range, and 2 E <= (c - 4) N (n_layers > 4: 2 E <= (c - 8) N);
 *     fused - one launch per stage - where gadapt_debug_set_narrow_backward_fused is on, ell_s, rowptr_s and col_s are present and
 *       2 E <= (c - 4) N;
 *     pairs - T_l, S_l for l = L-1 .. 1 (T_{L-1} only unless top_done), then the compact layer-0 target pass T_0 - otherwise.
 *   BUFFERS.  T_{L-1} (in either place) leaves dxd and the pairs in member 0 of their buffer pairs and writes every slab row (accumulate
 *   = 0); every later target pass of a shared conv accumulates.  Pairs: one member of dxd and of the pairs throughout; S_l writes g member
 *   (L - 1 - l) & 1.  Launch m = 0, 1, .. below T_{L-1} of fused / groups reads member m & 1 of the pairs and writes the other, writes g
 *   member m & 1 and reads the one the launch before wrote (m = 0: the top gradient); a group does with dxd as with the pairs, a fused
 *   launch keeps dxd in member 0 (row j is read and then written by the lane that owns node j).  The launch whose target half is layer 0
 *   writes slab rows only.
 * Serialised plan, int32 words.  Head [18]: 0 route (0: no launches), 1 forward launches, 2 backward launches, 3 forward kind (0 wide per
 * layer, 1 one node per lane per layer, 2 groups), 4 forward halo, 5 coefficients first, 6 top in forward (= *top_ran), 7 backward kind
 * (0 pairs, 1 fused, 2 groups), 8 backward halo, 9 top_done, 10 *block_ran, 11 words per record (13), 12..17 float offsets of the work
 * buffers: g members 0, 1 in g_ws, dxd members 0, 1 in dxd_ws, pairs member 0 in edge_ws and member 1 in dxd_ws (extents 4N, 4N, 2E).
 * Then one record per launch, forward first: 0 kind (0 wide forward, 1 one-node-per-lane forward, 2 forward group, 3 narrow target pass,
 * 4 narrow source pass, 5 compact layer-0 target pass, 6 fused stage, 7 group of fused stages), 1 layer (forward: first layer; backward:
 * the layer of the target pass, or of the (first) source pass), 2 layers / stages in the launch, 3 g read, 4 g written, 5 pairs read,
 * 6 pairs written, 7 dxd read, 8 dxd written (members; -1: none), 9 accumulate, 10 first (forward: starts at layer 0; backward: reads the
 * top gradient), 11 last (forward: ends the block; backward: target half is layer 0), 12 top (forward: T_{L-1} rides in the launch).
 * 18 + 39 n_layers words always hold a plan.  Both return the words written, or GADAPT_E_BADARG: NULL output, cap too small, sizes whose
 * offsets do not fit 32 bits (n_nodes c 4 >= 4 GiB, 8 N + 2 E >= 2^31), n_layers < 1.
 * gadapt_narrow_step_plan_host: facts = int64[22] {n_nodes, n_edges, c, n_layers, route takes the graph, target halo, source halo (0, 32,
 * 64), longest in-row, slab rows, tiles ok, ell_t, ell_s, tpos_s, rowptr_s, col_s present, shared conv, packed slab, target given,
 * backward buffers given, param given, top_done, may run groups}; switches = int32[4] {narrow_forward (0, 1, 2), backward_fused,
 * top_in_forward, backward_block}.
 * gadapt_narrow_step_plan: the plan the library would run right now on g (its registered halos, the live switches); flags: 1 shared conv,
 * 2 packed slab, 4 target given, 8 backward buffers given, 16 param given, 32 top_done, 64 may run groups. */
int gadapt_narrow_step_plan_host(const int64_t* facts, const int32_t* switches, int32_t* plan_out, int cap);
int gadapt_narrow_step_plan(const gadapt_graph* g, int c, int n_layers, int flags, int32_t* plan_out, int cap);

/* ------------------------------------------------------------------ small meshes: the whole evaluation forward in ONE launch
 * The reference's own sizes (params.py:37,56,107,130-134: 11x11 ... 23x23 meshes, hidden 8, 4 layers; evaluation one sample per call,
 * utils_eval.py:128-130,193-201; the Burgers rollout, utils_eval_Burgers.py:282-300): encoder (GNN.py:225-239,270), composite
 * coefficients, the L Euler steps (GNN.py:273-291 on GRAND_plus.py:225-343) and the head x[:, :out_cols] (GNN.py:299) by ONE workgroup
 * per mesh - the meshes of a batch are disconnected components, so only workgroup barriers are needed.  mesh_ptr [n_meshes+1]
 * (device): first node of each mesh (PyG's Batch.ptr); every edge must stay inside its mesh.  mesh_eptr (nullable, device)
 * [n_meshes+1]: first in-edge of each mesh = rowptr_t[mesh_ptr[m]] - given, a workgroup reads its node and edge bounds side by
 * side instead of one after the other (a dependent round trip of a ~10 us launch); n_meshes == 1 reads neither.
 * max_mesh_nodes / max_mesh_edges: the largest mesh
 * (<= 1024 nodes, 512 at hidden 32: one to four lanes per node; rows + CSR slice must fit 160 KB: gadapt_small_forward_lds_bytes returns the bytes, or -1).  hidden c in
 * {4, 8, 16, 32}.  x_comp [N,dim], f / uu [N] nullable, enc_w [c, n_feat] the frozen bias-free encoder weight; wq / bq / wk advance by
 * w_stride / b_stride floats per layer (0 = shared); layer_params [L,2] = (dt, score scale).  out [N,out_cols]; alpha_all nullable
 * [L,E] (target-CSR order).  No activations are kept: inference only. */
int64_t gadapt_small_forward_lds_bytes(int max_mesh_nodes, int max_mesh_edges, int c);
int gadapt_small_forward(const gadapt_graph* g, const int32_t* mesh_ptr, const int32_t* mesh_eptr, int n_meshes, int max_mesh_nodes, int max_mesh_edges,
                         const float* x_comp, int dim, const float* f, const float* uu, const float* enc_w, int n_feat,
                         const float* wq, const float* bq, const float* wk, int64_t w_stride, int64_t b_stride,
                         const float* layer_params, int n_layers, float* out, int out_cols, float* alpha_all, float* x_all, int c, void* stream);
/* The same launch as the head of a fused training step on a small-mesh batch (ABI 9): x_all / alpha_all are kept for
 * gadapt_small_backward, and the launch also writes seed = d loss / d out [N,out_cols] (loss = mean squared error over all N*out_cols
 * entries against target [N,out_cols], or mean absolute error when l1 != 0: run_GNN.py:80-84,106; the arithmetic of
 * gadapt_loss_forward, bit-identical gradients) and one partial sum of the loss per wave to loss_partials (gadapt_loss_partials_max()
 * floats; gadapt_step_tail sums them).  Returns the number of partials (> 0) or a negative error code.  1 <= out_cols <= 4. */
int gadapt_small_forward_loss(const gadapt_graph* g, const int32_t* mesh_ptr, const int32_t* mesh_eptr, int n_meshes, int max_mesh_nodes, int max_mesh_edges,
                              const float* x_comp, int dim, const float* f, const float* uu, const float* enc_w, int n_feat,
                              const float* wq, const float* bq, const float* wk, int64_t w_stride, int64_t b_stride,
                              const float* layer_params, int n_layers, float* out, int out_cols, float* alpha_all, float* x_all,
                              const float* target, int l1, float* seed, float* loss_partials, int c, void* stream);
/* x_all (nullable) [L,N,c]: when given, the input rows of every layer are kept for gadapt_small_backward (training; alpha_all must
 * be given too).
 * Backward of the same block in ONE launch, one workgroup per mesh (autograd of GRAND_plus.py:225-343 + GNN.py:288-291 through the
 * L layers; the encoder is frozen, GNN.py:82,89, so nothing is owed below layer 0): g_top = dL/dx_L[:, :g_cols] (zero beyond).
 * slab: [S][n_meshes][c*c + c] floats - per conv (S = 1 shared, L per-layer) one partial row per mesh (dA then dp0), the layout
 * gadapt_slab_reduce_coeffs_backward(slab + s * n_meshes * (c*c + c), n_meshes, ...) sums and chains to the Linear parameters. */
int64_t gadapt_small_backward_lds_bytes(int max_mesh_nodes, int max_mesh_edges, int c);
int gadapt_small_backward(const gadapt_graph* g, const int32_t* mesh_ptr, const int32_t* mesh_eptr, int n_meshes, int max_mesh_nodes, int max_mesh_edges,
                          const float* x_all, const float* alpha_all, const float* g_top, int g_cols,
                          const float* wq, const float* bq, const float* wk, int64_t w_stride, int64_t b_stride,
                          const float* layer_params, int n_layers, float* slab, int c, void* stream);

/* partials: the workspace gadapt_block_backward filled ([2][L][n_rows], n_rows = gadapt_backward_slab_rows).  d_layer_params
 * [2,L]: row 0 = d dt_l, row 1 = d score_scale_l (zeros when want_d_scale = 0) - two contiguous rows, so a caller can hand out
 * the d dt row as the gradients of L one-element step parameters laid side by side. */
int gadapt_layer_params_reduce(const float* partials, int n_rows, int n_layers, int want_d_scale, float* d_layer_params, void* stream);

/* ------------------------------------------------------------------ generic message-passing primitives
 * What PyG's MessagePassing.propagate / utils.softmax do with index_select + scatter, per CSR row, for the conv variants
 * besides GRAND / GRAND_plus that get_conv builds (GNN.py:108-124: GAT_plus GRAND_plus.py:386-416, GATConv, GCNConv), the
 * reg_skew scores (GRAND_plus.py:280-324) and hidden sizes the fused kernels are not built for.  Per-edge arrays are in
 * target-CSR order (like alpha_out).  transpose / by_source = 1 walks the source CSR (the transposed product a backward
 * pass needs).  C must be a multiple of 4.  Rows are summed in the caller's edge order: bit-reproducible.
 *   spmm:         out_i = sum_{e: j->i} w_e x_j (+ self_scale * x_i)      [transpose: out_j = sum_{e: j->i} w_e x_i]
 *                 w = NULL means w_e = 1.
 *   sddmm:        s_e = scale * <a_i, b_j> for e: j->i                    [transpose: scale * <a_j, b_i>]
 *   edge_softmax: alpha_e = exp(s_e - max_i) / (sum_i exp(.) + 1e-16) over the in-edges of i (PyG utils.softmax);
 *                 backward d_s_e = alpha_e (d_alpha_e - sum_i alpha d_alpha)
 *   edge_combine: o_e = u_src[j] + v_dst[i] (op 0) or u_src[j] * v_dst[i] (op 1) for e: j->i
 *   edge_rowsum:  r_i = sum of edge_vals over the in-edges of i           [by_source: over the out-edges of j]        */
int gadapt_spmm(const gadapt_graph* g, int transpose, const float* w /*nullable*/, const float* x, float* out, int c,
                float self_scale, void* stream);
int gadapt_sddmm(const gadapt_graph* g, int transpose, const float* a, const float* b, float* out, int c, float scale, void* stream);
int gadapt_edge_softmax_forward(const gadapt_graph* g, const float* scores, float* alpha, void* stream);
int gadapt_edge_softmax_backward(const gadapt_graph* g, const float* alpha, const float* d_alpha, float* d_scores, void* stream);
int gadapt_edge_combine(const gadapt_graph* g, const float* u_src, const float* v_dst, float* out, int op, void* stream);
int gadapt_edge_rowsum(const gadapt_graph* g, int by_source, const float* edge_vals, float* out, void* stream);
/* Per-edge VECTORS b [E,C] in target-CSR order (the conv option edge_dim / lin_edge, GRAND_plus.py:165-166: a per-edge term on
 * key and value, :273-277,338-340).  i = the target (row) of edge e.  C a multiple of 4.
 *   mode 0  s_e   = <a_i, b_e>                   out [E]      (score term <query_i, edge_e>; d w of mode 1)
 *   mode 1  out_i = sum_{e in row i} w_e b_e     out [N,C]    (aggregated edge term; d a of mode 0)
 *   mode 2  out_e = w_e a_i                      out [E,C]    (d b of modes 0 and 1)                                      */
int gadapt_edge_vector_op(const gadapt_graph* g, int mode, const float* w, const float* a, const float* b, float* out, int c, void* stream);

/* ------------------------------------------------------------------ GAT_plus block (fused)
 * Replaces, for conv_type = 'GAT_plus' (get_conv, GNN.py:120-121), the L iterations of GNN.forward's layer loop (GNN.py:273-296)
 * around GAT_plus.forward (GRAND_plus.py:400-416: GATConv attention with identity maps, re-applied as sparse(alpha)^T x):
 *     a = <x, att_src>, b = <x, att_dst>;  alpha_e = softmax_i(leaky_relu(a_j + b_i, 0.2)) over the in-edges e: j -> i of the
 *     SELF-LOOPED graph (GATConv: remove_self_loops + add_self_loops - `g` must be that graph);
 *     res_i = sum_e alpha_e x_j - x_i  (res_lap = 1, 'GAT_res_lap')  |  sum_e alpha_e x_j  (res_lap = 0, 'GAT_lin');
 *     x <- x + dt * non_lin(res)  (residual = 1)  |  x <- non_lin(res)  (residual = 0).
 * non_lin: 0 identity, 1 relu, 2 tanh, 3 sigmoid, 4 leaky_relu(0.01), 5 elu, 6 selu (get_nonlin, GNN.py:48-64).  Dropout is not
 * part of it (callers with dropout > 0 in training mode use the per-layer primitives below).
 * x_all [(L+1),N,C]: slot 0 = input, slot l+1 = output of layer l.  att_src / att_dst [C] per layer, att_stride floats apart
 * (0: one shared conv).  ab [L,2,N] (the per-node score halves of every layer) and alpha [L,max(E,1)] (target-CSR order of `g`)
 * are outputs the backward reads.  C in {4,...,128} like the GRAND kernels.
 * backward: g_top [N,C] = dL/dx_L; workspaces g_ws [2,N,C], gr_ws [N,C], dz_ws [max(E,1)], db_ws [N],
 * part_ws [gadapt_gat_plus_partial_rows(N,C), 2C]; d_att [S,2,C] = (d att_src | d att_dst) per distinct conv, written whole
 * (summed over the layers in a fixed order when shared: bit-reproducible); d_x0 [N,C] nullable. */
int gadapt_gat_plus_block_forward(const gadapt_graph* g, float* x_all, int n_layers, const float* att_src, const float* att_dst,
                                  int64_t att_stride, float dt, int residual, int res_lap, int non_lin, float* ab, float* alpha,
                                  int c, void* stream);
int gadapt_gat_plus_block_backward(const gadapt_graph* g, const float* x_all, const float* alpha, const float* ab, const float* g_top,
                                   int n_layers, const float* att_src, const float* att_dst, int64_t att_stride, float dt, int residual,
                                   int res_lap, int non_lin, float* g_ws, float* gr_ws, float* dz_ws, float* db_ws, float* part_ws,
                                   float* d_att, float* d_x0 /*nullable*/, int c, void* stream);
int gadapt_gat_plus_partial_rows(int64_t n_nodes, int c);

/* ------------------------------------------------------------------ loss seed
 * mesh_loss (run_GNN.py:80-84,106): loss = mean |x_phys - target|^p, p = 2 (mse) or 1 (l1),
 * x_phys = x_top[:, :d] (GNN.py:299).  Writes x_phys [N,d], g_top [N,C] (zero outside
 * the first d columns, scaled by grad_scale/(N*d)) and atomically adds the summed loss
 * (already divided by N*d) into loss_out[0] (caller zeroes it). */
int gadapt_mesh_loss_seed(const float* x_top, const float* target, float* x_phys, float* g_top,
                          float* loss_out, int64_t n_nodes, int d, int c, int l1, float grad_scale,
                          void* stream);

/* The training loop's loss, F.mse_loss / F.l1_loss(out, data.x_phys) with reduction 'mean'
 * (run_GNN.py:80-84,106), forward AND its derivative in one launch: pred [N,d] with a row stride of
 * pred_stride floats (the x[:, :dim] view of GNN.py:299 is not dense), target [N,d] dense;
 * loss_out[0] = the loss (fixed summation order), seed [N,d] = d loss / d pred.
 * scratch: gadapt_loss_scratch_floats() floats, zero-filled once by the caller; left zero-filled. */
int gadapt_loss_forward(const float* pred, int64_t pred_stride, const float* target, int64_t n_rows, int d,
                        int l1, float* seed, float* loss_out, float* scratch, void* stream);
int gadapt_loss_scratch_floats(void);

/* Batch assembly on the device (what PyG's DataLoader collation does on the host for the node fields, run_GNN.py:72-76, for a
 * dataset whose samples share one mesh): for up to GADAPT_GATHER_MAX fields k, dst[k][b, :] = src[k][idx[b], :] for b < n_take, rows
 * of row_floats[k] floats (x_comp, x_phys, f_tensor, uu_tensor ... stacked per sample).  idx: int64 on the device.  src / dst /
 * row_floats are host arrays of n_fields entries (device pointers inside).  One launch per batch. */
#define GADAPT_GATHER_MAX 8
int gadapt_gather_fields(int n_fields, const float* const* src, float* const* dst, const int64_t* row_floats, const int64_t* idx,
                         int n_take, void* stream);

/* Backward of the slice x_phys = x_top[:, :d] (GNN.py:299): g_top [N,C] = g_phys [N,d] zero-padded. */
int gadapt_pad_columns(const float* g_phys, float* g_top, int64_t n_nodes, int d, int c, void* stream);

/* ------------------------------------------------------------------ optimizer
 * torch.optim.Adam(lr, weight_decay) step on a flat fp32 bucket (run_GNN.py:88,128-131):
 * L2 weight decay added to the gradient, bias-corrected moments, eps outside the sqrt.
 * grad_scale multiplies the gradient first (1/world_size after an all-reduce SUM). */
int gadapt_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                     int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                     int step, float grad_scale, void* stream);

/* Same step with the step count on the device: state = int32[2] {steps taken so far, 0}, zero-filled once by the
 * caller and advanced by the launch itself - nothing in the argument list changes from step to step, so the launch can be
 * part of a captured hipGraph together with forward and backward. */
int gadapt_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                         int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                         int32_t* state, float grad_scale, void* stream);

/* ------------------------------------------------------------------ data-parallel gradient exchange
 * SUM (average = 0) or AVERAGE (average = 1) of a flat fp32 bucket over the ranks of an RCCL communicator, in place, enqueued
 * on `stream` (capturable like any RCCL collective).  Replaces what `torch.distributed` / DDP would do for the reference's
 * `loss.backward()` under data parallelism (src/run_GNN.py:106-131 runs single-process; SURVEY.md section 8(b) item 6 and 8(e): one
 * all-reduce of the 2(C^2+C)-float bucket per step).  `comm` is the CALLER's ncclComm_t (ncclCommInitRank, or the one a
 * framework hands out); the library owns no communicator and links no RCCL: it resolves ncclAllReduce from the librccl.so
 * already loaded in the process (or loads it), GADAPT_E_RUNTIME if there is none.  The Python mirror keeps using
 * torch.distributed (its process group owns the communicator); this entry point is for callers that hold their own. */
int gadapt_allreduce_flat(void* comm, float* bucket, int64_t n, int average, void* stream);

/* ------------------------------------------------------------------ global CNN features of a field (features.GlobalFeatureExtractorCNN, kernel='hip')
 * u / max|u| over the batch, four convolutions (3 taps at dim 1, 3 x 3 at dim 2; stride 1, zero padding 1; channels 1 -> mid -> mid -> mid ->
 * out) with SELU, average pool (src/feature_extractors.py:6-34).  One image shape per call: u [n_meshes][n0][n1] fp32, n0 = 1 at dim 1.
 * Weights as the Conv1d / Conv2d modules hold them: w_l [c_out][c_in][3] or [c_out][c_in][3][3], b_l [c_out]; nothing is copied or
 * reshaped.  One workgroup per mesh with its images in LDS, channel-major planes of (n0 + 2)(n1 + 2) floats with a zero border: the
 * forward holds 2 images of max(mid, out) planes, the backward 3, both beside a table of n0 n1 pixel offsets, and a call that needs
 * more than 65 536 bytes (the LDS a launch gets without asking for more) is refused: *_lds_bytes return that size (-1: dim outside {1, 2}, a size below 1, n0 != 1 at dim 1), so
 * at mid 8 / 16 / 32 / 64 the backward takes 2-D images up to 23 x 23 / 16 x 16 / 11 x 11 / 7 x 7.
 * Every sum has a fixed order and there are no floating-point atomics: two runs give the same bits, and a mesh's row of feat does
 * not depend on the other meshes of the batch beyond umax.  Argument checks run before anything is launched and need no GPU. */
int64_t gadapt_cnn_forward_lds_bytes(int dim, int n0, int n1, int mid, int out);
int64_t gadapt_cnn_backward_lds_bytes(int dim, int n0, int n1, int mid, int out);
/* floats of the saved activations [4][n_meshes, c_l, n0 n1] (c_l = mid, mid, mid, out), and of the packed parameters
 * w0, b0, w1, b1, w2, b2, w3, b3 */
int64_t gadapt_cnn_workspace_floats(int n_meshes, int dim, int n0, int n1, int mid, int out);
int gadapt_cnn_param_floats(int dim, int mid, int out);
/* feat [n_meshes][out].  umax: DEVICE pointer to max|u| over the whole batch (one float; the launch divides by it - zero gives NaN
 * like the reference).  acts (nullable): gadapt_cnn_workspace_floats floats, written for the backward. */
int gadapt_cnn_forward(const float* u, const float* umax, int n_meshes, int dim, int n0, int n1, int mid, int out,
                       const float* w0, const float* b0, const float* w1, const float* b1, const float* w2, const float* b2,
                       const float* w3, const float* b3, float* feat, float* acts, void* stream);
/* d_params [gadapt_cnn_param_floats]: the gradient of every weight and bias from d_feat [n_meshes][out] and the forward's acts, packed
 * in the order above (overwritten, not accumulated).  partials [n_meshes][gadapt_cnn_param_floats]: the per-mesh gradients the launch
 * leaves for the fixed-order sum over meshes, a second small launch (nullable at n_meshes = 1: the one mesh writes d_params itself).
 * No gradient wrt u. */
int gadapt_cnn_backward(const float* d_feat, const float* acts, const float* u, const float* umax, int n_meshes, int dim, int n0, int n1,
                        int mid, int out, const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                        const float* b2, const float* w3, const float* b3, float* partials, float* d_params, void* stream);

/* ------------------------------------------------------------------ timing (bench only)
 * When enabled, every launch of the three hot kernels is bracketed by hipEvents on its
 * stream; kernel_id 0 = forward, 1 = backward target pass, 2 = backward source pass.
 * gadapt_profile_read synchronises on the recorded events (host helper, not capturable). */
int gadapt_profile_enable(int on);
int gadapt_profile_read(int kernel_id, double* total_ms, int* count);
int gadapt_profile_samples(int kernel_id, double* out_ms, int cap);   /* returns the number written */
/* Variant of each recorded launch, aligned with gadapt_profile_samples: bit 0 = compact upstream gradient (g_top_cols),
 * bit 1 = compact layer input (x0_cols), bit 2 = head-only output (x_top4). */
int gadapt_profile_variants(int kernel_id, int* out, int cap);
int gadapt_profile_reset(void);
/* Dispatch share D of an event pair: n x one empty launch (kernel id 3, p1) and n x two empty launches (id 4, p2),
 * bracketed like the hot kernels; D = 2 p1 - p2. */
int gadapt_profile_calibrate(int n, void* stream);
/* Switch: 1 (the default; GADAPT_BWD_INPLACE=0 in the environment starts with 0) lets gadapt_block_backward keep a dense
 * layer's dxd rows in the buffer its source pass then writes g_out to - every lane group reads its dxd row before it stores the
 * same row of g_out - so a layer pair touches two [N,C] work buffers instead of three (dxd_ws then only serves layer 0 and the
 * 4-column pair).  Results are bit-identical either way (tests/test_gpu_ops.py::test_block_backward_inplace_is_bit_identical). */
int gadapt_debug_set_backward_inplace(int on);
/* Forward choice of the narrow route (gadapt_block_forward_narrow, gadapt_block_forward_loss_narrow); GADAPT_NARROW_FWD=0 / =2 in the
 * environment starts with that value.  1 (the default): the default choice - groups of up to 4 layers in one launch each where the
 * graph is registered with a halo (gadapt_narrow_block_register) and the conv is shared, else the one-node-per-lane kernel, one launch
 * per layer; 2: one launch per layer everywhere; 0: the wide kernel with its compact input, one launch per layer.  Results are
 * bit-identical all three ways (tests/test_gpu_narrow_forward.py, tests/test_gpu_narrow_block_forward.py). */
int gadapt_debug_set_narrow_forward(int on);
/* Switch: 1 (the default; GADAPT_NARROW_BWD_FUSED=0 in the environment starts with 0) lets gadapt_block_backward_narrow run the source
 * pass of each layer inside the target pass of the layer below (L launches instead of 2L - 1; the second edge buffer the fused launches
 * alternate with lives in the unused tail of dxd_ws); 0 runs the pair of launches per layer.  Results are bit-identical either way
 * (tests/test_gpu_narrow_backward.py). */
int gadapt_debug_set_narrow_backward_fused(int on);
/* Switch: 1 (the default; GADAPT_NARROW_TOP_FWD=0 in the environment starts with 0) lets gadapt_block_forward_loss_narrow_top run the top
 * layer's backward target pass inside its last forward launch where the step is eligible; 0 keeps the separate launch.  Results are
 * bit-identical either way (tests/test_gpu_narrow_top_in_forward.py). */
int gadapt_debug_set_narrow_top_in_forward(int on);
/* Switch: 1 (the default; GADAPT_NARROW_BWD_BLOCK=0 in the environment starts with 0) lets gadapt_block_backward_narrow_packed_block run the
 * layers below the top as one launch per group of up to three fused stages where the step is eligible; 0: the launches of
 * gadapt_block_backward_narrow_packed.  The slab carries the same bits either way. */
int gadapt_debug_set_narrow_backward_block(int on);
/* Switch: 1 (the default; GADAPT_NARROW_TAIL_SPREAD=0 in the environment starts with 0) lets gadapt_step_tail_narrow launch the tail
 * spread over row-owning workgroups (step_tail_narrow_spread_kernel); 0: the one-workgroup step_tail_narrow_kernel.  Results are
 * bit-identical either way (tests/test_gpu_narrow_tail_spread.py). */
int gadapt_debug_set_narrow_tail_spread(int on);
/* Diagnostic: runtime-reported workgroups per CU of {forward, backward target, backward source}. */
int gadapt_debug_occupancy(int c, int* out3);
/* Diagnostic: the wave sum of the slab partials (wave_sum_desc: DPP and lane-swap steps) beside the xor butterfly 32, 16, .., 1 on
 * __shfl_xor that defines it.  in [n_waves][64][n_values] (device): one workgroup of n_waves waves (1..16), lane l of wave w holds
 * in[w][l][0..n_values); out_shfl / out_desc, same shape: both sums as that lane sees them.  n_values = 1, 20 or 22.  The two must
 * agree bit for bit in every lane (tests/test_gpu_wave_sum_desc.py). */
int gadapt_debug_wave_sum_desc(const float* in, float* out_shfl, float* out_desc, int n_waves, int n_values, void* stream);
/* Diagnostic: wave_sum_scatter, the wave sum the block kernels use for their 20 slab partials (every exchange hands over half of the
 * values; each total ends in one lane), beside wave_sum_desc.  in [n_waves][64][20] (device), laid out as above; out_desc, same shape:
 * wave_sum_desc's sums as every lane sees them; out_scatter [n_waves][64]: what the helper returns to each lane; out_entry [n_waves][64]
 * int32: the entry that value is the total of, or -1.  Documented lanes: with base = 10 (lane >> 5) + 5 ((lane >> 4) & 1) and
 * c = lane & 15, lane c = 0, 4, 8, 12 of a row of 16 holds entry base + 0, 2, 1, 3 and lane c = 1 holds entry base + 4; the other 44
 * lanes hold no total.  out_scatter at those lanes must equal out_desc's lane-0 value of the entry bit for bit
 * (tests/test_gpu_wave_sum_scatter.py). */
int gadapt_debug_wave_sum_scatter(const float* in, float* out_desc, float* out_scatter, int* out_entry, int n_waves, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GADAPT_HIP_H */
