// gadapt_kernels.hip - fused GRAND attention-diffusion layer for gfx950 (MI355X).
//
// Three kernels carry the hot path:
//   grand_fwd_kernel<C>        x' = x + dt (sum_j alpha_ij x_j - x)            (target-centric)
//   grand_bwd_target_kernel<C> d(score), dP, weight-gradient partials, dxd     (target-centric)
//   grand_bwd_source_kernel<C> g_out = dxd + sum over out-edges                (source-centric)
// All three share one shape: a 256-thread workgroup owns tiles of TM consecutive nodes, C/8 lanes
// cover one node (two float4 per lane for C >= 32, one for C < 32: a gathered neighbour row is one or
// two coalesced reads), the tile's CSR slice sits in LDS, and workgroups of one XCD walk a contiguous
// node range.  The forward and the target pass keep the x rows of tiles t-1..t+1 in an LDS ring and
// gather from it when the tile's neighbours all lie there (per-tile metadata built with the graph);
// the [TM,C]x[C,C] projections run on the bf16 matrix cores with a three-piece split of both operands
// (fp32 accuracy, C >= 32) and on the VALU for C < 32.  Hidden 64 on row-major mesh batches runs the wide forward
// kernel of gadapt_wide.inc instead of grand_fwd_kernel.
//
// Round 3 added the kernels of the two bottom backward layers behind the identity (zero-pad) encoder:
//   grand_bwd_target_compact_kernel  layer 0 on the compact [N,4] input: the 4 x 4 corner of dA, one node per lane
//   grand_bwd_target_kernel<..,D4>   the layer above it: dxd as [N,4], dP A[:, :4] on the vector ALU, no projection phase
//   grand_bwd_source4_kernel         ... and its source pass: g_out as [N,4], three waves per SIMD
// and the per-workgroup partial sums of d dt / d score_scale (layer_params_reduce_block: no float atomics).
//
// Arithmetic follows /root/reference/src/GRAND_plus.py:225-343 and src/GNN.py:273-291 in the
// (A, p0) formulation described in include/gadapt_hip.h.

#include "gadapt_internal.h"
#include "gadapt_tail_plan.h"
#include <atomic>

// ------------------------------------------------------------------------------------------------
// error reporting
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[256] = "";
int gadapt_fail_(int code, const char* msg) { snprintf(g_err, sizeof(g_err), "%s", msg); return code; }
int gadapt_check_launch_(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e)); return GADAPT_E_LAUNCH; }
    return GADAPT_OK;
}
extern "C" const char* gadapt_last_error(void) { return g_err; }
extern "C" int gadapt_abi_version(void) { return 9; }   // 9: gadapt_graph::wide_half_deg_t, gadapt_wide_window_host(step); 8 (round 6): the wide backward, the strided tile walk and their graph fields / host helpers are gone (measured level twice: docs/measurements.md F, G); + fused training-step entry points
extern "C" int gadapt_clear_error(void) { g_err[0] = 0; return (int)hipGetLastError(); }
extern "C" int gadapt_supported_hidden_dim(int c) {
    return c == 4 || c == 8 || c == 16 || c == 32 || c == 64 || c == 128;
}

// ------------------------------------------------------------------------------------------------
// optional per-kernel timing (bench/roofline only): HIP events on the launch stream around every
// hot-kernel launch.  Off by default; when off the launch path touches none of this.
// ------------------------------------------------------------------------------------------------
struct ProfRec { int id, variant; hipEvent_t a, b; };
// Launches come from more than one host thread (forward: the Python thread, backward: autograd's worker thread), so the
// record list is guarded; the flag is read on every launch and stays a relaxed atomic.
static std::atomic<bool> g_prof_on{false};
static std::mutex g_prof_mu;
static std::vector<ProfRec> g_prof;
ProfScope::ProfScope(int id, hipStream_t s, int variant) : st(s) {
    if (!g_prof_on.load(std::memory_order_relaxed)) return;
    ProfRec r{id, variant, nullptr, nullptr};
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
    (void)hipEventRecord(r.a, st);
    eb = r.b;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.push_back(r);
    idx = (int)g_prof.size() - 1;
}
ProfScope::~ProfScope() { if (idx >= 0) (void)hipEventRecord(eb, st); }
#ifdef GADAPT_STAMPS
unsigned long long* g_stamp_buf = nullptr;
extern "C" int gadapt_debug_set_stamp_buffer(void* p) { g_stamp_buf = static_cast<unsigned long long*>(p); return 0; }
#endif
extern "C" int gadapt_profile_enable(int on) { g_prof_on.store(on != 0, std::memory_order_relaxed); return GADAPT_OK; }
extern "C" int gadapt_profile_read(int kernel_id, double* total_ms, int* count) {
    if (!total_ms || !count) return fail(GADAPT_E_BADARG, "profile_read: null pointer");
    double tot = 0.0; int n = 0;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_prof) {
        if (r.id != kernel_id) continue;
        float ms = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { tot += ms; ++n; }
    }
    *total_ms = tot; *count = n;
    return GADAPT_OK;
}
extern "C" int gadapt_profile_samples(int kernel_id, double* out_ms, int cap) {
    if (!out_ms || cap < 0) return fail(GADAPT_E_BADARG, "profile_samples: bad argument");
    int n = 0;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_prof) {
        if (r.id != kernel_id) continue;
        float ms = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess && n < cap) out_ms[n++] = ms;
    }
    return n;
}
extern "C" int gadapt_profile_variants(int kernel_id, int* out, int cap) {
    if (!out || cap < 0) return fail(GADAPT_E_BADARG, "profile_variants: bad argument");
    int n = 0;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_prof) {
        if (r.id != kernel_id) continue;
        float ms = 0.f;                                         // same filter as gadapt_profile_samples: entries stay aligned
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess && n < cap) out[n++] = r.variant;
    }
    return n;
}
// An event pair around a launch also times the dispatch of that launch.  gadapt_profile_calibrate brackets, the same
// way, n times ONE empty launch (kernel id 3) and n times TWO consecutive empty launches (id 4): with e = what one
// empty launch occupies, p1 = D + e and p2 = D + 2e, so the dispatch share of a pair is D = 2 p1 - p2.
__global__ void profile_empty_kernel() {}
extern "C" int gadapt_profile_calibrate(int n, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int i = 0; i < n; ++i) {
        {
            ProfScope prof(3, st);
            hipLaunchKernelGGL(profile_empty_kernel, dim3(1), dim3(64), 0, st);
        }
        {
            ProfScope prof(4, st);
            hipLaunchKernelGGL(profile_empty_kernel, dim3(1), dim3(64), 0, st);
            hipLaunchKernelGGL(profile_empty_kernel, dim3(1), dim3(64), 0, st);
        }
    }
    return check_launch("profile_empty_kernel");
}
extern "C" int gadapt_profile_reset(void) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    g_prof.clear();
    return GADAPT_OK;
}

#include "gadapt_small.inc"

// One launch of a small per-step kernel template at hidden size c: STMT runs with CC = c as a constant.  A c the kernels are not built
// for runs nothing (the entry points refuse it before they come here).
#define GADAPT_FOR_C(c, ...)                                                 \
    switch (c) {                                                             \
        case 4:   { constexpr int CC = 4;   __VA_ARGS__; } break;            \
        case 8:   { constexpr int CC = 8;   __VA_ARGS__; } break;            \
        case 16:  { constexpr int CC = 16;  __VA_ARGS__; } break;            \
        case 32:  { constexpr int CC = 32;  __VA_ARGS__; } break;            \
        case 64:  { constexpr int CC = 64;  __VA_ARGS__; } break;            \
        case 128: { constexpr int CC = 128; __VA_ARGS__; } break;            \
        default: break;                                                      \
    }

// The switches of the launch sequence, one row each: 1 unless the environment variable starts with one of `others` ('0', or '0' / '2'),
// read at first use - or whatever its setter (gadapt_debug_set_*) stored before or since.  What each one chooses between:
// include/gadapt_hip.h at its setter; every choice is bit-identical with the form it replaces (the tests named there).
//   SW_BWD_INPLACE        block backward: the source pass writes g_out over the dxd rows it has just read (same row, same lanes)
//   SW_NARROW_FWD         narrow forward: 1 groups of up to 4 layers where the graph has a halo, else one node per lane per layer; 2 the
//                         latter everywhere; 0 wide::fwd_kernel<XC = true> per layer
//   SW_NARROW_BWD_FUSED   narrow backward: each source pass inside the next layer's target pass, or the pair of launches
//   SW_NARROW_TOP_FWD     fused step: the top layer's target pass inside the block forward launch that seeds the loss
//   SW_NARROW_BWD_BLOCK   the backward layers below the top as one launch per group of up to three fused stages
//   SW_NARROW_TAIL_SPREAD the narrow tail spread over row-owning workgroups, or the one-workgroup kernel
enum { SW_BWD_INPLACE, SW_NARROW_FWD, SW_NARROW_BWD_FUSED, SW_NARROW_TOP_FWD, SW_NARROW_BWD_BLOCK, SW_NARROW_TAIL_SPREAD, SW_COUNT };
struct EnvSwitch { const char* name; const char* others; std::atomic<int> state{-1}; };
static EnvSwitch g_switch[SW_COUNT] = {{"GADAPT_BWD_INPLACE", "0"},        {"GADAPT_NARROW_FWD", "02"},      {"GADAPT_NARROW_BWD_FUSED", "0"},
                                       {"GADAPT_NARROW_TOP_FWD", "0"},     {"GADAPT_NARROW_BWD_BLOCK", "0"}, {"GADAPT_NARROW_TAIL_SPREAD", "0"}};
static int env_switch(int k) {
    EnvSwitch& s = g_switch[k];
    int v = s.state.load(std::memory_order_relaxed);
    if (v < 0) {
        const char* e = getenv(s.name);
        v = (e && e[0] && strchr(s.others, e[0])) ? e[0] - '0' : 1;
        s.state.store(v, std::memory_order_relaxed);
    }
    return v;
}
static int set_switch(int k, int v) { g_switch[k].state.store(v, std::memory_order_relaxed); return GADAPT_OK; }
extern "C" int gadapt_debug_set_backward_inplace(int on) { return set_switch(SW_BWD_INPLACE, on ? 1 : 0); }
extern "C" int gadapt_debug_set_narrow_forward(int on) { return set_switch(SW_NARROW_FWD, on == 0 ? 0 : (on == 2 ? 2 : 1)); }
extern "C" int gadapt_debug_set_narrow_backward_fused(int on) { return set_switch(SW_NARROW_BWD_FUSED, on ? 1 : 0); }
extern "C" int gadapt_debug_set_narrow_top_in_forward(int on) { return set_switch(SW_NARROW_TOP_FWD, on ? 1 : 0); }
extern "C" int gadapt_debug_set_narrow_backward_block(int on) { return set_switch(SW_NARROW_BWD_BLOCK, on ? 1 : 0); }
extern "C" int gadapt_debug_set_narrow_tail_spread(int on) { return set_switch(SW_NARROW_TAIL_SPREAD, on ? 1 : 0); }
static bool bwd_inplace_enabled() { return env_switch(SW_BWD_INPLACE) == 1; }
// the four that decide a narrow step's launches, read in one place
static gadapt_narrow_switches narrow_switches() {
    return {env_switch(SW_NARROW_FWD), env_switch(SW_NARROW_BWD_FUSED) == 1, env_switch(SW_NARROW_TOP_FWD) == 1, env_switch(SW_NARROW_BWD_BLOCK) == 1};
}

// one layer's backward: target pass, then - when a gradient is to be passed on - the source pass
static int launch_bwd(int c, const gadapt_graph* g, const LayerBwd& b, hipStream_t st) {
    if (int rc = gadapt_launch_bwd_target_c(c, g, b, st)) return rc;
    return b.g_out ? gadapt_launch_bwd_source_c(c, g, b, st) : GADAPT_OK;
}

// The flat parameter bucket [Wq | bq | Wk | bk] at hidden size c - and the flat gradient, laid out alike: float offsets of its parts
struct BucketAt { int bq, wk, bk; };
static BucketAt bucket_at(int c) { return {c * c, c * c + c, 2 * c * c + c}; }

static int check_graph(const gadapt_graph* g, int c) {
    if (!g || g->n_nodes <= 0 || g->n_edges < 0 || !g->rowptr_t || !g->col_t) return fail(GADAPT_E_BADARG, "bad graph");
    for (int k = 0; k < 3; ++k) if (!g->meta_t[k] || !g->meta_s[k]) return fail(GADAPT_E_BADARG, "graph without tile metadata (gadapt_tile_meta_host)");
    if ((int64_t)g->n_nodes * c * 4 >= ((int64_t)1 << 32)) return fail(GADAPT_E_BADARG, "n_nodes*C*4 must stay below 4 GiB (32-bit row offsets)");
    return GADAPT_OK;
}

// Diagnostic: what the runtime says about residency (blocks per CU) of the three hot kernels for hidden size c.
extern "C" int gadapt_debug_occupancy(int c, int* out3) {
    if (!out3) return fail(GADAPT_E_BADARG, "occupancy: null");
    if (!gadapt_supported_hidden_dim(c)) return fail(GADAPT_E_BADARG, "occupancy: unsupported hidden_dim");
    out3[0] = gadapt_occupancy_fwd_c(c); out3[1] = gadapt_occupancy_bwd_target_c(c); out3[2] = gadapt_occupancy_bwd_source_c(c);
    return GADAPT_OK;
}

// Diagnostic: wave_sum_desc (gadapt_common.inc) beside the butterfly it restates - the one place that still spells it with __shfl_xor.
// One workgroup of n_waves waves; thread t holds in[t][0..N) and writes both sums of its wave, as its lane sees them.
template <int N>
__global__ void wave_sum_desc_debug_kernel(const float* __restrict__ in, float* __restrict__ out_shfl, float* __restrict__ out_desc) {
    const size_t at = (size_t)threadIdx.x * N;
    float a[N], b[N];
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = b[k] = in[at + k];
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a[k] += __shfl_xor(a[k], off, 64);
    wave_sum_desc(b);
#pragma unroll
    for (int k = 0; k < N; ++k) { out_shfl[at + k] = a[k]; out_desc[at + k] = b[k]; }
}
extern "C" int gadapt_debug_wave_sum_desc(const float* in, float* out_shfl, float* out_desc, int n_waves, int n_values, void* stream) {
    if (!in || !out_shfl || !out_desc || n_waves < 1 || n_waves > 16) return fail(GADAPT_E_BADARG, "wave_sum_desc: null pointer, or not 1..16 waves");
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 block(64 * n_waves);
    if (n_values == 1) hipLaunchKernelGGL(wave_sum_desc_debug_kernel<1>, dim3(1), block, 0, st, in, out_shfl, out_desc);
    else if (n_values == 20) hipLaunchKernelGGL(wave_sum_desc_debug_kernel<20>, dim3(1), block, 0, st, in, out_shfl, out_desc);
    else if (n_values == 22) hipLaunchKernelGGL(wave_sum_desc_debug_kernel<22>, dim3(1), block, 0, st, in, out_shfl, out_desc);
    else return fail(GADAPT_E_BADARG, "wave_sum_desc: built for 1, 20 and 22 values per lane");
    return check_launch("wave_sum_desc_debug_kernel");
}

// Diagnostic: wave_sum_scatter (gadapt_common.inc) beside wave_sum_desc on the same 20 values per lane.  Thread t writes what
// wave_sum_desc leaves it with (out_desc[t][0..20)), what wave_sum_scatter returns to it (out_scatter[t]) and the entry the helper says
// that is the total of (out_entry[t], -1: none).
__global__ void wave_sum_scatter_debug_kernel(const float* __restrict__ in, float* __restrict__ out_desc, float* __restrict__ out_scatter,
                                              int* __restrict__ out_entry) {
    const size_t at = (size_t)threadIdx.x * 20;
    float a[20], b[20];
#pragma unroll
    for (int k = 0; k < 20; ++k) a[k] = b[k] = in[at + k];
    wave_sum_desc(a);
    const float tot = wave_sum_scatter(b, threadIdx.x & 63);
#pragma unroll
    for (int k = 0; k < 20; ++k) out_desc[at + k] = a[k];
    out_scatter[threadIdx.x] = tot;
    out_entry[threadIdx.x] = wave_sum_scatter_entry(threadIdx.x & 63);
}
extern "C" int gadapt_debug_wave_sum_scatter(const float* in, float* out_desc, float* out_scatter, int* out_entry, int n_waves, void* stream) {
    if (!in || !out_desc || !out_scatter || !out_entry || n_waves < 1 || n_waves > 16)
        return fail(GADAPT_E_BADARG, "wave_sum_scatter: null pointer, or not 1..16 waves");
    hipLaunchKernelGGL(wave_sum_scatter_debug_kernel, dim3(1), dim3(64 * n_waves), 0, static_cast<hipStream_t>(stream), in, out_desc, out_scatter, out_entry);
    return check_launch("wave_sum_scatter_debug_kernel");
}

extern "C" int gadapt_layer_forward(const gadapt_graph* g, const float* x_in, float* x_out, const float* a, const float* p0,
                                    const float* layer_params, float* alpha_out, int residual_only, int c, void* stream) {
    if (int rc = check_graph(g, c)) return rc;
    if (!x_in || !x_out || !a || !p0 || !layer_params || x_in == x_out) return fail(GADAPT_E_BADARG, "layer_forward: null or aliased pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    return gadapt_launch_fwd_c(c, g, LayerFwd{.x_in = x_in, .x_out = x_out, .a = a, .p0 = p0, .lp = layer_params, .alpha_out = alpha_out,
                                              .residual_only = residual_only}, st);
}

extern "C" int gadapt_backward_slab_rows(int64_t n_nodes, int c) {
    if (n_nodes <= 0) return fail(GADAPT_E_BADARG, "slab_rows: bad node count");
    return gadapt_slab_rows_c(n_nodes, c);
}
extern "C" int64_t gadapt_backward_slab_floats(int64_t n_nodes, int c) {
    const int rows = gadapt_backward_slab_rows(n_nodes, c);
    return rows < 0 ? rows : (int64_t)rows * (c * c + c);
}

extern "C" int gadapt_layer_backward(const gadapt_graph* g, const float* x_in, const float* g_in, const float* alpha,
                                     const float* a, const float* p0, const float* layer_params, float* edge_ws, float* dxd_ws,
                                     float* slab, int accumulate, float* sums_out, float* g_out, int residual_only, int c, void* stream) {
    if (int rc = check_graph(g, c)) return rc;
    if (!x_in || !g_in || !alpha || !a || !p0 || !layer_params || !edge_ws || !dxd_ws || !slab)
        return fail(GADAPT_E_BADARG, "layer_backward: null pointer");
    if (!g->tpos_s || (g_out && (!g->rowptr_s || !g->col_s))) return fail(GADAPT_E_BADARG, "layer_backward: source CSR missing");
    if (g_out == g_in || g_out == dxd_ws) return fail(GADAPT_E_BADARG, "layer_backward: g_out aliases an input");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // {d dt, d score_scale} side by side, atomically accumulated
    return launch_bwd(c, g, LayerBwd{.x_in = x_in, .g_in = g_in, .alpha = alpha, .a = a, .p0 = p0, .lp = layer_params, .edge_ws = edge_ws, .dxd = dxd_ws,
                                     .slab = slab, .accumulate = accumulate, .sums_out = sums_out, .sums_sc_out = sums_out ? sums_out + 1 : nullptr,
                                     .g_out = g_out, .residual_only = residual_only}, st);
}

extern "C" int gadapt_layer_params_reduce(const float* partials, int n_rows, int n_layers, int want_d_scale, float* d_layer_params, void* stream) {
    if (!partials || !d_layer_params || n_rows <= 0 || n_layers <= 0) return fail(GADAPT_E_BADARG, "layer_params_reduce: bad argument");
    hipLaunchKernelGGL(layer_params_reduce_kernel, dim3(2 * n_layers), dim3(256), 0, static_cast<hipStream_t>(stream), partials, n_rows, n_layers,
                       want_d_scale, d_layer_params);
    return check_launch("layer_params_reduce_kernel");
}

extern "C" int gadapt_slab_reduce(const float* slab, int n_rows, float* scratch, float* d_a, float* d_p0, int c, void* stream) {
    if (!slab || n_rows <= 0 || !scratch || !d_a || !d_p0 || !gadapt_supported_hidden_dim(c)) return fail(GADAPT_E_BADARG, "slab_reduce: bad argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int row_len = c * c + c;
    hipLaunchKernelGGL(slab_reduce1_kernel, dim3((row_len + 255) / 256, GADAPT_SLAB_CHUNKS), dim3(256), 0, st, slab, scratch,
                       n_rows, row_len);
    hipLaunchKernelGGL(slab_reduce2_kernel, dim3((row_len + 255) / 256), dim3(256), 0, st, scratch, d_a, d_p0, c);
    return check_launch("slab_reduce");
}

// second-level slab sums + chain rule to the Linear parameters (every workgroup repeats the second-level sums)
static void launch_reduce2_coeffs_bwd(int c, const float* scratch, const float* wq, const float* bq, const float* wk, float* d_wq, float* d_bq,
                                      float* d_wk, float* d_bk, hipStream_t st) {
    const int lds = (c * (c + 1) + c) * 4;
    int blocks = (2 * c * c + 2 * c + 1023) / 1024;             // one entry of the flat gradient per thread
    if (blocks > 33) blocks = 33;
    GADAPT_FOR_C(c, allow_lds(reduce2_coeffs_bwd_kernel<CC>, lds);
                 hipLaunchKernelGGL(reduce2_coeffs_bwd_kernel<CC>, dim3(blocks), dim3(1024), lds, st, scratch, wq, bq, wk, d_wq, d_bq, d_wk, d_bk));
}

// slab -> d_wq | d_bq | d_wk | d_bk in two launches (first-level partial sums, then second level + chain rule together)
extern "C" int gadapt_slab_reduce_coeffs_backward(const float* slab, int n_rows, float* scratch, const float* wq, const float* bq,
                                                  const float* wk, float* d_wq, float* d_bq, float* d_wk, float* d_bk, int c, void* stream,
                                                  const float* lp_partials, int n_layers, int want_d_scale, float* d_layer_params) {
    if (!slab || n_rows <= 0 || !scratch || !wq || !bq || !wk || !d_wq || !d_bq || !d_wk || !d_bk || !gadapt_supported_hidden_dim(c))
        return fail(GADAPT_E_BADARG, "slab_reduce_coeffs_backward: bad argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int row_len = c * c + c;
    const int nbx = (row_len + 255) / 256;
    if (lp_partials && (n_layers <= 0 || !d_layer_params)) return fail(GADAPT_E_BADARG, "slab_reduce_coeffs_backward: layer-parameter partials without a destination");
    hipLaunchKernelGGL(slab_reduce1_kernel, dim3(nbx + (lp_partials ? 2 * n_layers : 0), GADAPT_SLAB_CHUNKS), dim3(256), 0, st, slab, scratch, n_rows, row_len,
                       nbx, lp_partials, n_layers, want_d_scale, d_layer_params);
    launch_reduce2_coeffs_bwd(c, scratch, wq, bq, wk, d_wq, d_bq, d_wk, d_bk, st);
    return check_launch("slab_reduce_coeffs_backward");
}

extern "C" int gadapt_coeffs_forward(const float* wq, const float* bq, const float* wk, float* a_out, float* p0_out, int c, void* stream) {
    if (!wq || !bq || !wk || !a_out || !p0_out || c <= 0) return fail(GADAPT_E_BADARG, "coeffs_forward: bad argument");
    if (!gadapt_supported_hidden_dim(c)) return fail(GADAPT_E_BADARG, "coeffs_forward: unsupported hidden_dim");
    const int n = c * c + c;
    hipStream_t st = static_cast<hipStream_t>(stream);
    GADAPT_FOR_C(c, hipLaunchKernelGGL(coeffs_fwd_kernel<CC>, dim3((n + 255) / 256), dim3(256), 0, st, wq, bq, wk, a_out, p0_out));
    return check_launch("coeffs_fwd_kernel");
}
extern "C" int gadapt_coeffs_backward(const float* wq, const float* bq, const float* wk, const float* d_a, const float* d_p0,
                                      float* d_wq, float* d_bq, float* d_wk, float* d_bk, int c, void* stream) {
    if (!wq || !bq || !wk || !d_a || !d_p0 || !d_wq || !d_bq || !d_wk || !d_bk || c <= 0) return fail(GADAPT_E_BADARG, "coeffs_backward: bad argument");
    if (!gadapt_supported_hidden_dim(c)) return fail(GADAPT_E_BADARG, "coeffs_backward: unsupported hidden_dim");
    const int n = 2 * c * c + 2 * c;
    hipStream_t st = static_cast<hipStream_t>(stream);
    GADAPT_FOR_C(c, hipLaunchKernelGGL(coeffs_bwd_kernel<CC>, dim3((n + 255) / 256), dim3(256), 0, st, wq, bq, wk, d_a, d_p0, d_wq, d_bq, d_wk, d_bk));
    return check_launch("coeffs_bwd_kernel");
}

struct wq_t { const float* wq; const float* bq; const float* wk; float* a; float* p0; int c; };
static int launch_encode(const float* feats, int f0, const float* e1, const float* e2, const float* w, const float* b, float* x0,
                         int64_t n_nodes, int c, void* stream, const void* coeffs = nullptr) {
    const int f = f0 + (e1 ? 1 : 0) + (e2 ? 1 : 0);
    if (c % 4 || c > 256 || 256 % (c / 4) || (int64_t)c * f > GADAPT_ENC_MAX_WORDS)
        return fail(GADAPT_E_BADARG, "encode: need hidden_dim in {4,8,...,256} dividing 1024 and hidden_dim*in_dim <= 4096");
    const int rows_per_block = 256 / (c / 4);
    int64_t blocks = (n_nodes + 4 * rows_per_block - 1) / (4 * rows_per_block);    // four rows per thread and iteration
    if (blocks > 1024) blocks = 1024;                                              // resident set: the W^T table is staged once per block
    if (blocks < 1) blocks = 1;
    const wq_t* cf = static_cast<const wq_t*>(coeffs);
    EncArgs p{feats, f0, e1, e2, w, b, x0, n_nodes, f, c};
    if (!cf) {
        hipLaunchKernelGGL(encode_linear_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), p);
        return check_launch("encode_linear_kernel");
    }
    if (!gadapt_supported_hidden_dim(cf->c)) return fail(GADAPT_E_BADARG, "encode_features_coeffs: unsupported hidden_dim");
    const int cblocks = (cf->c * cf->c + cf->c + 255) / 256;
    GADAPT_FOR_C(cf->c, hipLaunchKernelGGL(encode_coeffs_kernel<CC>, dim3((unsigned)blocks + cblocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                                           p, (int)blocks, cf->wq, cf->bq, cf->wk, cf->a, cf->p0));
    return check_launch("encode_coeffs_kernel");
}
extern "C" int gadapt_encode_linear(const float* feats, const float* w, const float* b, float* x0, int64_t n_nodes, int f, int c, void* stream) {
    if (!feats || !w || !x0 || n_nodes <= 0 || f <= 0 || c <= 0) return fail(GADAPT_E_BADARG, "encode_linear: bad argument");
    return launch_encode(feats, f, nullptr, nullptr, w, b, x0, n_nodes, c, stream);
}
extern "C" int gadapt_encode_features(const float* x_comp, int dim, const float* f_tensor, const float* uu_tensor, const float* w,
                                      const float* b, float* x0, int64_t n_nodes, int c, void* stream) {
    if (!x_comp || !w || !x0 || n_nodes <= 0 || dim <= 0 || c <= 0) return fail(GADAPT_E_BADARG, "encode_features: bad argument");
    // the kernel reads "first extra" then "second extra": with only uu present it is the first one
    return launch_encode(x_comp, dim, f_tensor ? f_tensor : uu_tensor, f_tensor ? uu_tensor : nullptr, w, b, x0, n_nodes, c, stream);
}
extern "C" int gadapt_encode_features_coeffs(const float* x_comp, int dim, const float* f_tensor, const float* uu_tensor, const float* w,
                                             const float* b, float* x0, int64_t n_nodes, int c, const float* wq, const float* bq,
                                             const float* wk, float* a_out, float* p0_out, int c_conv, void* stream) {
    if (!x_comp || !w || !x0 || n_nodes <= 0 || dim <= 0 || c <= 0 || !wq || !bq || !wk || !a_out || !p0_out)
        return fail(GADAPT_E_BADARG, "encode_features_coeffs: bad argument");
    if (!gadapt_supported_hidden_dim(c_conv)) return fail(GADAPT_E_BADARG, "encode_features_coeffs: unsupported hidden_dim");
    const wq_t cf{wq, bq, wk, a_out, p0_out, c_conv};
    return launch_encode(x_comp, dim, f_tensor ? f_tensor : uu_tensor, f_tensor ? uu_tensor : nullptr, w, b, x0, n_nodes, c, stream, &cf);
}
extern "C" int gadapt_loss_forward(const float* pred, int64_t pred_stride, const float* target, int64_t n_rows, int d, int l1,
                                   float* seed, float* loss_out, float* scratch, void* stream) {
    if (!pred || !target || !seed || !loss_out || !scratch || n_rows <= 0 || d <= 0 || pred_stride < d)
        return fail(GADAPT_E_BADARG, "loss_forward: bad argument");
    int64_t blocks = (n_rows + 255) / 256;
    if (blocks > GADAPT_LOSS_BLOCKS) blocks = GADAPT_LOSS_BLOCKS;
    hipLaunchKernelGGL(loss_forward_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), pred, pred_stride, target,
                       n_rows, d, l1, seed, loss_out, scratch);
    return check_launch("loss_forward_kernel");
}
extern "C" int gadapt_loss_scratch_floats(void) { return GADAPT_LOSS_BLOCKS + 1; }

// ---- gradient exchange: the caller's RCCL communicator, ncclAllReduce resolved at run time (no link-time dependency: the process
// usually has an RCCL loaded already - torch ships one - and a second copy must not come in with this library)
#include <dlfcn.h>
extern "C" int gadapt_allreduce_flat(void* comm, float* bucket, int64_t n, int average, void* stream) {
    if (!comm || !bucket || n <= 0) return fail(GADAPT_E_BADARG, "allreduce_flat: null communicator / bucket or empty bucket");
    // ncclResult_t ncclAllReduce(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t)
    typedef int (*allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
    static std::atomic<allreduce_fn> fn{nullptr};
    allreduce_fn f = fn.load(std::memory_order_acquire);
    if (!f) {
        void* h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);          // the copy the process already uses, if any
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return fail(GADAPT_E_RUNTIME, "allreduce_flat: no librccl.so in this process or on the library path");
        f = reinterpret_cast<allreduce_fn>(dlsym(h, "ncclAllReduce"));
        if (!f) return fail(GADAPT_E_RUNTIME, "allreduce_flat: librccl.so without ncclAllReduce");
        fn.store(f, std::memory_order_release);
    }
    constexpr int NCCL_FLOAT32 = 7, NCCL_SUM = 0, NCCL_AVG = 4;          // rccl.h: ncclFloat, ncclSum, ncclAvg
    const int rc = f(bucket, bucket, (size_t)n, NCCL_FLOAT32, average ? NCCL_AVG : NCCL_SUM, comm, static_cast<hipStream_t>(stream));
    if (rc != 0) return fail(GADAPT_E_RUNTIME, "allreduce_flat: ncclAllReduce failed");
    return GADAPT_OK;
}

// ------------------------------------------------------------------------------------------------
// batch assembly on the device: sample rows of up to GADAPT_GATHER_MAX stacked per-sample fields -> the batch's node fields
// ------------------------------------------------------------------------------------------------
struct GatherArgs {
    const float* src[GADAPT_GATHER_MAX]; float* dst[GADAPT_GATHER_MAX]; int64_t row[GADAPT_GATHER_MAX];   // row: floats per sample
    const int64_t* idx; int n_fields, n_take;
};
__global__ __launch_bounds__(256) void gather_fields_kernel(GatherArgs p) {
    const int f = blockIdx.z, b = blockIdx.y;
    if (f >= p.n_fields) return;
    const int64_t row = p.row[f];
    const float* s = p.src[f] + p.idx[b] * row;
    float* d = p.dst[f] + (int64_t)b * row;
    if ((row & 3) == 0 && ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 15) == 0) {
        const int64_t n4 = row >> 2;
        for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n4; e += (int64_t)gridDim.x * 256)
            reinterpret_cast<float4*>(d)[e] = reinterpret_cast<const float4*>(s)[e];
    } else {
        for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < row; e += (int64_t)gridDim.x * 256) d[e] = s[e];
    }
}
extern "C" int gadapt_gather_fields(int n_fields, const float* const* src, float* const* dst, const int64_t* row_floats, const int64_t* idx,
                                    int n_take, void* stream) {
    if (n_fields <= 0 || n_fields > GADAPT_GATHER_MAX || !src || !dst || !row_floats || !idx || n_take <= 0)
        return fail(GADAPT_E_BADARG, "gather_fields: 1..GADAPT_GATHER_MAX fields, a sample index vector and a positive count");
    GatherArgs p{};
    int64_t longest = 0;
    for (int f = 0; f < n_fields; ++f) {
        if (!src[f] || !dst[f] || row_floats[f] <= 0) return fail(GADAPT_E_BADARG, "gather_fields: null field or empty row");
        p.src[f] = src[f]; p.dst[f] = dst[f]; p.row[f] = row_floats[f];
        longest = row_floats[f] > longest ? row_floats[f] : longest;
    }
    p.idx = idx; p.n_fields = n_fields; p.n_take = n_take;
    int bx = (int)((longest / 4 + 255) / 256);
    bx = bx < 1 ? 1 : (bx > 32 ? 32 : bx);
    hipLaunchKernelGGL(gather_fields_kernel, dim3(bx, n_take, n_fields), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    return check_launch("gather_fields_kernel");
}

extern "C" int gadapt_pad_columns(const float* g_phys, float* g_top, int64_t n_nodes, int d, int c, void* stream) {
    if (!g_phys || !g_top || n_nodes <= 0 || d <= 0 || d > c || c % 4) return fail(GADAPT_E_BADARG, "pad_columns: bad argument");
    const int64_t n = n_nodes * (c / 4);
    hipLaunchKernelGGL(pad_columns_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), g_phys, g_top, n_nodes, d, c);
    return check_launch("pad_columns_kernel");
}

extern "C" int gadapt_mesh_loss_seed(const float* x_top, const float* target, float* x_phys, float* g_top, float* loss_out,
                                     int64_t n_nodes, int d, int c, int l1, float grad_scale, void* stream) {
    if (!x_top || !target || !x_phys || !g_top || !loss_out || n_nodes <= 0 || d <= 0 || d > c) return fail(GADAPT_E_BADARG, "mesh_loss_seed: bad argument");
    const int64_t n = n_nodes * c;
    hipLaunchKernelGGL(mesh_loss_seed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x_top, target,
                       x_phys, g_top, loss_out, n_nodes, d, c, l1, grad_scale);
    return check_launch("mesh_loss_seed_kernel");
}

extern "C" int gadapt_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                                float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step <= 0) return fail(GADAPT_E_BADARG, "adam_step: bad argument");
    const float bc1 = 1.0f - powf(beta1, (float)step);
    const float bc2_sqrt = sqrtf(1.0f - powf(beta2, (float)step));
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), param, grad,
                       exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale);
    return check_launch("adam_step_kernel");
}

extern "C" int gadapt_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                                    float beta2, float eps, float weight_decay, int32_t* state, float grad_scale, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || !state) return fail(GADAPT_E_BADARG, "adam_step_dev: bad argument");
    hipLaunchKernelGGL(adam_step_dev_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), param, grad,
                       exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, state, grad_scale);
    return check_launch("adam_step_dev_kernel");
}

// ------------------------------------------------------------------------------------------------
// L-step Euler block (GNN.py:273-291)
// ------------------------------------------------------------------------------------------------
// The narrow route (hidden 64, every layer on [N,4] rows).  Which launches a step runs is decided by gadapt_narrow_plan_of
// (gadapt_narrow_plan.h) from the facts gathered here and the switches above; the entry points below walk the plan.
//
// The halo of a block launch is a property of the graph that only the host build can know (gadapt_narrow_block_halo_host reads the CSR
// on the host; gadapt_graph holds device pointers and its layout is frozen at ABI 9).  The caller registers it once per graph and side
// - target: the in-edges (rowptr_t, ell_t), the forward groups; source: the out-edges (rowptr_s, ell_s), the backward groups - keyed by
// what identifies that side's device arrays; an unregistered graph has halo 0.
struct HaloEntry { const void* rowptr; const void* ell; int32_t n_nodes, n_edges; int halo; };
enum { SIDE_TARGET, SIDE_SOURCE };
static std::mutex g_halo_mu;
static std::vector<HaloEntry> g_halo[2];
static HaloEntry halo_key(const gadapt_graph* g, int side) {
    return side == SIDE_TARGET ? HaloEntry{g->rowptr_t, g->ell_t, g->n_nodes, g->n_edges, 0} : HaloEntry{g->rowptr_s, g->ell_s, g->n_nodes, g->n_edges, 0};
}
static bool halo_is(const HaloEntry& e, const HaloEntry& k) { return e.rowptr == k.rowptr && e.ell == k.ell && e.n_nodes == k.n_nodes && e.n_edges == k.n_edges; }
static int halo_register(const gadapt_graph* g, int side, int halo, const char* refusal) {
    if (!g || g->n_nodes <= 0 || (halo != 0 && halo != 32 && halo != 64)) return fail(GADAPT_E_BADARG, refusal);
    HaloEntry k = halo_key(g, side);
    if (!k.rowptr || !k.ell) return fail(GADAPT_E_BADARG, refusal);
    std::vector<HaloEntry>& v = g_halo[side];
    std::lock_guard<std::mutex> lk(g_halo_mu);
    for (size_t i = 0; i < v.size(); ++i)
        if (halo_is(v[i], k)) { v[i] = v.back(); v.pop_back(); break; }
    k.halo = halo;
    if (halo) v.push_back(k);
    return GADAPT_OK;
}
static int halo_registered(const gadapt_graph* g, int side) {
    const HaloEntry k = halo_key(g, side);
    if (!k.rowptr || !k.ell) return 0;
    std::lock_guard<std::mutex> lk(g_halo_mu);
    for (const HaloEntry& e : g_halo[side])
        if (halo_is(e, k)) return e.halo;
    return 0;
}
extern "C" int gadapt_narrow_block_register(const gadapt_graph* g, int halo) {
    return halo_register(g, SIDE_TARGET, halo, "narrow_block_register: a graph with its ELL copy, halo 0 (forget), 32 or 64");
}
extern "C" int gadapt_narrow_block_register_source(const gadapt_graph* g, int halo) {
    return halo_register(g, SIDE_SOURCE, halo, "narrow_block_register_source: a graph with the ELL copy of its out-edges, halo 0 (forget), 32 or 64");
}

// What is known about a step on graph g (not NULL) at hidden size c, gathered once per entry-point call: the graph's side (one registry
// lookup per side) and the call's (flags).
enum { NF_SHARED = 1, NF_PACKED = 2, NF_TARGET = 4, NF_BUFFERS = 8, NF_COEFFS = 16, NF_TOP_DONE = 32, NF_MAY_BLOCK = 64 };
static_assert(GADAPT_NARROW_ROW_MAX == GADAPT_MAXD, "the rows the one-node-per-lane kernels take from registers");
static gadapt_narrow_facts narrow_facts(const gadapt_graph* g, int c, int n_layers, int flags) {
    gadapt_narrow_facts f{};
    f.n_nodes = g->n_nodes; f.n_edges = g->n_edges; f.c = c; f.n_layers = n_layers;
    f.ell_t = g->ell_t != nullptr; f.ell_s = g->ell_s != nullptr; f.tpos_s = g->tpos_s != nullptr;
    f.rowptr_s = g->rowptr_s != nullptr; f.col_s = g->col_s != nullptr;
    f.shared = (flags & NF_SHARED) != 0; f.packed = (flags & NF_PACKED) != 0; f.target = (flags & NF_TARGET) != 0;
    f.buffers = (flags & NF_BUFFERS) != 0; f.coeffs = (flags & NF_COEFFS) != 0; f.top_done = (flags & NF_TOP_DONE) != 0;
    f.may_block = (flags & NF_MAY_BLOCK) != 0;
    f.takes = g->n_nodes > 0 && gadapt_narrow_takes_c(g, c);
    if (!f.takes) return f;                                      // (no launches: the rest is not looked at)
    f.halo_t = halo_registered(g, SIDE_TARGET); f.halo_s = halo_registered(g, SIDE_SOURCE);
    f.kmax = gadapt_narrow_kmax_c(g);
    f.slab_rows = gadapt_slab_rows_c(g->n_nodes, c);
    f.tiles_ok = gadapt_narrow_block_tiles_ok_c(g);
    return f;
}
static gadapt_narrow_plan narrow_plan(const gadapt_graph* g, int c, int n_layers, int flags) {
    const gadapt_narrow_facts f = narrow_facts(g, c, n_layers, flags);
    const gadapt_narrow_switches s = narrow_switches();
    return gadapt_narrow_plan_of(&f, &s);
}
// the halo the forward groups run with on this graph at this hidden size under the current forward choice, or 0: per-layer launches
extern "C" int gadapt_narrow_block_halo(const gadapt_graph* g, int c) { return g ? narrow_plan(g, c, 1, NF_SHARED).fwd_halo : 0; }
// The plan the library would run right now on this graph (registered halos, live switches), as int32 words; nothing is launched.
extern "C" int gadapt_narrow_step_plan(const gadapt_graph* g, int c, int n_layers, int flags, int32_t* plan_out, int cap) {
    if (!g || !plan_out || n_layers < 1 || flags < 0 || flags >= 2 * NF_MAY_BLOCK || !gadapt_narrow_sizes_ok(g->n_nodes, g->n_edges, c))
        return fail(GADAPT_E_BADARG, "narrow_step_plan: a graph, 1 or more layers, known flags, somewhere to write, sizes whose offsets fit 32 bits");
    const gadapt_narrow_plan p = narrow_plan(g, c, n_layers, flags);
    const int n = gadapt_narrow_plan_write(&p, plan_out, cap);
    return n < 0 ? fail(GADAPT_E_BADARG, "narrow_step_plan: cap is smaller than the plan (18 + 39 n_layers words always hold one)") : n;
}

// A block of n_layers Euler steps as its entry points see it (built once their checks have passed): where layer l finds its input slot,
// coefficients, {dt, scale}, alpha, slab and gradient buffer.  x_all and alpha_all are written by the forward and read by the backward;
// the slab fields and g_ws are the backward's.
struct Block {
    const gadapt_graph* g; int c, n_layers;
    float* x_all; size_t nc;                                    // slot l: [N,C] rows (compact / narrow: [N,4] rows at its start), nc = N * C
    const float* a_all; int64_t a_stride; const float* p0_all; int64_t p0_stride;   // stride 0: one shared conv
    const float* layer_params; float* alpha_all;                // alpha_all nullable (forward)
    float* slab_all; int64_t slab_floats; bool shared;          // shared: one slab, accumulated over the layers; else one per layer
    float* g_ws;                                                // two [N,C] buffers the layers alternate between
    float* x(int l) const { return x_all + l * nc; }
    const float* a(int l) const { return a_all + l * a_stride; }
    const float* p0(int l) const { return p0_all + l * p0_stride; }
    const float* lp(int l) const { return layer_params + 2 * l; }
    float* alpha(int l) const { return alpha_all ? alpha_all + (size_t)l * g->n_edges : nullptr; }
    float* slab(int l) const { return shared ? slab_all : slab_all + (size_t)l * slab_floats; }
    float* g_buf(int l) const { return g_ws + ((n_layers - 1 - l) & 1) * nc; }
};
// The extras of a fused step for one launch of its block: the node fields and the weights (in-kernel coefficients) go to the first
// launch, the loss to the last
static FwdExtra slice_extra(const FwdExtra& e, bool first, bool last, bool top) {
    FwdExtra s{};
    if (first) { s.fs = e.fs; s.x0c = e.x0c; s.cw = e.cw; s.a_out = e.a_out; s.p0_out = e.p0_out; }
    if (last) { s.loss = e.loss; s.n_partials_out = e.n_partials_out; }
    if (top) s.top = e.top;
    return s;
}
// The forward launches of a narrow plan: [N,4] slot in, [N,4] slot out (the last launch: the head rows).  A later group reads its input
// slot from global memory, where the owners of the group before wrote it (the backward needs it there anyway).
static int walk_forward_narrow(const Block& b, const gadapt_narrow_plan& plan, float* x_top4, const FwdExtra* extra, hipStream_t st) {
    for (int i = 0; i < plan.n_fwd; ++i) {
        const gadapt_narrow_launch r = gadapt_narrow_fwd_launch(&plan, i);
        const int l = r.layer;
        FwdExtra ex_l{};
        if (extra) ex_l = slice_extra(*extra, r.first, r.last, r.top);
        LayerFwd f{.x_in = b.x(l), .a = b.a(l), .p0 = b.p0(l), .lp = b.lp(l), .alpha_out = b.alpha(l), .extra = extra ? &ex_l : nullptr};
        int rc;
        if (r.kind == GADAPT_NARROW_L_FWD_GROUP) {
            f.x_top4 = b.x(l + 1);
            rc = gadapt_launch_fwd_narrow_block_c(b.c, b.g, f, plan.fwd_halo, r.count, (int64_t)b.nc, b.g->n_edges, r.last ? x_top4 : nullptr, st);
        } else {
            f.x_top4 = r.last ? x_top4 : b.x(l + 1);
            f.x_cols = 4;                                        // (read by the wide kernel only)
            rc = r.kind == GADAPT_NARROW_L_FWD_NODE ? gadapt_launch_fwd_narrow_c(b.c, b.g, f, st) : gadapt_launch_fwd_c(b.c, b.g, f, st);
        }
        if (rc) return rc;
    }
    return GADAPT_OK;
}
// narrow: the narrow route, by the plan its caller obtained - or, given none, by the one of a plain forward
static int block_forward(const gadapt_graph* g, float* x_all, int x0_cols, int n_layers, const float* a, int64_t a_stride,
                         const float* p0, int64_t p0_stride, const float* layer_params, float* alpha_all, float* x_top4,
                         int c, void* stream, const FwdExtra* extra, bool narrow = false, const gadapt_narrow_plan* plan = nullptr) {
    if (int rc = check_graph(g, c)) return rc;
    if (!x_all || n_layers <= 0 || !a || !p0 || !layer_params) return fail(GADAPT_E_BADARG, "block_forward: bad argument");
    if (x0_cols != 0 && (x0_cols != 4 || n_layers < 2 || c < 8)) return fail(GADAPT_E_BADARG, "block_forward: compact x0 needs 4 columns, >= 2 layers, hidden >= 8");
    if (narrow && (x0_cols != 4 || !x_top4 || !gadapt_narrow_takes_c(g, c)))
        return fail(GADAPT_E_BADARG, "block_forward (narrow): compact x0, head rows, hidden 64 on a graph the wide forward takes (gadapt_narrow_route)");
    const Block b{.g = g, .c = c, .n_layers = n_layers, .x_all = x_all, .nc = (size_t)g->n_nodes * c, .a_all = a, .a_stride = a_stride, .p0_all = p0,
                  .p0_stride = p0_stride, .layer_params = layer_params, .alpha_all = alpha_all};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (narrow) return walk_forward_narrow(b, plan ? *plan : narrow_plan(g, c, n_layers, (a_stride == 0 && p0_stride == 0) ? NF_SHARED : 0), x_top4, extra, st);
    for (int l = 0; l < n_layers; ++l) {
        const bool last = (l + 1 == n_layers);
        int rc;
        if ((l == 0 && x0_cols) || (last && x_top4)) {           // compact input and/or compact-only output
            FwdExtra ex_l{};
            if (extra) ex_l = slice_extra(*extra, l == 0, last, false);
            rc = gadapt_launch_fwd_c(c, g, LayerFwd{.x_in = b.x(l), .x_out = (last && x_top4) ? nullptr : b.x(l + 1), .x_top4 = last ? x_top4 : nullptr,
                                                    .a = b.a(l), .p0 = b.p0(l), .lp = b.lp(l), .alpha_out = b.alpha(l), .x_cols = l == 0 ? x0_cols : 0,
                                                    .extra = extra ? &ex_l : nullptr}, st);
        } else {
            rc = gadapt_layer_forward(g, b.x(l), b.x(l + 1), b.a(l), b.p0(l), b.lp(l), b.alpha(l), 0, c, stream);
        }
        if (rc) return rc;
    }
    return GADAPT_OK;
}
extern "C" int gadapt_block_forward(const gadapt_graph* g, float* x_all, int x0_cols, int n_layers, const float* a, int64_t a_stride,
                                    const float* p0, int64_t p0_stride, const float* layer_params, float* alpha_all, float* x_top4,
                                    int c, void* stream) {
    return block_forward(g, x_all, x0_cols, n_layers, a, a_stride, p0, p0_stride, layer_params, alpha_all, x_top4, c, stream, nullptr);
}
extern "C" int gadapt_narrow_route(const gadapt_graph* g, int c) { return g ? gadapt_narrow_takes_c(g, c) : 0; }
extern "C" int gadapt_block_forward_narrow(const gadapt_graph* g, float* x_all, int x0_cols, int n_layers, const float* a, int64_t a_stride,
                                           const float* p0, int64_t p0_stride, const float* layer_params, float* alpha_all, float* x_top4,
                                           int c, void* stream) {
    return block_forward(g, x_all, x0_cols, n_layers, a, a_stride, p0, p0_stride, layer_params, alpha_all, x_top4, c, stream, nullptr, true);
}

// ------------------------------------------------------------------------------------------------
// fused training step (run_GNN.py:99-131 as 13 launches): forward with the node fields as layer-0 input and the loss in the last
// layer's launch; tail = slab sums + chain rule + Adam + the next step's composite coefficients
// ------------------------------------------------------------------------------------------------
extern "C" int gadapt_loss_partials_max(void) { return GADAPT_LOSS_PARTIALS_MAX; }
extern "C" int gadapt_forward_computes_coeffs(const gadapt_graph* g, int c) { return g ? gadapt_forward_computes_coeffs_c(g, c) : 0; }
static int block_forward_loss(const gadapt_graph* g, float* x_all, const float* x_comp, int dim, const float* f_tensor, const float* uu_tensor,
                              int n_layers, float* a, float* p0, const float* param, const float* layer_params, float* alpha_all, float* x_top4,
                              const float* target, int d, int l1, float* seed, float* loss_partials, int c, void* stream, bool narrow,
                              NarrowTop* top = nullptr, int* top_ran = nullptr) {   // top: the backward's buffers; *top_ran: the plan's report
    if (!x_comp || dim < 1 || dim > 4 || dim + (f_tensor ? 1 : 0) + (uu_tensor ? 1 : 0) > 4)
        return fail(GADAPT_E_BADARG, "block_forward_loss: 1..4 coordinates, coordinates + extras <= 4 columns");
    // target == NULL: no loss - the evaluation forward on the node fields (inference.GraphedForward issues it as this one call)
    if (!x_top4 || (target && (!seed || !loss_partials || d < 1 || d > 4))) return fail(GADAPT_E_BADARG, "block_forward_loss: head rows; with a target: seed, partials, 1 <= d <= 4");
    if (!g || g->n_nodes <= 0) return fail(GADAPT_E_BADARG, "bad graph");
    int n_partials = 0;
    // x_all slot 0 starts with the compact [N,4] layer-0 input (written by the layer-0 launch for the layer-0 backward)
    if (param && !gadapt_forward_computes_coeffs_c(g, c))
        return fail(GADAPT_E_BADARG, "block_forward_loss: param given, but this graph / hidden size does not compute the coefficients in its layer-0 launch (gadapt_forward_computes_coeffs)");
    gadapt_narrow_plan plan{};
    if (narrow) {
        const gadapt_narrow_facts f = narrow_facts(g, c, n_layers, NF_SHARED | (target ? NF_TARGET : 0) | (param ? NF_COEFFS : 0) |
                                                                   ((top && top->dxd && top->edge_out && top->slab) ? NF_BUFFERS : 0));
        const gadapt_narrow_switches s = narrow_switches();
        plan = gadapt_narrow_plan_of(&f, &s);
        if (top) top->slab_rows = f.slab_rows;
    }
    // narrow route: the layer-0 launch leaves one row of A / p0 per workgroup 0..63, so a batch of fewer workgroups than that gets its
    // coefficients from the coefficient launch first (the same arithmetic: coeffs_fwd_body) and the layers take them as given
    if (plan.coeffs_first) {
        if (!a || !p0) return fail(GADAPT_E_BADARG, "block_forward_loss (narrow): param given without the coefficient buffers");
        const BucketAt at = bucket_at(c);
        if (int rc = gadapt_coeffs_forward(param, param + at.bq, param + at.wk, a, p0, c, stream)) return rc;
        param = nullptr;
    }
    FwdExtra ex{FieldSrc{x_comp, f_tensor, uu_tensor, dim}, x_all,
                LossArgs{target, seed, loss_partials, d, l1 ? 1 : 0, 1.0f / (float)((int64_t)g->n_nodes * (d > 0 ? d : 1))}, &n_partials, param, a, p0};
    if (plan.top_in_fwd) ex.top = top;                           // the top layer's target pass in the last forward launch
    if (int rc = block_forward(g, x_all, 4, n_layers, a, 0, p0, 0, layer_params, alpha_all, x_top4, c, stream, &ex, narrow, &plan)) return rc;
    if (top_ran) *top_ran = plan.top_in_fwd;
    if (!target) return 0;
    if (n_partials <= 0 || n_partials > GADAPT_LOSS_PARTIALS_MAX) return fail(GADAPT_E_RUNTIME, "block_forward_loss: loss partial count out of range");
    return n_partials;
}
extern "C" int gadapt_block_forward_loss(const gadapt_graph* g, float* x_all, const float* x_comp, int dim, const float* f_tensor, const float* uu_tensor,
                                         int n_layers, float* a, float* p0, const float* param, const float* layer_params, float* alpha_all, float* x_top4,
                                         const float* target, int d, int l1, float* seed, float* loss_partials, int c, void* stream) {
    return block_forward_loss(g, x_all, x_comp, dim, f_tensor, uu_tensor, n_layers, a, p0, param, layer_params, alpha_all, x_top4, target, d, l1,
                              seed, loss_partials, c, stream, false);
}
extern "C" int gadapt_block_forward_loss_narrow(const gadapt_graph* g, float* x_all, const float* x_comp, int dim, const float* f_tensor,
                                                const float* uu_tensor, int n_layers, float* a, float* p0, const float* param, const float* layer_params,
                                                float* alpha_all, float* x_top4, const float* target, int d, int l1, float* seed, float* loss_partials,
                                                int c, void* stream) {
    return block_forward_loss(g, x_all, x_comp, dim, f_tensor, uu_tensor, n_layers, a, p0, param, layer_params, alpha_all, x_top4, target, d, l1,
                              seed, loss_partials, c, stream, true);
}
// gadapt_block_forward_loss_narrow given the backward's buffers: where the plan says so (top_in_fwd) its last forward launch also runs
// the top layer's backward target pass - dxd_ws, the pairs in edge_ws and every row of the packed slab as T_{L-1} of
// gadapt_block_backward_narrow_packed leaves them - and *top_ran = 1: the backward then starts below it (top_done).  Otherwise the
// launches of gadapt_block_forward_loss_narrow and *top_ran = 0.
extern "C" int gadapt_block_forward_loss_narrow_top(const gadapt_graph* g, float* x_all, const float* x_comp, int dim, const float* f_tensor,
                                                    const float* uu_tensor, int n_layers, float* a, float* p0, const float* param, const float* layer_params,
                                                    float* alpha_all, float* x_top4, const float* target, int d, int l1, float* seed, float* loss_partials,
                                                    float* dxd_ws, float* edge_ws, float* slab, int* top_ran, int c, void* stream) {
    if (!top_ran) return fail(GADAPT_E_BADARG, "block_forward_loss_narrow_top: nowhere to report whether the top target pass ran");
    *top_ran = 0;
    NarrowTop top{dxd_ws, edge_ws, slab, 0};
    return block_forward_loss(g, x_all, x_comp, dim, f_tensor, uu_tensor, n_layers, a, p0, param, layer_params, alpha_all, x_top4, target, d, l1,
                              seed, loss_partials, c, stream, true, &top, top_ran);
}

extern "C" int gadapt_step_tail(const float* slab, int n_rows, float* scratch, float* param, float* grad, float* exp_avg, float* exp_avg_sq,
                                float lr, float beta1, float beta2, float eps, float weight_decay, int32_t* state, float grad_scale,
                                float* a_out, float* p0_out, const float* loss_partials, int n_loss_partials, float* loss_out, int64_t loss_count,
                                int c, void* stream) {
    const bool gradient_only = slab && !exp_avg && !exp_avg_sq;     // data parallel, first half: stop at the flat gradient
    if (!param || !grad || !gadapt_supported_hidden_dim(c) || (!gradient_only && (!state || !exp_avg || !exp_avg_sq || (!a_out != !p0_out))))
        return fail(GADAPT_E_BADARG, "step_tail: bad argument");
    if (slab && (n_rows <= 0 || !scratch)) return fail(GADAPT_E_BADARG, "step_tail: slab without row count / scratch");
    if (loss_partials && (n_loss_partials <= 0 || !loss_out || loss_count <= 0 || !slab))
        return fail(GADAPT_E_BADARG, "step_tail: loss partials need a count, a destination and the slab launch they ride in");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int row_len = c * c + c;
    const BucketAt at = bucket_at(c);
    if (slab) {
        const int nbx = (row_len + 255) / 256;
        // (+ one workgroup: the step count for the Adam launch of this step, and the loss value)
        hipLaunchKernelGGL(slab_reduce1_kernel, dim3(nbx + 1, GADAPT_SLAB_CHUNKS), dim3(256), 0, st, slab, scratch, n_rows, row_len,
                           nbx, (const float*)nullptr, 0, 0, (float*)nullptr, loss_partials, n_loss_partials, loss_partials ? 1.0f / (float)loss_count : 0.f, loss_out,
                           gradient_only ? nullptr : state);     // (data parallel: the count advances with the Adam half)
    } else {
        hipLaunchKernelGGL(step_count_kernel, dim3(1), dim3(64), 0, st, state);
    }
    if (gradient_only) {                                            // second-level sums + chain rule, as gadapt_slab_reduce_coeffs_backward
        launch_reduce2_coeffs_bwd(c, scratch, param, param + at.bq, param + at.wk, grad, grad + at.bq, grad + at.wk, grad + at.bk, st);
        return check_launch("step_tail (gradient)");
    }
    TailArgs p{slab ? scratch : nullptr, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, grad_scale, state};
    GADAPT_FOR_C(c, constexpr int lds = tail_lds_floats<CC>() * 4; allow_lds(step_tail_kernel<CC>, lds);
                 hipLaunchKernelGGL(step_tail_kernel<CC>, dim3(tail_blocks<CC>()), dim3(1024), lds, st, p));
    if (int rc = check_launch("step_tail")) return rc;
    // the composite coefficients of the UPDATED weights for the next step's forward - unless that forward computes them itself
    // (a_out = p0_out = NULL: gadapt_forward_computes_coeffs)
    if (!a_out) return GADAPT_OK;
    return gadapt_coeffs_forward(param, param + at.bq, param + at.wk, a_out, p0_out, c, stream);
}

// The narrow route's tail over the PACKED slab (gadapt_block_backward_narrow_packed) as ONE launch, hidden 64: step_tail_narrow_kernel.
// The forms of gadapt_step_tail that read a slab - the whole tail, and (no moments) the flat gradient only; bit-identical to them on
// the equivalent full-width slab (tests/test_gpu_narrow_tail.py).  The gradient-given form has no slab: gadapt_step_tail.
extern "C" int gadapt_step_tail_narrow(const float* slab, int n_rows, float* scratch, float* param, float* grad, float* exp_avg, float* exp_avg_sq,
                                       float lr, float beta1, float beta2, float eps, float weight_decay, int32_t* state, float grad_scale,
                                       float* a_out, float* p0_out, const float* loss_partials, int n_loss_partials, float* loss_out,
                                       int64_t loss_count, int c, void* stream) {
    const bool gradient_only = !exp_avg && !exp_avg_sq;             // data parallel, first half: stop at the flat gradient
    if (c != 64) return fail(GADAPT_E_BADARG, "step_tail_narrow: hidden 64 only (gadapt_narrow_route)");
    if (!slab || n_rows <= 0 || !scratch) return fail(GADAPT_E_BADARG, "step_tail_narrow: the packed slab, its row count and the scratch");
    if (!param || !grad || (!gradient_only && (!state || !exp_avg || !exp_avg_sq || (!a_out != !p0_out))))
        return fail(GADAPT_E_BADARG, "step_tail_narrow: bad argument");
    if (loss_partials && (n_loss_partials <= 0 || !loss_out || loss_count <= 0))
        return fail(GADAPT_E_BADARG, "step_tail_narrow: loss partials need a count and a destination");
    hipStream_t st = static_cast<hipStream_t>(stream);
    TailNarrowArgs p{slab, n_rows, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, grad_scale, gradient_only ? nullptr : state,
                     loss_partials, n_loss_partials, loss_partials ? 1.0f / (float)loss_count : 0.f, loss_out};
    if (env_switch(SW_NARROW_TAIL_SPREAD) == 1)                   // (bit-identical either way: tests/test_gpu_narrow_tail_spread.py)
        hipLaunchKernelGGL((step_tail_narrow_spread_kernel<GADAPT_NARROW_TAIL_THREADS, GADAPT_NARROW_TAIL_ROWS>),
                           dim3(gadapt_narrow_tail_grid(loss_partials != nullptr)), dim3(GADAPT_NARROW_TAIL_THREADS), 0, st, p);
    else
        hipLaunchKernelGGL(step_tail_narrow_kernel, dim3(loss_partials ? 2 : 1), dim3(1024), 0, st, p);
    if (int rc = check_launch("step_tail_narrow")) return rc;
    if (gradient_only || !a_out) return GADAPT_OK;
    const BucketAt at = bucket_at(c);
    return gadapt_coeffs_forward(param, param + at.bq, param + at.wk, a_out, p0_out, c, stream);
}

extern "C" int gadapt_block_backward(const gadapt_graph* g, const float* x_all, int x0_cols, const float* alpha_all, const float* g_top, int g_top_cols, int n_layers,
                                     const float* a, int64_t a_stride, const float* p0, int64_t p0_stride, const float* layer_params,
                                     float* g_ws, float* dxd_ws, float* edge_ws, float* slab, float* d_layer_params, int want_d_scale, float* d_x0,
                                     int c, void* stream) {
    if (int rc = check_graph(g, c)) return rc;
    if (!x_all || !alpha_all || !g_top || n_layers <= 0 || !a || !p0 || !layer_params || !g_ws || !dxd_ws || !edge_ws || !slab)
        return fail(GADAPT_E_BADARG, "block_backward: bad argument");
    if (x0_cols != 0 && (x0_cols != 4 || n_layers < 2 || c < 8 || d_x0))
        return fail(GADAPT_E_BADARG, "block_backward: compact x0 needs 4 columns, >= 2 layers, hidden >= 8, no d_x0");
    const int64_t slab_floats = gadapt_backward_slab_floats(g->n_nodes, c);
    if (slab_floats < 0) return (int)slab_floats;
    const int slab_rows = gadapt_backward_slab_rows(g->n_nodes, c);
    // (x_all and alpha_all: read only)
    const Block b{.g = g, .c = c, .n_layers = n_layers, .x_all = const_cast<float*>(x_all), .nc = (size_t)g->n_nodes * c, .a_all = a, .a_stride = a_stride,
                  .p0_all = p0, .p0_stride = p0_stride, .layer_params = layer_params, .alpha_all = const_cast<float*>(alpha_all), .slab_all = slab,
                  .slab_floats = slab_floats, .shared = (a_stride == 0), .g_ws = g_ws};
    const hipStream_t st = static_cast<hipStream_t>(stream);
    // Layer 1 above a compact layer 0: that layer's backward contracts over the four live columns of its input, so all it
    // reads of this layer's g_out are columns 0..3 - this layer runs the 4-column pair (dxd and g_out as [N,4]).
    // (not for a two-layer block with learnable steps / temperature: layer 1 is then also the top layer, and the SUMS + GC + D4
    // instantiation spills at hidden 32 - that corner keeps the dense pair)
    const bool pair4 = x0_cols && c >= 8 && n_layers >= 2 && !(n_layers == 2 && g_top_cols > 0 && d_layer_params);
    const float* g_cur = g_top;
    for (int l = n_layers - 1; l >= 0; --l) {
        float* g_next = (l == 0) ? d_x0 : b.g_buf(l);
        if (!g->tpos_s || (g_next && (!g->rowptr_s || !g->col_s))) return fail(GADAPT_E_BADARG, "block_backward: source CSR missing");
        const int out4 = (pair4 && l == 1) ? 1 : 0;
        // dense layers that hand their result to the next layer of the block: dxd lives in the g_out buffer (see bwd_inplace_enabled)
        const bool inplace = bwd_inplace_enabled() && l > 0 && g_next && !out4;
        const LayerBwd lb{
            .x_in = b.x(l), .g_in = g_cur, .alpha = b.alpha(l), .a = b.a(l), .p0 = b.p0(l), .lp = b.lp(l), .edge_ws = edge_ws,
            .dxd = inplace ? g_next : dxd_ws, .slab = b.slab(l), .accumulate = (b.shared && l != n_layers - 1) ? 1 : 0,
            // per-workgroup partials [2][L][G] (G = gadapt_backward_slab_rows: the grid of every target-pass launch), d dt block first
            .sums_out = d_layer_params ? d_layer_params + (size_t)l * slab_rows : nullptr,
            .sums_sc_out = (d_layer_params && want_d_scale) ? d_layer_params + ((size_t)n_layers + l) * slab_rows : nullptr,
            .g_out = g_next,
            // compact upstream gradient [N,g_top_cols] (top layer) / compact layer-0 input [N,4] (no d x0: checked by the target launch)
            .g_cols = (l == n_layers - 1) ? g_top_cols : 0, .x_cols = (l == 0) ? x0_cols : 0, .out4 = out4,
            .g_stride = (pair4 && l == 0) ? 4 : 0, .sums_partials = 1};
        if (int rc = launch_bwd(c, g, lb, st)) return rc;
        g_cur = g_next;
    }
    return GADAPT_OK;
}

// Backward of the narrow route (gadapt_block_forward_narrow): every slot of x_all holds [N,4] rows at its start, g_top is the compact
// [N,g_top_cols] top gradient.  The launches are the plan's backward (gadapt_narrow_plan.h; DESIGN.md "How a message-passing entry point
// is put together"): pairs T_{L-1}, S_{L-1}, .., S_1, T_0; fused T_{L-1}, [S_{L-1}+T_{L-2}], .., [S_1+T_0]; or T_{L-1} and the fused
// stages in groups of up to three per launch - without T_{L-1} where the forward call ran it (top_done).  Every per-layer address is
// Block's, every work buffer a member of a pair of the plan's layout.
// packed (gadapt_block_backward_narrow_packed): the slab rows are GADAPT_NARROW_SLAB_ROW = 32 floats - the 20 partials a workgroup owes
// and 12 zeros, one 128-byte line - instead of C*C + C of which 4140 are written zero: every launcher of the route passes the layout on,
// the sums and their order are the same.  One shared conv only (one slab).
static int block_backward_narrow(const gadapt_graph* g, const float* x_all, int x0_cols, const float* alpha_all, const float* g_top,
                                 int g_top_cols, int n_layers, const float* a, int64_t a_stride, const float* p0, int64_t p0_stride,
                                 const float* layer_params, float* g_ws, float* dxd_ws, float* edge_ws, float* slab, float* d_layer_params,
                                 float* d_x0, int c, void* stream, int packed, bool top_done = false, int* block_ran = nullptr) {
    if (int rc = check_graph(g, c)) return rc;
    if (!x_all || !alpha_all || !g_top || n_layers < 2 || !a || !p0 || !layer_params || !g_ws || !dxd_ws || !edge_ws || !slab)
        return fail(GADAPT_E_BADARG, "block_backward (narrow): bad argument");
    if (x0_cols != 4 || g_top_cols < 1 || g_top_cols > 4 || d_x0 || d_layer_params || !gadapt_narrow_takes_c(g, c))
        return fail(GADAPT_E_BADARG, "block_backward (narrow): compact x0, compact top gradient, no d_x0, fixed steps and temperature, "
                                     "hidden 64 on a graph the wide forward takes (gadapt_narrow_route)");
    if (packed && (a_stride != 0 || p0_stride != 0)) return fail(GADAPT_E_BADARG, "block_backward (narrow, packed slab): one shared conv (a_stride = p0_stride = 0)");
    const int64_t slab_floats = gadapt_backward_slab_floats(g->n_nodes, c);
    if (slab_floats < 0) return (int)slab_floats;
    const gadapt_narrow_facts facts = narrow_facts(g, c, n_layers, ((a_stride == 0 && p0_stride == 0) ? NF_SHARED : 0) | (packed ? NF_PACKED : 0) |
                                                                   (top_done ? NF_TOP_DONE : 0) | (block_ran ? NF_MAY_BLOCK : 0));
    const gadapt_narrow_switches sw = narrow_switches();
    const gadapt_narrow_plan plan = gadapt_narrow_plan_of(&facts, &sw);
    // (x_all and alpha_all: read only)
    const Block b{.g = g, .c = c, .n_layers = n_layers, .x_all = const_cast<float*>(x_all), .nc = (size_t)g->n_nodes * c, .a_all = a, .a_stride = a_stride,
                  .p0_all = p0, .p0_stride = p0_stride, .layer_params = layer_params, .alpha_all = const_cast<float*>(alpha_all), .slab_all = slab,
                  .slab_floats = slab_floats, .shared = (a_stride == 0), .g_ws = g_ws};
    const hipStream_t st = static_cast<hipStream_t>(stream);
    // a record's buffers: member k of a pair (gadapt_narrow_layout), -1: none - and as the upstream gradient of a `first` launch, g_top
    auto g_at = [&](int k) { return k < 0 ? nullptr : g_ws + plan.at.g[k]; };
    auto dxd_at = [&](int k) { return k < 0 ? nullptr : dxd_ws + plan.at.dxd[k]; };
    auto edge_at = [&](int k) { return k < 0 ? nullptr : (k == 0 ? edge_ws : dxd_ws) + plan.at.edge[k]; };
    for (int i = 0; i < plan.n_bwd; ++i) {
        const gadapt_narrow_launch r = gadapt_narrow_bwd_launch(&plan, i);
        const int l = r.layer;
        const float* g_in = r.first ? g_top : g_at(r.g_in);
        // layer l of the route as a target pass (writes edge_out, dxd_out) or a source pass (reads edge_in, dxd_in; writes g_out)
        auto layer = [&](int at, bool source) {
            return LayerBwd{.x_in = b.x(at), .g_in = g_in, .alpha = b.alpha(at), .a = b.a(at), .p0 = b.p0(at), .lp = b.lp(at),
                            .edge_ws = edge_at(source ? r.edge_in : r.edge_out), .dxd = dxd_at(source ? r.dxd_in : r.dxd_out), .slab = b.slab(at),
                            .accumulate = r.accumulate, .g_out = source ? g_at(r.g_out) : nullptr, .g_cols = r.first ? g_top_cols : 0, .slab_packed = packed};
        };
        int rc;
        switch (r.kind) {
        case GADAPT_NARROW_L_TARGET: rc = gadapt_launch_bwd_target_narrow_c(c, g, layer(l, false), st); break;
        case GADAPT_NARROW_L_SOURCE: rc = gadapt_launch_bwd_source_narrow_c(c, g, layer(l, true), st); break;
        case GADAPT_NARROW_L_TARGET0: {                          // the [N,4] result of layer 1 into the compact layer-0 launch of the tiled route
            LayerBwd lb = layer(l, false);
            lb.x_cols = 4; lb.g_stride = 4; lb.sums_partials = 1;
            rc = gadapt_launch_bwd_target_c(c, g, lb, st);
        } break;
        case GADAPT_NARROW_L_FUSED: {                            // source pass of layer l + target pass of layer l - 1 (its dxd row: read, then written)
            LayerBwd tgt = layer(l - 1, false);
            tgt.g_in = nullptr; tgt.g_cols = 0; tgt.dxd = dxd_at(r.dxd_in);
            rc = gadapt_launch_bwd_fused_narrow_c(c, g, layer(l, true), tgt, edge_at(r.edge_in), edge_at(r.edge_out), r.last, st);
        } break;
        case GADAPT_NARROW_L_GROUP:
            rc = gadapt_launch_bwd_narrow_block_c(c, g, BwdBlockLaunch{.x_src0 = b.x(l), .slot_stride = (int64_t)b.nc, .alpha0 = b.alpha(l - 1),
                    .alpha_stride = g->n_edges, .lp0 = b.lp(l - 1), .a = b.a(l), .p0 = b.p0(l), .g_in = g_in, .g_cols = r.first ? g_top_cols : 0,
                    .edge_in = edge_at(r.edge_in), .dxd_in = dxd_at(r.dxd_in), .g_out = g_at(r.g_out), .edge_out = edge_at(r.edge_out),
                    .dxd_out = dxd_at(r.dxd_out), .slab = b.slab(l), .slab_rows = facts.slab_rows, .K = r.count, .halo = plan.bwd_halo, .layer0 = r.last}, st);
            break;
        default: rc = fail(GADAPT_E_RUNTIME, "block_backward (narrow): a launch kind the backward does not have");
        }
        if (rc) return rc;
    }
    if (block_ran) *block_ran = plan.block_ran;
    return GADAPT_OK;
}
extern "C" int gadapt_block_backward_narrow(const gadapt_graph* g, const float* x_all, int x0_cols, const float* alpha_all, const float* g_top,
                                            int g_top_cols, int n_layers, const float* a, int64_t a_stride, const float* p0, int64_t p0_stride,
                                            const float* layer_params, float* g_ws, float* dxd_ws, float* edge_ws, float* slab, float* d_layer_params,
                                            int want_d_scale, float* d_x0, int c, void* stream) {
    (void)want_d_scale;
    return block_backward_narrow(g, x_all, x0_cols, alpha_all, g_top, g_top_cols, n_layers, a, a_stride, p0, p0_stride, layer_params, g_ws, dxd_ws,
                                 edge_ws, slab, d_layer_params, d_x0, c, stream, 0);
}
extern "C" int64_t gadapt_narrow_slab_floats(int64_t n_nodes) {
    const int rows = gadapt_backward_slab_rows(n_nodes, 64);
    return rows < 0 ? rows : (int64_t)rows * GADAPT_NARROW_SLAB_ROW;
}
extern "C" int gadapt_block_backward_narrow_packed(const gadapt_graph* g, const float* x_all, int x0_cols, const float* alpha_all, const float* g_top,
                                                   int g_top_cols, int n_layers, const float* a, int64_t a_stride, const float* p0, int64_t p0_stride,
                                                   const float* layer_params, float* g_ws, float* dxd_ws, float* edge_ws, float* slab,
                                                   float* d_layer_params, int want_d_scale, float* d_x0, int c, void* stream) {
    (void)want_d_scale;
    return block_backward_narrow(g, x_all, x0_cols, alpha_all, g_top, g_top_cols, n_layers, a, a_stride, p0, p0_stride, layer_params, g_ws, dxd_ws,
                                 edge_ws, slab, d_layer_params, d_x0, c, stream, 1);
}
// ... behind gadapt_block_forward_loss_narrow_top with *top_ran = 1: the same arguments, the same launches without the first - the top
// layer's target pass ran in the forward launch; the edge buffers alternate as if it had just written edge_ws.
extern "C" int gadapt_block_backward_narrow_packed_below_top(const gadapt_graph* g, const float* x_all, int x0_cols, const float* alpha_all,
                                                             const float* g_top, int g_top_cols, int n_layers, const float* a, int64_t a_stride,
                                                             const float* p0, int64_t p0_stride, const float* layer_params, float* g_ws, float* dxd_ws,
                                                             float* edge_ws, float* slab, float* d_layer_params, int want_d_scale, float* d_x0, int c,
                                                             void* stream) {
    (void)want_d_scale;
    return block_backward_narrow(g, x_all, x0_cols, alpha_all, g_top, g_top_cols, n_layers, a, a_stride, p0, p0_stride, layer_params, g_ws, dxd_ws,
                                 edge_ws, slab, d_layer_params, d_x0, c, stream, 1, true);
}
// gadapt_block_backward_narrow_packed (top_done = 0) or ..._below_top (top_done = 1) with the layers below the top in one launch per
// group of up to three fused stages where the step is eligible (narrow_bwd_block_eligible; *block_ran = 1): the slab carries the same
// bits, the work buffers are written only as include/gadapt_hip.h states.  Not eligible: exactly those entry points' launches, *block_ran = 0.
extern "C" int gadapt_block_backward_narrow_packed_block(const gadapt_graph* g, const float* x_all, int x0_cols, const float* alpha_all,
                                                         const float* g_top, int g_top_cols, int n_layers, const float* a, int64_t a_stride,
                                                         const float* p0, int64_t p0_stride, const float* layer_params, float* g_ws, float* dxd_ws,
                                                         float* edge_ws, float* slab, float* d_layer_params, int want_d_scale, float* d_x0, int c,
                                                         void* stream, int top_done, int* block_ran) {
    (void)want_d_scale;
    if (!block_ran) return fail(GADAPT_E_BADARG, "block_backward_narrow_packed_block: nowhere to report whether the block launch ran");
    *block_ran = 0;
    return block_backward_narrow(g, x_all, x0_cols, alpha_all, g_top, g_top_cols, n_layers, a, a_stride, p0, p0_stride, layer_params, g_ws, dxd_ws,
                                 edge_ws, slab, d_layer_params, d_x0, c, stream, 1, top_done != 0, block_ran);
}
