// gadapt_narrow_fwd.inc - forward of the narrow route (gadapt_block_forward_narrow), included by gadapt_tu_fwd.hip after gadapt_wide.inc:
// wide::fwd_narrow_kernel, one layer per launch (described first), and wide::fwd_narrow_block_kernel, up to four layers per launch by halo
// recompute (at the end of the file; its TOP instantiations also run the top layer's backward target pass, narrow_top_target).  Both run
// the per-node statements of gadapt_narrow_node.inc.
//
// On the narrow route every layer reads and writes [N,4] slots: columns 4.. stay exactly zero behind the zero-pad encoder
// (DESIGN.md section 4), so of the wide kernel's work (wide::fwd_kernel<XC = true>) only channels 0..3 of P, one 16-byte chunk per
// neighbour row and one aggregated chunk carry data.  This kernel does just that part, ONE NODE PER LANE (a wave owns 64 consecutive
// nodes, a 256-thread workgroup steps over 256-node blocks of the batch, grid-stride):
//   round trip 1: the ELL row (8 neighbour indices), the CSR row bounds, the own [N,4] row (layer 0: assembled from the node fields,
//                 Cols4) and, on the last layer, the loss target row;
//   round trip 2: the neighbour rows, 16 bytes each, straight from L2 (no LDS window: the whole [N,4] slot is cache-resident).
// The weights are requested together with round trip 1 and the A fragment is built while round trip 2 is in flight, so a one-step
// workgroup (the headline batch: 512 workgroups) waits for two memory round trips.  No weight fragments in LDS, no window ring, no
// workgroup barrier in the node loop; LDS holds the per-wave alpha staging (and, with cw, the coefficient partial sums).
//
// Bit-identical to wide::fwd_kernel<true, ...> on channels 0..3 (tests/test_gpu_narrow_forward.py compares both with torch.equal):
//  - P[0..3] on the matrix cores with the wide kernel's operands and instruction sequence (mfma6 at ob = 0, ks = 0, accumulators
//    starting at p0).  A 32x32x16 MFMA covers 32 nodes, so a wave runs two groups: group a = lanes 0..31 (B operand: own row in
//    lanes 0..31, zeros at k = 8..15 in lanes 32..63 - exactly the wide kernel's B), group b = lanes 32..63 (their rows moved down
//    by one v_permlane32_swap per column).  Group b's P[0..3] then goes back up with one swap per channel.  Output rows o >= 4 of the
//    MFMA are never read, and an MFMA row depends only on its own A row, so the A fragment carries rows 0..3 and zeros elsewhere.
//  - score, softmax and aggregation in the wide kernel's expression shapes (same contraction into fma); the h = 1 half of its pair
//    sum is an exact +0 (zero columns), added here as such.
//  - the re-base decision is the wide kernel's wave ballot over ONE aligned 32-node group: each half of this wave's ballot mask.
//  - layer 0 with the flat parameter bucket (cw): the coefficients A = Wk^T Wq, p0 = Wk^T bq with coeffs_fwd_body's arithmetic (four
//    interleaved partial sums over r; p0 one chain).  Each workgroup forms only the 64 entries A[0..3][0..15] and p0[0..3] its
//    fragments use, one partial sum per thread; workgroups 0..63 each also form ONE row of the full A / p0 for a_out / p0_out, so
//    no workgroup carries the whole 64 x 64 product.

namespace wide {

constexpr int NRW_NT = 256;                    // threads per workgroup = nodes per workgroup step
constexpr int NRW_AST = 64 * 8;                // alpha staging floats per wave: 64 rows x up to 8 entries

__device__ __forceinline__ void swap32(float& a, float& b) {   // a(lanes 32..63) <-> b(lanes 0..31)
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}

// acc += A x B on the three bf16 pieces of each operand, in mfma6's order
__device__ __forceinline__ void mfma6r(f32x16& acc, const Split3& a, const Split3& b) {
    acc = mfma_bf16(a.h, b.l, acc);                               // small pieces first
    acc = mfma_bf16(a.l, b.h, acc);
    acc = mfma_bf16(a.m, b.m, acc);
    acc = mfma_bf16(a.h, b.m, acc);
    acc = mfma_bf16(a.m, b.h, acc);
    acc = mfma_bf16(a.h, b.h, acc);
}

// round trip 1 of a step: this lane's ELL row, CSR row bounds, own row and (HEAD) loss target row
struct NarrowIn { int4 ea, eb; int rp0, rp1; float4 own, tgt; };

// row `row` of the [N,4] layer input: the matrix (one 16-byte load), or (FLD: layer 0 of a fused step) assembled from the node fields
template <bool FLD> __device__ __forceinline__ float4 ld_x4(const Cols4& cx, const float* __restrict__ x, int row) {
    if constexpr (FLD) return ld_cols4(cx, row);
    else return *reinterpret_cast<const float4*>(x + 4 * (size_t)row);
}
// a loop-invariant scalar made opaque where it is used: hoisted, its comparisons stay live as 64-bit masks (SGPR spills)
__device__ __forceinline__ int opaque(int v) { asm volatile("" : "+s"(v)); return v; }

template <bool HEAD, bool FLD>
__device__ __forceinline__ void narrow_issue1(NarrowIn& t, const FwdArgs& p, const Cols4& cx, const float* tgt_base, int tgt_d, int i) {
    const int N = p.n_nodes, ic = min(i, N - 1);
    t.ea = *reinterpret_cast<const int4*>(p.ell + 8 * (size_t)i);          // ELL rows are padded to a multiple of 256
    t.eb = *reinterpret_cast<const int4*>(p.ell + 8 * (size_t)i + 4);
    t.rp0 = p.rowptr[min(i, N)];
    t.rp1 = p.rowptr[min(i + 1, N)];
    t.own = ld_x4<FLD>(cx, p.x_in, ic);
    t.tgt = f4zero();
    if constexpr (HEAD) t.tgt = loss_target4(tgt_base, opaque(tgt_d), ic);
}
// round trip 2: the neighbour rows k < kmax (unused ELL entries -> own row, as the wide kernel)
template <bool FLD>
__device__ __forceinline__ void narrow_issue2(v4f (&xv)[8], const NarrowIn& t, const FwdArgs& p, const Cols4& cx, int i) {
    const int ic = min(i, p.n_nodes - 1), kmax = opaque(p.kmax);
    const int jn[8] = {t.ea.x, t.ea.y, t.ea.z, t.ea.w, t.eb.x, t.eb.y, t.eb.z, t.eb.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k < kmax) {
            const float4 v = ld_x4<FLD>(cx, p.x_in, jn[k] < 0 ? ic : jn[k]);
            xv[k] = v4f{v.x, v.y, v.z, v.w};
        }
    }
}

// HEAD: last layer of a fused step with a loss (loss seed and one partial per wave).  FLD: the layer input comes from the node fields
// (p.fs), else from the [N,4] matrix p.x_in.  x_out is not written: the result rows go to x_top4.  The launcher keeps the grid at most
// n_steps (every workgroup has a first step) and, with cw, at least 64 (one row of A per workgroup 0..63).
template <bool HEAD, bool FLD>
__global__ __launch_bounds__(NRW_NT) void fwd_narrow_kernel(FwdArgs p) {
    __shared__ float astage[4][NRW_AST];
    __shared__ float cpart[4][64];                               // cw: partial sums of A[o][cc], o < 4, cc < 16 (index 16 o + cc) ...
    __shared__ float rpart[4][64];                               // ... and of the row of A this workgroup writes to a_out
    __shared__ float cst[64][6];                                 // cw: Wk[r][0..3], bq[r], Wk[r][row]
    __shared__ float p0s[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
    const float dt = p.lp[0], sc = p.lp[1];
    const int N = p.n_nodes;
    const Cols4 cx = make_cols4(p.x_in, p.fs);                   // FLD: where the layer-0 rows come from
    const float* tgt_base = (HEAD && p.loss.target) ? p.loss.target : p.x_in;
    const int tgt_d = (HEAD && p.loss.target) ? p.loss.d : 1;
    const int row = blockIdx.x;                                  // cw: the row of A / p0 this workgroup writes (row < 64)

    // ---- requests first: the weights this launch needs, then round trip 1 of the first step; round trip 2 is issued as soon as the
    // indices are in, and the A fragment is built while the neighbour rows are in flight
    float kv[16], wv[16], kr[16], wr[16];
    float4 k4 = f4zero(), a0 = f4zero(), a1 = f4zero();
    float bqv = 0.f, wkr = 0.f;
    float pv[4];
    const float* gwq = p.cw; const float* gbq = p.cw + C * C; const float* gwk = gbq + C;
    if (p.cw) {
        // thread t: the partial sum over r = t / 64 (mod 4) of A[o][cc], (o, cc) = (lane / 16, lane % 16) ...
#pragma unroll
        for (int q = 0; q < 16; ++q) { kv[q] = gwk[(4 * q + wave) * C + (lane >> 4)]; wv[q] = gwq[(4 * q + wave) * C + (lane & 15)]; }
        if (row < C) {                                           // ... and of A[row][lane]
#pragma unroll
            for (int q = 0; q < 16; ++q) { kr[q] = gwk[(4 * q + wave) * C + row]; wr[q] = gwq[(4 * q + wave) * C + lane]; }
        }
        if (wave == 0) { k4 = *reinterpret_cast<const float4*>(gwk + lane * C); bqv = gbq[lane]; }
        if (wave == 1 && row < C) { wkr = gwk[lane * C + row]; bqv = gbq[lane]; }
    } else {
        const int o = min(lane & 31, 3);
        a0 = *reinterpret_cast<const float4*>(p.A + o * C + 8 * h);
        a1 = *reinterpret_cast<const float4*>(p.A + o * C + 8 * h + 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) pv[r] = p.p0[r];
    }
    int s = blockIdx.x;
    NarrowIn t1;
    narrow_issue1<HEAD, FLD>(t1, p, cx, tgt_base, tgt_d, s * NRW_NT + 64 * wave + lane);
    v4f xv[8];
    narrow_issue2<FLD>(xv, t1, p, cx, s * NRW_NT + 64 * wave + lane);

    // ---- A fragment (lane (o, h): A[o][8 h .. 8 h + 7], rows o >= 4 zero) and p0[0..3]
    float fa[8];
    if (p.cw) {
        // coeffs_fwd_body's arithmetic: four interleaved partial sums over r of fmaf(Wk[r][o], Wq[r][cc], .), p0 one chain over r
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) v = fmaf(kv[q], wv[q], v);
        cpart[wave][lane] = v;
        if (row < C) {
            float vr = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) vr = fmaf(kr[q], wr[q], vr);
            rpart[wave][lane] = vr;
        }
        if (wave == 0) {                                         // p0[o], o < 4: lanes 0..3
            cst[lane][0] = k4.x; cst[lane][1] = k4.y; cst[lane][2] = k4.z; cst[lane][3] = k4.w; cst[lane][4] = bqv;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // same wave: LDS operations complete in order
            if (lane < 4) {
                float p0v = 0.f;
#pragma unroll 8
                for (int r = 0; r < C; ++r) p0v = fmaf(cst[r][lane], cst[r][4], p0v);
                p0s[lane] = p0v;
            }
        }
        if (wave == 1 && row < C) {                              // p0[row] for p0_out: lane 0
            cst[lane][5] = wkr; cst[lane][4] = bqv;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) {
                float p0v = 0.f;
#pragma unroll 8
                for (int r = 0; r < C; ++r) p0v = fmaf(cst[r][5], cst[r][4], p0v);
                p.p0_out[row] = p0v;
            }
        }
        __syncthreads();
        const int o = lane & 31;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int L = 16 * min(o, 3) + 8 * h + e;
            const float av = (cpart[0][L] + cpart[1][L]) + (cpart[2][L] + cpart[3][L]);
            fa[e] = o < 4 ? av : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) pv[r] = p0s[r];
        if (row < C && tid < C) p.a_out[row * C + tid] = (rpart[0][tid] + rpart[1][tid]) + (rpart[2][tid] + rpart[3][tid]);
    } else {
        const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) fa[e] = (lane & 31) < 4 ? av[e] : 0.f;
    }
    const Split3 af = split8(fa);

    float loss_lv = 0.f;                                         // fused loss: this lane's terms
    float* sa = astage[wave];
#pragma unroll 1
    for (;;) {
        const int i = s * NRW_NT + 64 * wave + lane;             // this lane's node

#include "gadapt_narrow_node.inc"                                 // own, xc, deg, lo | hi, w[0..7] of node i

        if (i < N) {
            *reinterpret_cast<v4f*>(p.x_top4 + 4 * (size_t)i) = v4f{lo.x, lo.y, hi.x, hi.y};
            if (p.x0c) *reinterpret_cast<v4f*>(p.x0c + 4 * (size_t)i) = xc;   // the layer-0 input rows, for the layer-0 backward
            if constexpr (HEAD) {
                if (p.loss.target) {
                    LossArgs la = p.loss;
                    la.d = opaque(tgt_d);                        // (= p.loss.d where there is a target)
                    loss_lv = loss_node(la, i, make_float4(lo.x, lo.y, hi.x, hi.y), t1.tgt, loss_lv);
                }
            }
        }
        // ---- alpha in CSR order: staged per wave, then coalesced stores
        if (p.alpha_out) {
            const int e_first = __builtin_amdgcn_readfirstlane(t1.rp0), e_cnt = __builtin_amdgcn_readlane(t1.rp1, 63) - e_first;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k < deg) sa[t1.rp0 - e_first + k] = w[k];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // same wave: LDS operations complete in order
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (64 * t + lane < e_cnt) p.alpha_out[e_first + 64 * t + lane] = sa[64 * t + lane];
        }
        s += gridDim.x;                                          // (one step per workgroup up to 1024 steps: N <= 262 144)
        if (s >= p.n_steps) break;
        narrow_issue1<HEAD, FLD>(t1, p, cx, tgt_base, tgt_d, s * NRW_NT + 64 * wave + lane);
        narrow_issue2<FLD>(xv, t1, p, cx, s * NRW_NT + 64 * wave + lane);
    }
    if constexpr (HEAD) { if (p.loss.target) loss_wave_partial<4>(p.loss, loss_lv, tid); }   // every wave of the grid owns a slot
}

// The weights of a block launch: fwd_narrow_kernel's prologue on an eight-wave workgroup.  Given coefficients: this lane's A fragment
// rows and p0[0..3].  cw (layer 0 with the flat parameter bucket): A = Wk^T Wq, p0 = Wk^T bq with coeffs_fwd_body's arithmetic - waves
// 0..3 each carry one of the four interleaved partial sums over r, one entry per thread, waves 4..7 only take the results; workgroup
// `row` < 64 also forms row `row` of the full A / p0 for a_out / p0_out.  narrow_w_issue requests them, narrow_w_finish (one workgroup
// barrier with cw) gives the fragment fa and p0[0..3] in t.pv; the caller puts its own first loads between the two.
// (A copy of that prologue with the wave guard, not a shared function: fwd_narrow_kernel keeps its text, and with it its instruction stream.)
struct NarrowW { float kv[16], wv[16], kr[16], wr[16]; float4 k4, a0, a1; float bqv, wkr; float pv[4]; };
struct NarrowWLds {
    float cpart[4][64];                                          // partial sums of A[o][cc], o < 4, cc < 16 (index 16 o + cc) ...
    float rpart[4][64];                                          // ... and of the row of A this workgroup writes to a_out
    float cst[64][6];                                            // Wk[r][0..3], bq[r], Wk[r][row]
    float p0s[4];
};
__device__ __forceinline__ void narrow_w_issue(NarrowW& t, const FwdArgs& p, int row, int wave, int lane) {
    const int h = lane >> 5;
    t.k4 = f4zero(); t.a0 = f4zero(); t.a1 = f4zero();
    t.bqv = 0.f; t.wkr = 0.f;
    const float* gwq = p.cw; const float* gbq = p.cw + C * C; const float* gwk = gbq + C;
    if (p.cw) {
        const bool part = wave < 4;
        // thread t: the partial sum over r = t / 64 (mod 4) of A[o][cc], (o, cc) = (lane / 16, lane % 16) ...
        if (part) {
#pragma unroll
            for (int q = 0; q < 16; ++q) { t.kv[q] = gwk[(4 * q + wave) * C + (lane >> 4)]; t.wv[q] = gwq[(4 * q + wave) * C + (lane & 15)]; }
        }
        if (part && row < C) {                                           // ... and of A[row][lane]
#pragma unroll
            for (int q = 0; q < 16; ++q) { t.kr[q] = gwk[(4 * q + wave) * C + row]; t.wr[q] = gwq[(4 * q + wave) * C + lane]; }
        }
        if (wave == 0) { t.k4 = *reinterpret_cast<const float4*>(gwk + lane * C); t.bqv = gbq[lane]; }
        if (wave == 1 && row < C) { t.wkr = gwk[lane * C + row]; t.bqv = gbq[lane]; }
    } else {
        const int o = min(lane & 31, 3);
        t.a0 = *reinterpret_cast<const float4*>(p.A + o * C + 8 * h);
        t.a1 = *reinterpret_cast<const float4*>(p.A + o * C + 8 * h + 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) t.pv[r] = p.p0[r];
    }
}
__device__ __forceinline__ void narrow_w_finish(float (&fa)[8], NarrowW& t, NarrowWLds& ws, const FwdArgs& p, int row, int tid) {
    const int lane = tid & 63, wave = tid >> 6, h = lane >> 5;
    if (p.cw) {
        // coeffs_fwd_body's arithmetic: four interleaved partial sums over r of fmaf(Wk[r][o], Wq[r][cc], .), p0 one chain over r
        const bool part = wave < 4;
        if (part) {
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) v = fmaf(t.kv[q], t.wv[q], v);
            ws.cpart[wave][lane] = v;
        }
        if (part && row < C) {
            float vr = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) vr = fmaf(t.kr[q], t.wr[q], vr);
            ws.rpart[wave][lane] = vr;
        }
        if (wave == 0) {                                         // p0[o], o < 4: lanes 0..3
            ws.cst[lane][0] = t.k4.x; ws.cst[lane][1] = t.k4.y; ws.cst[lane][2] = t.k4.z; ws.cst[lane][3] = t.k4.w; ws.cst[lane][4] = t.bqv;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // same wave: LDS operations complete in order
            if (lane < 4) {
                float p0v = 0.f;
#pragma unroll 8
                for (int r = 0; r < C; ++r) p0v = fmaf(ws.cst[r][lane], ws.cst[r][4], p0v);
                ws.p0s[lane] = p0v;
            }
        }
        if (wave == 1 && row < C) {                              // p0[row] for p0_out: lane 0
            ws.cst[lane][5] = t.wkr; ws.cst[lane][4] = t.bqv;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) {
                float p0v = 0.f;
#pragma unroll 8
                for (int r = 0; r < C; ++r) p0v = fmaf(ws.cst[r][5], ws.cst[r][4], p0v);
                p.p0_out[row] = p0v;
            }
        }
        __syncthreads();
        const int o = lane & 31;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int L = 16 * min(o, 3) + 8 * h + e;
            const float av = (ws.cpart[0][L] + ws.cpart[1][L]) + (ws.cpart[2][L] + ws.cpart[3][L]);
            fa[e] = o < 4 ? av : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) t.pv[r] = ws.p0s[r];
        if (row < C && tid < C) p.a_out[row * C + tid] = (ws.rpart[0][tid] + ws.rpart[1][tid]) + (ws.rpart[2][tid] + ws.rpart[3][tid]);
    } else {
        const float av[8] = {t.a0.x, t.a0.y, t.a0.z, t.a0.w, t.a1.x, t.a1.y, t.a1.z, t.a1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) fa[e] = (lane & 31) < 4 ? av[e] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------
// K <= 4 consecutive layers in ONE launch by halo recompute (gadapt_block_plan.h).  A workgroup of eight waves owns
// GADAPT_NARROW_TILE = 512 consecutive nodes.  Layer k + 1 of node i needs layer k of i's in-neighbours, all within `halo` nodes of i's
// aligned 32-node group (gadapt_narrow_block_halo_host), so the workgroup computes layer k on its owned range widened by
// (K - 1 - k) halo on each side, for itself: no workgroup waits for another, the only barriers are workgroup barriers.
//   one global round trip: the input rows of the frame (layer 0 of a fused step: from the node fields) into LDS, the ELL rows and CSR
//   row bounds of this lane's two nodes into registers, the loss target row, the weights;
//   per layer: own row and neighbour rows from LDS (16-byte rows, consecutive lanes read consecutive own rows), the per-node
//   statements of fwd_narrow_kernel (gadapt_narrow_node.inc), the new row into the other LDS buffer, one workgroup barrier.
// Frame: row r holds node frame0 + r, frame0 = 512 t - margin, margin = K halo rounded up to 64.  Thread `tid` owns frame rows tid and
// tid + 512 at every layer (wave w: the 64-node blocks w and w + 8), so the indices stay in registers and exactly one of a wave's two
// blocks is owned, whole.  A block runs a layer when one of its halves lies in that layer's range; each half is one aligned 32-node
// group, the groups fwd_narrow_kernel ballots over, so every stored value is bit-identical with the per-layer launches.  Rows outside
// a layer's range are computed on stale rows and dropped: nothing in a later range reads them.
// Only owned nodes store to global memory: the [N,4] rows of every layer, alpha, the layer-0 input rows, the loss seed; one loss
// partial per wave (8 per workgroup).
// TOP (with HEAD and a loss target; gadapt_block_forward_loss_narrow_top): the launch also runs the top layer's backward target pass -
// the first launch of the narrow backward, grand_bwd_target_narrow_kernel with accumulate = 0, which needs nothing from another workgroup.
// The lane that owns node i has, after the last layer, all that pass reads: the seed row it has just computed, the layer's input row,
// neighbour rows and alpha, {dt, scale}, the 4 x 4 corner of A (given, or this launch's own sums); it requests the positions of its edges
// in source order at the top of the last layer, runs narrow_top_target and stores dxd[i] and its {alpha dt, ds} pairs.  The 20 slab
// partials go through the standalone kernel's wave butterfly and, per owned 64-node block, through LDS; after one more workgroup barrier
// the tile writes packed slab rows 2 t and 2 t + 1 as (b0 + b1) + (b2 + b3) over their blocks in node order, and zeros to its share of
// the rows past the last tile's (gadapt_block_slab_plan) - every row of the slab is written, each by one tile, with the bits the
// standalone launch writes.  The launcher takes this form only where a lane of that launch has at most one node (N <= 256 rows).
struct BlockArgs {
    FwdArgs f;                  // x_in: the group's input rows; x_top4, lp, alpha_out: output rows, {dt, scale} and alpha of its FIRST layer
    int K, halo;
    long long slot_stride, alpha_stride;    // floats from one layer's output rows / alpha to the next layer's
    float* x_last;              // nullable: the group's last layer stores its rows here instead (the head rows)
    // TOP instantiations only (behind the fields every instantiation reads): the top layer's backward target pass
    const int32_t* tpos; float2* edge_out; float* dxd; float* slab;   // gadapt_graph::tpos_s, the pairs' buffer, dxd [N,4], packed slab rows
    int slab_rows, n_edges;
};
constexpr int NRB_NT = GADAPT_NARROW_TILE;     // threads per workgroup = nodes a workgroup owns
constexpr int NRB_ROWS = 2 * NRB_NT;           // frame rows: 512 + 2 margin <= 1024

// TOP: this node's terms of the loss as loss_node (same expressions), which also hands the seed row back - zero beyond L.d columns, as
// ld_row4_compact reads it - for the target pass that follows in the same lane
__device__ __forceinline__ float loss_node_seed(const LossArgs& L, int row, const float4& pred, const float4& tgt, float lv, float4& seed) {
    const float pv[4] = {pred.x, pred.y, pred.z, pred.w}, tv[4] = {tgt.x, tgt.y, tgt.z, tgt.w};
    float sv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < L.d) {
            const float diff = pv[k] - tv[k];
            if (L.l1) { lv += fabsf(diff); sv[k] = (diff > 0.f ? L.inv : (diff < 0.f ? -L.inv : 0.f)); }
            else      { lv = fmaf(diff, diff, lv); sv[k] = 2.0f * diff * L.inv; }
            L.seed[(size_t)row * L.d + k] = sv[k];
        }
    }
    seed = make_float4(sv[0], sv[1], sv[2], sv[3]);
    return lv;
}

// TOP: the target pass of the top layer for ONE node, in the lane that has just run its forward - the NARROW, SUMS = 0, deg <= 8
// branch of bwd_target_compact_body (gadapt_bwd_target.inc) on operands the forward still holds: g4 = the seed row, xi = the layer's
// input row, xn[k] / al[k] = the neighbour rows and alpha of the edge walk, a4 = A[o][c] (o, c < 4).  Same expressions in the same
// order, fmaf where that body calls fmaf and nowhere else (no contraction: that kernel's instruction stream has none either), so every
// value stored carries the bits grand_bwd_target_narrow_kernel stores.  Entries k >= deg: weight 0 on a zero difference (that kernel
// multiplies its zero weight with the difference to some valid row; either way the terms are zeros that leave every sum as it is).
// live = the lane owns a node of the batch: only then it stores, and only then part[] (dA[o][c] at 4 o + c, dp0[o] at 16 + o) is its
// node's share of the slab row - else zeros, as for a lane of that kernel whose node loop runs no iteration.
// (A copy of those statements, not a shared function: the standalone kernels keep their text, and with it their instruction streams.)
__device__ __forceinline__ void narrow_top_target(float (&part)[20], const float4& g4, const float4& xi, const v4f (&xn)[8], const float (&al)[8],
                                                  int deg, float dt, float sc, const float (&a4)[4][4], const int (&tp)[8], bool live, int i,
                                                  float2* __restrict__ edge_out, float* __restrict__ dxd) {
#pragma clang fp contract(off)
    const float w1 = 1.0f - dt;
    const float4 dm = make_float4(dt * g4.x, dt * g4.y, dt * g4.z, dt * g4.w);
    float D = 0.f;
    float4 dP = f4zero();
    float ak[8], da[8];
    float4 xk[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const bool on = k < deg;
        ak[k] = on ? al[k] : 0.f;
        xk[k] = on ? make_float4(xn[k].x - xi.x, xn[k].y - xi.y, xn[k].z - xi.z, xn[k].w - xi.w) : f4zero();
        da[k] = dot4(dm, xk[k]);
        D = fmaf(ak[k], da[k], D);
    }
    float dsum = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float ds = ak[k] * (da[k] - D) * sc;
        dsum += ds;
        axpy4(dP, ds, xk[k]);
        if (live && k < deg) edge_out[tp[k]] = make_float2(ak[k] * dt, ds);
    }
    axpy4(dP, dsum, xi);
    const float dp[4] = {dP.x, dP.y, dP.z, dP.w}, xv4[4] = {xi.x, xi.y, xi.z, xi.w};
    float t4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int c = 0; c < 4; ++c) t4[c] = fmaf(dp[o], a4[o][c], t4[c]);
    if (live)
        *reinterpret_cast<float4*>(dxd + 4 * (size_t)i) =
            make_float4(fmaf(w1, g4.x, t4[0]), fmaf(w1, g4.y, t4[1]), fmaf(w1, g4.z, t4[2]), fmaf(w1, g4.w, t4[3]));
    float zero = 0.f;
    asm volatile("" : "+v"(zero));                               // the sums start at +0 and ADD their one node (the standalone kernel's loop): not folded
#pragma unroll
    for (int o = 0; o < 4; ++o) {
#pragma unroll
        for (int c = 0; c < 4; ++c) part[4 * o + c] = live ? fmaf(dp[o], xv4[c], zero) : 0.f;
        part[16 + o] = live ? zero + dp[o] : 0.f;
    }
}

template <bool HEAD, bool FLD, bool TOP = false>
__global__ __launch_bounds__(NRB_NT) void fwd_narrow_block_kernel(BlockArgs q) {
    static_assert(!TOP || HEAD, "the top layer's target pass rides in the launch that seeds the loss");
    __shared__ float4 rows[2][NRB_ROWS];                         // layer input rows / layer output rows, ping-pong
    __shared__ float astage[NRB_NT / 64][NRW_AST];
    __shared__ NarrowWLds wl;
    __shared__ float tred[TOP ? NRB_NT / 64 : 1][32];           // TOP: the 20 slab partials of each owned 64-node block, by block in node order
    const FwdArgs& p = q.f;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), h = lane >> 5;
    const int N = p.n_nodes, K = q.K;
    const int margin = gadapt_block_frame_margin(q.halo, K);
    const int own0 = NRB_NT * blockIdx.x, frame0 = own0 - margin, last_row = NRB_NT + 2 * margin - 1;
    const Cols4 cx = make_cols4(p.x_in, p.fs);                   // FLD: where the layer-0 rows come from
    const float* tgt_base = (HEAD && p.loss.target) ? p.loss.target : p.x_in;
    const int tgt_d = (HEAD && p.loss.target) ? p.loss.d : 1;
    const int row = blockIdx.x;                                  // cw: the row of A / p0 this workgroup writes (row < 64)

    // ---- the one global round trip: weights, {dt, scale} of every layer, this lane's two nodes, the loss target row of the owned one
    NarrowW wt;
    narrow_w_issue(wt, p, row, wave, lane);
    float dts[GADAPT_NARROW_BLOCK_LAYERS], scs[GADAPT_NARROW_BLOCK_LAYERS];
#pragma unroll
    for (int k = 0; k < GADAPT_NARROW_BLOCK_LAYERS; ++k) { dts[k] = p.lp[2 * min(k, K - 1)]; scs[k] = p.lp[2 * min(k, K - 1) + 1]; }
    NarrowIn tn[2];
    const int ell_rows = (N + 255) & ~255;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int i = frame0 + tid + NRB_NT * s, ie = min(max(i, 0), ell_rows - 1);   // (nodes outside [0, N) are in no layer's range)
        tn[s].ea = *reinterpret_cast<const int4*>(p.ell + 8 * (size_t)ie);
        tn[s].eb = *reinterpret_cast<const int4*>(p.ell + 8 * (size_t)ie + 4);
        tn[s].rp0 = p.rowptr[min(max(i, 0), N)];
        tn[s].rp1 = p.rowptr[min(max(i + 1, 0), N)];
        rows[0][tid + NRB_NT * s] = ld_x4<FLD>(cx, p.x_in, min(max(i, 0), N - 1));
    }
    const int so = 64 * wave < margin ? 1 : 0;                   // which of this wave's two blocks is owned
    if constexpr (TOP) {                                         // an owned block past ceil32(N) runs no layer: its partials are zeros
        if (lane < 32) tred[gadapt_block_owned_block(margin, wave)][lane] = 0.f;   // (the same wave writes them again: LDS operations complete in order)
    }
    float4 tgt = f4zero();
    if constexpr (HEAD) tgt = loss_target4(tgt_base, opaque(tgt_d), min(frame0 + tid + NRB_NT * so, N - 1));
    float fa[8];
    narrow_w_finish(fa, wt, wl, p, row, tid);
    float pv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) pv[r] = wt.pv[r];
    const Split3 af = split8(fa);
    __syncthreads();                                             // the frame is in LDS

    float loss_lv = 0.f;                                         // fused loss: this lane's terms
    float* sa = astage[wave];
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        int64_t lo64, hi64;
        gadapt_block_range(N, q.halo, K, blockIdx.x, k, &lo64, &hi64);
        const int klo = (int)lo64, khi = (int)hi64;
        const float dt = k == 0 ? dts[0] : (k == 1 ? dts[1] : (k == 2 ? dts[2] : dts[3]));
        const float sc = k == 0 ? scs[0] : (k == 1 ? scs[1] : (k == 2 ? scs[2] : scs[3]));
        const float4* cur = rows[k & 1];
        float4* nxt = rows[(k + 1) & 1];
        float* x_out = (k == K - 1 && q.x_last) ? q.x_last : p.x_top4 + k * q.slot_stride;
        float* alpha_out = p.alpha_out ? p.alpha_out + k * q.alpha_stride : nullptr;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int b0 = frame0 + 64 * wave + NRB_NT * s;      // this wave's block: nodes b0 .. b0 + 63
            if (b0 + 64 <= klo || b0 >= khi) continue;           // (workgroup barriers stay outside: every wave runs K of them)
            const int r = tid + NRB_NT * s, i = frame0 + r;      // this lane's frame row and node
            NarrowIn t1 = tn[s];
            t1.own = cur[r];
            v4f xv[8];
            {
                const int kmax = opaque(p.kmax);
                const int jn[8] = {t1.ea.x, t1.ea.y, t1.ea.z, t1.ea.w, t1.eb.x, t1.eb.y, t1.eb.z, t1.eb.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (e < kmax) {                              // (an index outside the frame - never on an eligible graph - is clamped into it)
                        const float4 v = cur[jn[e] < 0 ? r : (int)min((unsigned)max(jn[e] - frame0, 0), (unsigned)last_row)];
                        xv[e] = v4f{v.x, v.y, v.z, v.w};
                    }
                }
            }
            // TOP, the owned block of the last layer: what the target pass needs beyond the forward's operands is requested here, ahead of
            // the layer's arithmetic - the positions of this node's edges in source order (the one new global read: unconditional,
            // clamped as in bwd_target_compact_body) and the 4 x 4 corner of A (given, or this launch's own sums: the bits of a_out)
            [[maybe_unused]] int tp[8];
            [[maybe_unused]] float a4[4][4];
            if constexpr (TOP) {
                if (k == K - 1 && s == so) {
                    const int last = q.n_edges - 1;
#pragma unroll
                    for (int e = 0; e < 8; ++e) tp[e] = q.tpos[min(t1.rp0 + e, last)];
                    if (p.cw) {
#pragma unroll
                        for (int L = 0; L < 16; ++L)             // entry 16 o + c of the partial sums, o < 4, c < 4 of 16
                            a4[L >> 2][L & 3] = (wl.cpart[0][4 * L - 3 * (L & 3)] + wl.cpart[1][4 * L - 3 * (L & 3)]) +
                                                (wl.cpart[2][4 * L - 3 * (L & 3)] + wl.cpart[3][4 * L - 3 * (L & 3)]);
                    } else {
#pragma unroll
                        for (int L = 0; L < 16; ++L) a4[L >> 2][L & 3] = p.A[(L >> 2) * C + (L & 3)];
                    }
                }
            }
            // (this kernel's accumulators are VGPRs: 16 wait states between the last MFMA and the swaps that read it - an 8-pass MFMA needs 11)
#define GADAPT_NARROW_NODE_SETTLE(pa, pb) asm volatile("s_nop 15" : "+v"(pa), "+v"(pb))
#include "gadapt_narrow_node.inc"                                 // own, xc, deg, lo | hi, w[0..7] of node i
#undef GADAPT_NARROW_NODE_SETTLE

            if (i >= klo && i < khi) nxt[r] = make_float4(lo.x, lo.y, hi.x, hi.y);
            if (s != so) continue;                               // halo lanes store nothing
            [[maybe_unused]] float4 g4 = f4zero();               // TOP: the seed row of this lane's node
            if (i < N) {
                *reinterpret_cast<v4f*>(x_out + 4 * (size_t)i) = v4f{lo.x, lo.y, hi.x, hi.y};
                if (k == 0 && p.x0c) *reinterpret_cast<v4f*>(p.x0c + 4 * (size_t)i) = xc;   // the layer-0 input rows, for the layer-0 backward
                if constexpr (HEAD) {
                    if (k == K - 1 && p.loss.target) {
                        LossArgs la = p.loss;
                        la.d = opaque(tgt_d);                    // (= p.loss.d where there is a target)
                        if constexpr (TOP) loss_lv = loss_node_seed(la, i, make_float4(lo.x, lo.y, hi.x, hi.y), tgt, loss_lv, g4);
                        else loss_lv = loss_node(la, i, make_float4(lo.x, lo.y, hi.x, hi.y), tgt, loss_lv);
                    }
                }
            }
            // ---- alpha in CSR order: staged per wave, then coalesced stores
            if (alpha_out) {
                const int e_first = __builtin_amdgcn_readfirstlane(t1.rp0), e_cnt = __builtin_amdgcn_readlane(t1.rp1, 63) - e_first;
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (e < deg) sa[t1.rp0 - e_first + e] = w[e];
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // same wave: LDS operations complete in order
#pragma unroll
                for (int t = 0; t < 8; ++t)
                    if (64 * t + lane < e_cnt) alpha_out[e_first + 64 * t + lane] = sa[64 * t + lane];
            }
            // ---- TOP: the backward target pass of the top layer on this node (every lane of the owned block; lanes past N add zeros)
            if constexpr (TOP) {
                if (k == K - 1) {
                    __builtin_amdgcn_sched_barrier(0);           // behind the node statements: nothing of it among the MFMA results' readers
                    float part[20];
                    narrow_top_target(part, g4, own, xv, w, deg, dt, sc, a4, tp, i < N, i, q.edge_out, q.dxd);
                    const int ob = gadapt_block_owned_block(margin, wave);
                    // the wave sum of bwd_target_compact_body, butterfly 32, 16, .., 1 - the same additions on DPP / lane swaps, stage by
                    // stage over the 20 independent values, each total in the one lane that parks it (wave_sum_scatter: wave_sum_desc's
                    // additions; every lane of the owned block's wave is here: halo waves left at the `continue` above as a whole, lanes
                    // past N carry zeros)
                    const float tot = wave_sum_scatter(part, lane);
                    const int pe = wave_sum_scatter_entry(lane);
                    if (pe >= 0) tred[ob][pe] = tot;
                }
            }
        }
        if (k + 1 < K) __syncthreads();                          // layer k is in LDS; its input buffer is free for layer k + 1's output
    }
    if constexpr (HEAD) { if (p.loss.target) loss_wave_partial<NRB_NT / 64>(p.loss, loss_lv, tid); }   // every wave of the grid owns a slot
    if constexpr (TOP) {
        // ---- the slab rows this tile owes (gadapt_block_slab_plan): rows 2 t and 2 t + 1 = (b0 + b1) + (b2 + b3) over their four blocks in
        // node order, entries 20..31 zero; then its share of the rows no tile has nodes for.  Every wave arrives: each owns one block.
        __syncthreads();
        const gadapt_block_slab sp = gadapt_block_slab_plan(N, margin, blockIdx.x);
        if (tid < 2 * GADAPT_NARROW_SLAB_ROW) {
            const int j = tid >> 5, e = tid & 31, r = j ? sp.rows[1] : sp.rows[0];   // (a select: indexed, the plan would live in scratch)
            if (r < q.slab_rows)
                q.slab[(size_t)r * GADAPT_NARROW_SLAB_ROW + e] =
                    e < 20 ? (tred[4 * j][e] + tred[4 * j + 1][e]) + (tred[4 * j + 2][e] + tred[4 * j + 3][e]) : 0.f;
        }
        if (tid < GADAPT_NARROW_SLAB_ROW)
            for (int r = sp.zero_first; r < q.slab_rows; r += sp.zero_step) q.slab[(size_t)r * GADAPT_NARROW_SLAB_ROW + tid] = 0.f;
    }
}

}  // namespace wide
