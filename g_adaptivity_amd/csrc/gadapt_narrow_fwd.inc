// gadapt_narrow_fwd.inc - forward layer of the narrow route (gadapt_block_forward_narrow), included by gadapt_tu_fwd.hip after
// gadapt_wide.inc.
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

        // ---- P[0..3] = (A x + p0)[0..3] on the matrix cores, two 32-node groups
        const float4 own = t1.own;
        float xa[4] = {own.x, own.y, own.z, own.w}, xb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c) swap32(xa[c], xb[c]);      // xa: own row in lanes 0..31, zeros above; xb: rows of lanes 32..63, moved down
        const float va[8] = {xa[0], xa[1], xa[2], xa[3], 0.f, 0.f, 0.f, 0.f};
        const float vb[8] = {xb[0], xb[1], xb[2], xb[3], 0.f, 0.f, 0.f, 0.f};
        const Split3 ba = split8(va), bb = split8(vb);
        f32x16 Pa, Pb;
#pragma unroll
        for (int q = 0; q < 16; ++q) { Pa[q] = (q < 4 && h == 0) ? pv[q & 3] : 0.f; Pb[q] = Pa[q]; }
        mfma6r(Pa, af, ba);
        mfma6r(Pb, af, bb);
        float P4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { float a = Pa[r], b = Pb[r]; swap32(a, b); P4[r] = a; }

        // ---- edge walk (wide::fwd_kernel's expressions on chunk 0)
        const int kmax = opaque(p.kmax);
        const int deg = (i < N) ? t1.rp1 - t1.rp0 : 0;
        v2f acc[2] = {v2f{0.f, 0.f}, v2f{0.f, 0.f}};
        float w[8];
        float mref = 0.f, den = 0.f;
        const v2f plo = {P4[0], P4[1]}, phi = {P4[2], P4[3]};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            w[k] = 0.f;
            if (k < kmax) {
                v2f d[4] = {v2f{0.f, 0.f}, v2f{0.f, 0.f}, v2f{0.f, 0.f}, v2f{0.f, 0.f}};
                d[0] += plo * xv[k].xy;
                d[1] += phi * xv[k].zw;
                const v2f dd = (d[0] + d[1]) + (d[2] + d[3]);
                const float sk = ((dd.x + dd.y) + 0.f) * sc;     // (+ the wide kernel's other half: an exact +0)
                const bool valid = k < deg;
                float wk;
                if (k == 0) {
                    mref = valid ? sk : 0.f;
                    wk = valid ? 1.f : 0.f;
                } else {
                    float dlt = sk - mref;
                    const unsigned long long bal = __builtin_amdgcn_ballot_w64(valid && dlt > REBASE);
                    if ((h ? (unsigned)(bal >> 32) : (unsigned)bal) != 0u) {   // rare: re-base every node of the 32-node group
                        const float nref = valid ? fmaxf(mref, sk) : mref;
                        const float corr = sm_exp(mref - nref);
                        den *= corr;
                        acc[0] *= corr; acc[1] *= corr;
#pragma unroll
                        for (int kk = 0; kk < k; ++kk) w[kk] *= corr;
                        mref = nref;
                        dlt = sk - mref;
                    }
                    wk = valid ? sm_exp(dlt) : 0.f;
                }
                w[k] = wk;
                den += wk;
                acc[0] += xv[k].xy * wk;
                acc[1] += xv[k].zw * wk;
            }
        }
        // ---- x' = x + dt (m - x), alpha = w / (sum + 1e-16)
        const float inv = sm_rcp(den + 1e-16f);
        const v4f xc = v4f{own.x, own.y, own.z, own.w};
        v2f lo = acc[0] * inv - xc.xy, hi = acc[1] * inv - xc.zw;
        if (!p.residual_only) { lo = xc.xy + lo * dt; hi = xc.zw + hi * dt; }
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] *= inv;

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

}  // namespace wide
