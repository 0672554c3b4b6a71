// gadapt_common.inc - compile-time geometry, lane/row helpers, the split-precision tile GEMM, LDS staging of CSR slices and row tiles shared by the tiled kernels (included by every translation unit through gadapt_internal.h; gfx950 only).

// ------------------------------------------------------------------------------------------------
// compile-time geometry
// ------------------------------------------------------------------------------------------------
template <int C> struct Cfg {
    static constexpr bool MFMA = (C >= 32);
    static constexpr int FPL = MFMA ? 8 : 4;  // floats per lane
    static constexpr int NV = FPL / 4;                 // float4 chunks per lane
    static constexpr int LPN = C / FPL;                // lanes per node
    static constexpr int NT = 256;                     // threads per workgroup
    static constexpr int NW = NT / 64;                 // waves per workgroup
    static constexpr int SLOTS = NT / LPN;             // nodes in flight per workgroup
    static constexpr int TM = MFMA ? (C == 32 ? 128 : 64) : (SLOTS < 64 ? 64 : SLOTS);
    static constexpr int ITERS = TM / SLOTS;
    static constexpr int LD = C + 4;                   // padded LDS row (floats): conflict-free b128 rows
    static constexpr int TILE_FLOATS = TM * LD;
    static constexpr int CB = C / 32;                  // 32-wide column blocks (MFMA path)
    static constexpr int RB = TM / 32;                 // 32-high row blocks
    static constexpr int CAP = 7 * TM;                 // CSR entries of one tile staged in LDS (rest read from HBM)
    static constexpr int COLN = CAP + 64;              // + padding: reads up to MAXD past a row's end stay in
                                                       //   bounds and return a valid node id (weight 0)
    // LDS: `tiles` [TM][LD] tiles, rowptr[TM+1] (padded to TM+4), col[COLN], aux[AUXW*COLN]
    static constexpr int MAXM = 64;                    // tile-metadata words of this workgroup's tiles kept in LDS
    static constexpr int lds_bytes(int auxw, int tiles = 2, int ext = 0) { return (tiles * TILE_FLOATS + (TM + 4) + COLN + (auxw + ext) * COLN + 4 * MAXM) * 4; }
    static constexpr int RING = C <= 64 ? 3 : 1;   // LDS slabs of x rows kept by the rolling-window kernels; C = 128: a
                                                       //   3-slab window would leave one workgroup per CU, so only the tile itself
    static constexpr int LEAD = (RING == 3) ? 1 : 0;   // the slab staged during tile t is slab t + LEAD
    // The target pass keeps the window at hidden 128 too: its 392 registers allow one workgroup per CU whatever the LDS
    // footprint is (4 tiles of 33 KB + slices = 145 KB), and at one wave per SIMD an L2 gather is fully exposed latency.
    static constexpr int RING_T = 3;
    static constexpr int LEAD_T = (RING_T == 3) ? 1 : 0;
};

__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float dot4(const float4& a, const float4& b) {
    return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)));
}
__device__ __forceinline__ void axpy4(float4& y, float a, const float4& x) {
    y.x = fmaf(a, x.x, y.x); y.y = fmaf(a, x.y, y.y); y.z = fmaf(a, x.z, y.z); y.w = fmaf(a, x.w, y.w);
}

// Sum over the LPN lanes that share a node, result in every lane.  DPP row operations (no LDS
// crossbar): quad_perm xor-1 / xor-2, row_half_mirror, row_mirror; the 32-lane case adds one
// ds_swizzle (xor 16).
template <int CTRL> __device__ __forceinline__ float dpp_add(float v) {
    const int moved = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true);
    return v + __builtin_bit_cast(float, moved);
}
template <int LPN> __device__ __forceinline__ float group_sum(float v) {
    if constexpr (LPN >= 2) v = dpp_add<0xB1>(v);      // quad_perm [1,0,3,2]
    if constexpr (LPN >= 4) v = dpp_add<0x4E>(v);      // quad_perm [2,3,0,1]
    if constexpr (LPN >= 8) v = dpp_add<0x141>(v);     // row_half_mirror
    if constexpr (LPN >= 16) v = dpp_add<0x140>(v);    // row_mirror
    if constexpr (LPN >= 32) v += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F));
    return v;
}

// Row gather with a 32-bit byte offset (the launcher checks N*C*4 < 4 GiB).
template <int C> __device__ __forceinline__ float4 ld_row4(const float* __restrict__ base, int row, int sub) {
    const uint32_t off = (uint32_t)row * (uint32_t)(C * 4) + (uint32_t)sub * 16u;
    return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + off);
}
// streaming forms (read or written once per launch: keep them from displacing the rows other workgroups gather through L2)
typedef float f32x4nt __attribute__((ext_vector_type(4)));
template <int C> __device__ __forceinline__ float4 ld_row4_nt(const float* __restrict__ base, int row, int sub) {
    const uint32_t off = (uint32_t)row * (uint32_t)(C * 4) + (uint32_t)sub * 16u;
    const f32x4nt v = __builtin_nontemporal_load(reinterpret_cast<const f32x4nt*>(reinterpret_cast<const char*>(base) + off));
    return make_float4(v.x, v.y, v.z, v.w);
}
template <int C> __device__ __forceinline__ void st_row4_nt(float* __restrict__ base, int row, int sub, const float4& v) {
    const uint32_t off = (uint32_t)row * (uint32_t)(C * 4) + (uint32_t)sub * 16u;
    const f32x4nt t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, reinterpret_cast<f32x4nt*>(reinterpret_cast<char*>(base) + off));
}
template <int C> __device__ __forceinline__ void st_row4(float* __restrict__ base, int row, int sub, const float4& v) {
    const uint32_t off = (uint32_t)row * (uint32_t)(C * 4) + (uint32_t)sub * 16u;
    *reinterpret_cast<float4*>(reinterpret_cast<char*>(base) + off) = v;
}

// Tiles [t, t_end) step `step` for this workgroup.  Workgroups with equal blockIdx%8 are observed to
// share an XCD (placement is a speed assumption only); each such group walks one contiguous eighth
// of the tiles so gathered neighbour rows hit that XCD's L2.
struct TileRange { int t, t_end, step; };
__device__ __forceinline__ TileRange tile_range(int n_tiles) {
    const int gx = gridDim.x >> 3, xcd = blockIdx.x & 7, bi = blockIdx.x >> 3;
    const int per = (n_tiles + 7) >> 3;
    const int t0 = xcd * per;
    const int t1 = min(n_tiles, t0 + per);
    return {t0 + bi, t1, gx};
}

// Contiguous tiles [t0, t1) for this workgroup (rolling-window kernels): XCD group x walks the x-th eighth of the
// tiles, split evenly between that group's workgroups.
struct TileChunk { int t0, t1; };
__device__ __forceinline__ TileChunk tile_chunk(int n_tiles) {
    const int gx = gridDim.x >> 3, xcd = blockIdx.x & 7, bi = blockIdx.x >> 3;
    const int per = (n_tiles + 7) >> 3;
    const int x0 = xcd * per, x1 = min(n_tiles, x0 + per);
    if (x1 <= x0) return {0, 0};
    const int pw = (x1 - x0 + gx - 1) / gx;
    const int t0 = x0 + bi * pw;
    return {min(t0, x1), min(x1, t0 + pw)};
}

// ------------------------------------------------------------------------------------------------
// [TM,C] x [C,C] on the matrix cores.  D[n][j] = sum_k IN[n][k] * B[k][j] (+ bias[j]).
//   TRANS = false: B[k][j] = M[j*C + k]   (D = IN M^T : forward P = x A^T, source pass A y)
//   TRANS = true : B[k][j] = M[k*C + j]   (D = IN M   : target pass dP A)
// v_mfma_f32_32x32x2_f32: lane l feeds A[l&31][k=l>>5] and B[k=l>>5][l&31]; the k index is
// permuted so each lane-half reads 16 contiguous bytes of its IN row per 4 MFMAs (half h owns
// k in {8q+4h .. 8q+4h+3}); any permutation is valid as long as A and B agree.
// ------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// fp32 values on the bf16 matrix cores without losing fp32 accuracy: x = h + m + l exactly, three bf16 pieces of 8
// mantissa bits each (truncation; every subtraction is exact).  A product x*y keeps the six piece products down to
// 2^-16 relative (hh, hm, mh, mm, hl, lh); the dropped ones (ml, lm, ll) are below 2^-23 of |x*y|, the rounding
// level of an fp32 product, and every piece product is exact in the fp32 accumulator.  v_mfma_f32_32x32x16_bf16
// does 16x the work of v_mfma_f32_32x32x2_f32 in half its cycles, so six of them per 16 k cost 3/8 of the fp32 form.
struct Split3 { u32x4 h, m, l; };
// (The same pipeline over the dA phase's (k-step, block) sequence was measured slower - target pass 32.5 -> 35.1 us at hidden
// 64, 97 -> 104.5 at hidden 128 - and its sched_group_barrier patterns took the build from 2 to 16 minutes: not kept.)
__device__ __forceinline__ Split3 split8(const float (&x)[8]) {
    Split3 s;
    float r[8], r2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        r[e] = x[e] - __uint_as_float(__float_as_uint(x[e]) & 0xFFFF0000u);
        r2[e] = r[e] - __uint_as_float(__float_as_uint(r[e]) & 0xFFFF0000u);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {                       // element 2q in the low half, 2q+1 in the high half
        s.h[q] = __builtin_amdgcn_perm(__float_as_uint(x[2 * q + 1]), __float_as_uint(x[2 * q]), 0x07060302u);
        s.m[q] = __builtin_amdgcn_perm(__float_as_uint(r[2 * q + 1]), __float_as_uint(r[2 * q]), 0x07060302u);
        s.l[q] = __builtin_amdgcn_perm(__float_as_uint(r2[2 * q + 1]), __float_as_uint(r2[2 * q]), 0x07060302u);
    }
    return s;
}
__device__ __forceinline__ f32x16 mfma_bf16(const u32x4& a, const u32x4& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// Two-piece f16 form (where it is used: see below): the operand block is first multiplied by a power of two that brings its
// largest magnitude into [2^14, 2^15) - exact, and it puts the whole block into f16's range - then x = h + l with
// h = f16(x) and l = f16(x - h), round to nearest: 22 to 23 significant bits, |x - h - l| <= 2^-23 |x| or 2^-25 (f16's
// subnormal spacing, i.e. 2^-39 of the block's maximum), whichever is larger.  Products: hh + hl + lh (ll is below 2^-22
// of |x y| and 2^-24 on average, the rounding level of an fp32 product), every piece product exact in the fp32
// accumulator; the result is multiplied by the inverse powers of two.  Against the three-piece bf16 form (split8): half
// the matrix instructions (3 per 16 k instead of 6), 24 instead of 44 vector instructions per 8 values, fragments of 8
// instead of 12 registers per k-step; in exchange a maximum per scale group per use.  Scale groups follow the operand
// layout so that they cost two or three cross-lane steps and no wave-wide reduction (a first version with one scale per
// wave block - DPP reduction, readfirstlane - serialised every matrix phase behind it and was slower than the bf16 form):
// the A operand (lane (i, h): row i, half h of each k-step) shares a scale between FOUR consecutive rows - quad DPP and
// one half swap - because the 32x32 output layout gives a lane four consecutive rows per register quad, so it fetches four
// inverses (ds_bpermute) instead of sixteen; the B operand (lane (j, h): column j) has one scale per column, lane-local
// after the half swap.  An entry 2^-q below its group's maximum keeps min(23, 39 - q) bits.
// Measured (MI355X, same box, us per launch, bf16 three-piece -> f16 two-piece): source pass 26.8 -> 25.9 (hidden 64),
// 86.5 -> 83.4 (hidden 128); tiled forward 61.0 -> 60.3 (hidden 128); wide forward 17.9 -> 18.0; target pass 32.6 -> 34.6
// (hidden 64), 96.4 -> 98.6 (hidden 128): the f16 form has to hold a whole operand block until its maximum is known, where the
// bf16 form streams k-step by k-step, and the target pass has neither the registers (3 spills) nor the slack for that.  With
// the scales known in advance (diagnostic build, unit scale) the target pass would gain 0.9 / 7 us - not pursued.
// Tiled forward at hidden 64 (128-wide meshes): 50.1 -> 52.0; at hidden 32: 12.6 -> 12.4.
// So: on for the source pass and for the tiled forward at hidden 32 / 128, off for the target pass and the wide forward.
// tiled forward P = x A^T: the f16 form except at hidden 64
constexpr bool split_f16_fwd(int c) { return c != 64; }
// (The dA phase of the target pass on the fp32 matrix instruction - v_mfma_f32_32x32x2_f32, no operand splits - measured slower at
// every hidden size, docs/measurements.md J: 32 fp32 matrix instructions of 64 cycles per wave and tile are a longer chain than six
// bf16 ones per 16 nodes plus their splits.  Removed in round 6.)
// PRE-SPLIT A operand: the [TM,C] operand tile is written to LDS ONCE, already in the two-piece f16
// form, by the lanes that own its rows - one power-of-two scale per ROW (a lane group holds a whole row: its maximum is a DPP
// reduction over the group), h and l pieces of 8 consecutive k side by side in the 32 bytes the 8 fp32 values would take, so
// the tile keeps its footprint and a matrix-core lane fetches a k-step's fragment pair with two ds_read_b128 and NO vector
// arithmetic.  The per-wave splits this replaces are redundant across the waves that share rows: x4 at hidden 128 (every
// wave split the whole tile: 704 vector instructions per lane and tile in the target pass's projection, 1584 with its dA
// phase, a quarter of the kernel), x2 at hidden 64.  The row's inverse scale stays with the lanes that wrote the row - the
// same lanes read the product's row back and fold it into that read.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
struct Split2 { u32x4 h, l; };
struct Pow2 { float s, inv; };
// largest power-of-two scale that keeps mx below 2^15, and its inverse (both normal fp32 numbers for every mx)
__device__ __forceinline__ Pow2 pow2_scale(float mx) {
    int e = (int)((__float_as_uint(mx) >> 23) & 0xFFu);
    e = min(max(e, 15), 254);
    return {__uint_as_float((unsigned)(268 - e) << 23), __uint_as_float((unsigned)(e - 14) << 23)};
}
template <int CTRL> __device__ __forceinline__ float dpp_max(float v) {
    const int moved = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true);
    return fmaxf(v, __builtin_bit_cast(float, moved));
}
// max(v(lane), v(lane ^ 32)), in both lanes
__device__ __forceinline__ float half_max(float v) {
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return fmaxf(a, b);
}
// scale of an A-operand lane (row r31, half h): maximum over the four rows 4 (r31 / 4) .. + 3 and both halves
__device__ __forceinline__ float quad_rows_max(float v) {
    v = dpp_max<0xB1>(v); v = dpp_max<0x4E>(v);
    return half_max(v);
}
// the four inverse scales a lane of the 32x32 output needs: register r holds row (r & 3) + 8 (r >> 2) + 4 h, i.e. row quad
// 2 (r >> 2) + h, whose scale sits in lane 8 (r >> 2) + 4 h of the A operand
__device__ __forceinline__ void quad_rows_inverse(float inv, int h, float (&out)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
        out[q] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(32 * q + 16 * h, __builtin_bit_cast(int, inv)));
}
// maximum of a non-negative value over the wave, wave-uniform (scalar register)
__device__ __forceinline__ float wave_max(float v) {
    v = dpp_max<0xB1>(v); v = dpp_max<0x4E>(v); v = dpp_max<0x141>(v); v = dpp_max<0x140>(v);     // rows of 16 lanes
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F)));   // xor 16
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));                   // xor 32
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, fmaxf(a, b))));
}
__device__ __forceinline__ float absmax8(const float (&x)[8], float m) {
#pragma unroll
    for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(x[e]));
    return m;
}
__device__ __forceinline__ Split2 split8h(const float (&x)[8], float s) {
    Split2 r;
#pragma unroll
    for (int q = 0; q < 4; ++q) {                       // element 2q in the low half, 2q+1 in the high half
        const float t0 = x[2 * q] * s, t1 = x[2 * q + 1] * s;
        f16x2 h; h.x = (_Float16)t0; h.y = (_Float16)t1;
        f16x2 l; l.x = (_Float16)(t0 - (float)h.x); l.y = (_Float16)(t1 - (float)h.y);   // the differences are exact
        r.h[q] = __builtin_bit_cast(unsigned, h);
        r.l[q] = __builtin_bit_cast(unsigned, l);
    }
    return r;
}
__device__ __forceinline__ f32x16 mfma_f16(const u32x4& a, const u32x4& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mma3(const Split2& a, const Split2& b, f32x16 c) {
    c = mfma_f16(a.h, b.l, c);                          // small pieces first
    c = mfma_f16(a.l, b.h, c);
    return mfma_f16(a.h, b.h, c);
}

// Instruction order for the scheduler (sched_group_barrier): NDS LDS reads, then six times {one matrix instruction, NVALU
// vector instructions} - the shape of one software-pipelined k-step of the split products.
template <int NDS, int NVALU, int NM = 6> __device__ __forceinline__ void mfma_gap_pattern() {
    if constexpr (NDS > 0) __builtin_amdgcn_sched_group_barrier(0x100, NDS, 0);
#pragma unroll
    for (int g = 0; g < NM; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, NVALU, 0);
    }
}

template <int C, bool TRANS, bool F16_ = false> struct TileGemm {
    using K = Cfg<C>;
    static constexpr int BPW = (K::CB * K::RB) / K::NW;   // 32x32 output blocks per wave
    static_assert(!K::MFMA || ((K::CB * K::RB) % K::NW == 0 && K::NW % K::CB == 0), "output blocks split evenly over the waves");
    static constexpr bool SPLIT = true;               // every matrix-core size (32, 64, 128) runs the split forms
    static constexpr int KS = C / 16;                  // k-steps of the bf16 form
    static constexpr bool F16 = SPLIT && F16_;
    float bf[SPLIT ? 1 : C / 2];
    Split3 bs[(SPLIT && !F16) ? KS : 1];
    Split2 bh[F16 ? KS : 1];
    float binv;                                        // F16: inverse scale of this lane's B column
    float oinv[BPW][4];                                // F16: inverse of (A scale x B scale) of the last accumulate: output block, row quad
    float bias;
    int cb, rb0, lane;

    __device__ __forceinline__ void init(int lane_, int wave) {
        lane = lane_;
        cb = wave % K::CB;
        rb0 = wave / K::CB;
    }
    // Issue the B-operand loads ([C,C] matrix: L2-resident, same lines for every workgroup).
    __device__ __forceinline__ void load(const float* __restrict__ M, const float* __restrict__ bias_vec) {
        const int h = lane >> 5, j = cb * 32 + (lane & 31);
        if constexpr (F16) {
            float v[KS][8];
            float mx = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (!TRANS) {
                    const float4 v0 = *reinterpret_cast<const float4*>(M + (size_t)j * C + 16 * ks + 8 * h);
                    const float4 v1 = *reinterpret_cast<const float4*>(M + (size_t)j * C + 16 * ks + 8 * h + 4);
                    v[ks][0] = v0.x; v[ks][1] = v0.y; v[ks][2] = v0.z; v[ks][3] = v0.w;
                    v[ks][4] = v1.x; v[ks][5] = v1.y; v[ks][6] = v1.z; v[ks][7] = v1.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[ks][e] = M[(size_t)(16 * ks + 8 * h + e) * C + j];
                }
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) mx = absmax8(v[ks], mx);
            const Pow2 sb = pow2_scale(half_max(mx));
            binv = sb.inv;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) bh[ks] = split8h(v[ks], sb.s);
        } else if constexpr (SPLIT) {
            // lane (j, h) holds B[k][j] for k = 16 ks + 8 h + e, e = 0..7 (both operands use this k order)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                float v[8];
                if (!TRANS) {
                    const float4 v0 = *reinterpret_cast<const float4*>(M + (size_t)j * C + 16 * ks + 8 * h);
                    const float4 v1 = *reinterpret_cast<const float4*>(M + (size_t)j * C + 16 * ks + 8 * h + 4);
                    v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w; v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = M[(size_t)(16 * ks + 8 * h + e) * C + j];
                }
                bs[ks] = split8(v);
            }
        } else {
#pragma unroll
            for (int q = 0; q < C / 8; ++q) {
                if (!TRANS) {
                    const float4 v = *reinterpret_cast<const float4*>(M + (size_t)j * C + 8 * q + 4 * h);
                    bf[4 * q + 0] = v.x; bf[4 * q + 1] = v.y; bf[4 * q + 2] = v.z; bf[4 * q + 3] = v.w;
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) bf[4 * q + t] = M[(size_t)(8 * q + 4 * h + t) * C + j];
                }
            }
        }
        bias = bias_vec ? bias_vec[j] : 0.f;
    }

    // The same in two halves: the loads are requested before other work (a launch's prologue: ahead of the window requests and of the
    // scalar metadata trip; the hidden-128 forward, which rebuilds the fragments per tile: ahead of the staging commits), the split runs
    // after it - the L2 round trip is no longer exposed.
    struct BRaw { float v[SPLIT ? KS : 1][8]; float bias; };
    __device__ __forceinline__ void load_issue(const float* __restrict__ M, const float* __restrict__ bias_vec, BRaw& raw) const {
        raw.bias = bias_vec ? bias_vec[cb * 32 + (lane & 31)] : 0.f;
        if constexpr (SPLIT) {
            const int h = lane >> 5, j = cb * 32 + (lane & 31);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (!TRANS) {
                    const float4 v0 = *reinterpret_cast<const float4*>(M + (size_t)j * C + 16 * ks + 8 * h);
                    const float4 v1 = *reinterpret_cast<const float4*>(M + (size_t)j * C + 16 * ks + 8 * h + 4);
                    raw.v[ks][0] = v0.x; raw.v[ks][1] = v0.y; raw.v[ks][2] = v0.z; raw.v[ks][3] = v0.w;
                    raw.v[ks][4] = v1.x; raw.v[ks][5] = v1.y; raw.v[ks][6] = v1.z; raw.v[ks][7] = v1.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) raw.v[ks][e] = M[(size_t)(16 * ks + 8 * h + e) * C + j];
                }
            }
        }
    }
    __device__ __forceinline__ void load_finish(const BRaw& raw) {
        bias = raw.bias;
        if constexpr (F16) {
            float mx = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) mx = absmax8(raw.v[ks], mx);
            const Pow2 sb = pow2_scale(half_max(mx));
            binv = sb.inv;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) bh[ks] = split8h(raw.v[ks], sb.s);
        } else {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) bs[ks] = split8(raw.v[ks]);
        }
    }

    // in_tile/out_tile: LDS [TM][LD].  Caller synchronises around it.
    // KSU: k-steps that carry data (the caller knows the operand is zero beyond 16 KSU columns: compact layer input)
    template <int KSU = KS> __device__ __forceinline__ void accumulate(const float* in_tile, f32x16 (&acc)[BPW]) {
        const int h = lane >> 5, r31 = lane & 31;
#pragma unroll
        for (int b = 0; b < BPW; ++b) {
            const int rb = rb0 + b * (K::NW / K::CB);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
            if constexpr (F16) {
                const float* arow = in_tile + (rb * 32 + r31) * K::LD + 8 * h;
                auto rd = [&](int ks, float (&v)[8]) __attribute__((always_inline)) {
                    const float4 a0 = *reinterpret_cast<const float4*>(arow + 16 * ks);
                    const float4 a1 = *reinterpret_cast<const float4*>(arow + 16 * ks + 4);
                    v[0] = a0.x; v[1] = a0.y; v[2] = a0.z; v[3] = a0.w; v[4] = a1.x; v[5] = a1.y; v[6] = a1.z; v[7] = a1.w;
                };
                float mx = 0.f;
                if constexpr (KSU <= 4) {                               // the block's rows stay in registers between the two uses
                    float v[KSU][8];
#pragma unroll
                    for (int ks = 0; ks < KSU; ++ks) rd(ks, v[ks]);
#pragma unroll
                    for (int ks = 0; ks < KSU; ++ks) mx = absmax8(v[ks], mx);
                    const Pow2 sa = pow2_scale(quad_rows_max(mx));
                    quad_rows_inverse(sa.inv, h, oinv[b]);
                    Split2 cur = split8h(v[0], sa.s);
#pragma unroll
                    for (int ks = 0; ks < KSU; ++ks) {                  // split of k-step ks+1 in the gaps of the three products of ks
                        Split2 nxt = cur;
                        if (ks + 1 < KSU) nxt = split8h(v[ks + 1], sa.s);
                        acc[b] = mma3(cur, bh[ks], acc[b]);
                        if (ks + 1 < KSU) mfma_gap_pattern<0, 8, 3>();
                        cur = nxt;
                    }
                } else {                                               // hidden 128: read twice rather than hold 64 registers
#pragma unroll
                    for (int ks = 0; ks < KSU; ++ks) { float v[8]; rd(ks, v); mx = absmax8(v, mx); }
                    const Pow2 sa = pow2_scale(quad_rows_max(mx));
                    quad_rows_inverse(sa.inv, h, oinv[b]);
                    float v0[8];
                    rd(0, v0);
                    Split2 cur = split8h(v0, sa.s);
#pragma unroll
                    for (int ks = 0; ks < KSU; ++ks) {
                        Split2 nxt = cur;
                        if (ks + 1 < KSU) { float v[8]; rd(ks + 1, v); nxt = split8h(v, sa.s); }
                        acc[b] = mma3(cur, bh[ks], acc[b]);
                        if (ks + 1 < KSU) mfma_gap_pattern<2, 8, 3>();
                        cur = nxt;
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) oinv[b][q] *= binv;
            } else if constexpr (SPLIT) {
                const float* arow = in_tile + (rb * 32 + r31) * K::LD + 8 * h;
                auto ldsplit = [&](int ks) __attribute__((always_inline)) {
                    const float4 a0 = *reinterpret_cast<const float4*>(arow + 16 * ks);
                    const float4 a1 = *reinterpret_cast<const float4*>(arow + 16 * ks + 4);
                    const float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                    return split8(v);
                };
                // Software pipeline: the split of k-step ks+1 (44 vector instructions) is issued in the gaps of the six matrix
                // instructions of k-step ks.  A wave issues in order, so six matrix instructions back to back (192 cycles of
                // pipe time, 8 cycles of issue each) followed by the next split leave the matrix pipe idle during the split and
                // the vector ALU idle during the six: 384 cycles per k-step measured at one wave per SIMD (hidden 128).
                Split3 cur = ldsplit(0);
#pragma unroll
                for (int ks = 0; ks < KSU; ++ks) {
                    Split3 nxt = cur;
                    if (ks + 1 < KSU) nxt = ldsplit(ks + 1);
                    acc[b] = mfma_bf16(cur.h, bs[ks].l, acc[b]);        // small pieces first
                    acc[b] = mfma_bf16(cur.l, bs[ks].h, acc[b]);
                    acc[b] = mfma_bf16(cur.m, bs[ks].m, acc[b]);
                    acc[b] = mfma_bf16(cur.h, bs[ks].m, acc[b]);
                    acc[b] = mfma_bf16(cur.m, bs[ks].h, acc[b]);
                    acc[b] = mfma_bf16(cur.h, bs[ks].h, acc[b]);
                    if (ks + 1 < KSU) mfma_gap_pattern<2, 8>();
                    cur = nxt;
                }
            } else {
                const float* arow = in_tile + (rb * 32 + r31) * K::LD + 4 * h;
#pragma unroll
                for (int q = 0; q < C / 8; ++q) {
                    const float4 a = *reinterpret_cast<const float4*>(arow + 8 * q);
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bf[4 * q + 0], acc[b], 0, 0, 0);
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bf[4 * q + 1], acc[b], 0, 0, 0);
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bf[4 * q + 2], acc[b], 0, 0, 0);
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bf[4 * q + 3], acc[b], 0, 0, 0);
                }
            }
        }
    }
    __device__ __forceinline__ void store(float* out_tile, const f32x16 (&acc)[BPW]) const {
        const int h = lane >> 5, r31 = lane & 31;
#pragma unroll
        for (int b = 0; b < BPW; ++b) {
            const int rb = rb0 + b * (K::NW / K::CB);
            float* ocol = out_tile + cb * 32 + r31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                ocol[row * K::LD] = F16 ? fmaf(acc[b][r], oinv[b][r >> 2], bias) : acc[b][r] + bias;
            }
        }
    }
    // PRE-SPLIT A operand (lds_put_split): in_tile holds, per row and group of 8 k, the h pieces (16 bytes) then the l pieces
    __device__ __forceinline__ void accumulate_presplit(const float* in_tile, f32x16 (&acc)[BPW]) const {
        static_assert(F16, "pre-split operands are two-piece f16");
        const int h = lane >> 5, r31 = lane & 31;
#pragma unroll
        for (int b = 0; b < BPW; ++b) {
            const int rb = rb0 + b * (K::NW / K::CB);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
            const float* arow = in_tile + (rb * 32 + r31) * K::LD + 8 * h;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                Split2 a;
                a.h = *reinterpret_cast<const u32x4*>(arow + 16 * ks);
                a.l = *reinterpret_cast<const u32x4*>(arow + 16 * ks + 4);
                acc[b] = mma3(a, bh[ks], acc[b]);
            }
        }
    }
    // result of accumulate_presplit times the B column's inverse scale; the row's inverse scale is applied by the reader
    __device__ __forceinline__ void store_presplit(float* out_tile, const f32x16 (&acc)[BPW]) const {
        const int h = lane >> 5, r31 = lane & 31;
#pragma unroll
        for (int b = 0; b < BPW; ++b) {
            const int rb = rb0 + b * (K::NW / K::CB);
            float* ocol = out_tile + cb * 32 + r31;
#pragma unroll
            for (int r = 0; r < 16; ++r) ocol[(rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * K::LD] = acc[b][r] * binv;
        }
    }
    template <int KSU = KS> __device__ __forceinline__ void run(const float* in_tile, float* out_tile) {
        f32x16 acc[BPW];
        accumulate<KSU>(in_tile, acc);
        store(out_tile, acc);
    }
    // out == in: every wave reads its operand rows before any wave overwrites them (two workgroup barriers inside)
    __device__ __forceinline__ void run_in_place(float* tile) {
        f32x16 acc[BPW];
        accumulate(tile, acc);
        __syncthreads();
        store(tile, acc);
    }
};

// The tile's slice of one CSR orientation in LDS: rowptr[TM+1], col[COLN] and AUXW per-edge words.  Where the slice
// starts, how long it is and the tile's longest row come from per-tile metadata built with the graph
// (gadapt_tile_meta_host), so every load of the stage is issued at once: one memory round trip per tile.
// A tile whose slice does not fit (more than CAP entries) or that has a row longer than MAXD is "slow":
// the whole workgroup walks the HBM copy with plain loops instead.
// EXT = 1: one more per-edge int32 array (separate in HBM) staged with the slice.  EXT = 2: no such array in HBM - the LDS
// array holds the ring offsets of the slice's columns when the tile is windowed, next to the node ids in col (a kernel that
// gathers one matrix from the ring and another one from HBM through the same edges: the source pass).
template <int C, int AUXW, int EXT = 0> struct TileCsr {
    using K = Cfg<C>;
    int* rp; int* col; float* aux; int* ext; int4* metas;
    const int32_t* rowptr_g; const int32_t* col_g; const float* aux_g; const int32_t* ext_g; const int4* meta_g;
    int ebase, n_edges_m1, m_first, m_step, m_ntiles;

    __device__ __forceinline__ void bind(float* lds_after_tiles, const int32_t* rowptr_g_, const int32_t* col_g_, const float* aux_g_,
                                         const int32_t* meta_g_, int n_edges, const int32_t* ext_g_ = nullptr) {
        n_edges_m1 = max(n_edges - 1, 0);
        rp = reinterpret_cast<int*>(lds_after_tiles);
        col = rp + (K::TM + 4);
        aux = reinterpret_cast<float*>(col + K::COLN);
        ext = reinterpret_cast<int*>(aux + AUXW * K::COLN);
        metas = reinterpret_cast<int4*>(ext + (EXT > 0 ? 1 : 0) * K::COLN);
        rowptr_g = rowptr_g_; col_g = col_g_; aux_g = aux_g_; ext_g = ext_g_; meta_g = reinterpret_cast<const int4*>(meta_g_);
    }
    // Metadata of this workgroup's tiles first, first+step, ... -> LDS, once per launch.  Read per tile with
    // meta_at(k): a per-tile global load would be moved to SGPRs by hipcc (v_readfirstlane) and its s_waitcnt,
    // vmcnt being in-order, would also wait for every older load - the GEMM's B fragments.  Caller barriers.
    __device__ __forceinline__ void load_metas(int first, int step, int n_tiles, int tid) {
        metas_commit(metas_issue(first, step, n_tiles, tid), tid);
    }
    // The same in two halves, so a kernel's prologue can put this load in ONE memory round trip with its other first loads
    // (window slabs, weight fragments): request everything, then consume - vmcnt is in-order, the first wait covers all.
    __device__ __forceinline__ int4 metas_issue(int first, int step, int n_tiles, int tid) {
        m_first = first; m_step = step; m_ntiles = n_tiles;
        return meta_g[max(min(first + min(tid, K::MAXM - 1) * step, n_tiles - 1), 0)];   // unconditional (see issue())
    }
    __device__ __forceinline__ void metas_commit(const int4& m, int tid) {
        if (tid < K::MAXM) metas[tid] = m;
    }
    // pure LDS read (the launch grid guarantees at most MAXM tiles per workgroup): a global-load fallback here,
    // even on a never-taken branch, makes hipcc wait vmcnt(0) at the join in every tile
    __device__ __forceinline__ int4 meta_at(int k) const { return metas[min(k, K::MAXM - 1)]; }
    // Staging is split so a kernel can request tile k+1 while it computes tile k: issue() only starts the
    // loads (results stay in registers), commit() writes them to LDS.  Nothing depends on an earlier load
    // except the slice position, which comes from the metadata word read one tile ahead.
    static constexpr int CQ = (K::CAP + GADAPT_MAXD + K::NT - 1) / K::NT;
    struct Regs {
        int4 meta;
        int rpv, rpv2;
        int colv[CQ];
        float auxv[AUXW > 0 ? AUXW * CQ : 1];
        int extv[EXT == 1 ? CQ : 1];
    };
    // Every load here is
    // UNCONDITIONAL with a clamped address (validity is applied in commit): a load under a branch or an exec mask
    // makes hipcc assume the worst at the join and emit s_waitcnt vmcnt(small) later, which drains the whole
    // prefetch right where the B fragments of the GEMM are waited for (vmcnt is in-order).
    // k = index of the tile within this workgroup's sequence (see load_metas)
    __device__ __forceinline__ void issue(Regs& r, int k, int node0, int n_nodes, int tid) const {
        issue_meta(r, meta_at(k), node0, n_nodes, tid);
    }
    // The FIRST tile of a launch.  Its slice position is in the metadata, which the other tiles read from the LDS copy one tile ahead;
    // waiting for that copy made the first tile's slice a second memory round trip of every launch (2.6k of a target launch's 26.6k
    // cycles at one tile per workgroup, docs/measurements.md K).  The tile index is wave-uniform, so its metadata word comes through
    // the SCALAR cache - its own counter (lgkmcnt), not the in-order vector one - and the slice is requested in the SAME round trip as
    // the prologue's slabs and weight fragments.
    // (load and wait are ONE asm statement: the compiler takes an asm's outputs as valid when it ends - with the wait in a second
    // statement it copied the still-unwritten registers in between and the slice was requested from a garbage position: a GPU memory
    // fault.  The wait is short - the scalar cache answers in a few hundred cycles - and the vector loads issued before it are in flight.)
    typedef int i32x4_t __attribute__((ext_vector_type(4)));
    __device__ __forceinline__ int4 meta_scalar(int tile, int n_tiles) const {
        const int4* ptr = meta_g + max(min(tile, n_tiles - 1), 0);
        i32x4_t r;
        asm volatile("s_load_dwordx4 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(r) : "s"(ptr) : "memory");
        return make_int4(r.x, r.y, r.z, r.w);
    }
    __device__ __forceinline__ void issue_meta(Regs& r, const int4& meta, int node0, int n_nodes, int tid) const {
        r.meta = meta;
        const int eb = max(r.meta.x, 0);
        const int nb = min(max(node0, 0), n_nodes);              // a request one tile past either end of the chunk stays in bounds
        r.rpv = rowptr_g[min(nb + min(tid, K::TM), n_nodes)];
        r.rpv2 = (K::TM >= K::NT) ? rowptr_g[min(nb + min(K::NT + tid, K::TM), n_nodes)] : 0;
#pragma unroll
        for (int q = 0; q < CQ; ++q) {
            const int idx = q * K::NT + tid;
            r.colv[q] = col_g[min(eb + idx, n_edges_m1)];
            if constexpr (EXT == 1) r.extv[q] = ext_g[min(eb + idx, n_edges_m1)];
            if constexpr (AUXW > 0) {
#pragma unroll
                for (int w = 0; w < AUXW; ++w) {
                    const int ia = (q * AUXW + w) * K::NT + tid;
                    r.auxv[q * AUXW + w] = aux_g[min((size_t)AUXW * eb + ia, (size_t)AUXW * n_edges_m1 + (AUXW - 1))];
                }
            }
        }
    }
    // Float offset, inside a RING-slab LDS ring, of the row of node j when slabs t-1, t, t+1 are resident
    // (slab s lives in slot s % RING).
    template <int RINGN = K::RING> static __device__ __forceinline__ int ring_off(int j, int t) {
        int slot = (t + RINGN - 1) % RINGN + (j / K::TM - (t - 1));
        if (slot >= RINGN) slot -= RINGN;
        return slot * K::TILE_FLOATS + (j % K::TM) * K::LD;
    }
    // LDS writes of a previously issued tile; returns its row-length bound (-1: slow tile).  Caller barriers.
    // windowed_tile >= 0: the tile's neighbours all live in slabs t-1..t+1 (metadata word 3): store ring offsets
    // instead of node ids so the gathers read LDS directly.
    template <int RINGN = K::RING> __device__ __forceinline__ int commit(const Regs& r, int tid, int node0_pad, int windowed_tile = -1) {
        static_assert(K::TM + 1 <= 2 * K::NT, "rowptr slice: at most 2 entries per thread");
        auto off = [&](int jv) __attribute__((always_inline)) { return ring_off<RINGN>(jv, windowed_tile); };
        ebase = r.meta.x;
        if (tid <= K::TM) rp[tid] = r.rpv;
        if (K::TM >= K::NT && K::NT + tid <= K::TM) rp[K::NT + tid] = r.rpv2;
#pragma unroll
        for (int q = 0; q < CQ; ++q) {
            const int idx = q * K::NT + tid;
            const int cnt = min(r.meta.y, K::CAP);
            const int jv = (idx < cnt) ? r.colv[q] : node0_pad;       // padding entries: a valid node of this tile
            if constexpr (EXT == 2) {
                if (idx < K::CAP + GADAPT_MAXD) { col[idx] = jv; ext[idx] = (windowed_tile >= 0) ? off(jv) : 0; }
            } else {
                if (idx < K::CAP + GADAPT_MAXD) col[idx] = (windowed_tile >= 0) ? off(jv) : jv;
            }
            if constexpr (EXT == 1) { if (idx < K::CAP + GADAPT_MAXD) ext[idx] = r.extv[q]; }
            if constexpr (AUXW > 0) {
#pragma unroll
                for (int w = 0; w < AUXW; ++w) {
                    const int ia = (q * AUXW + w) * K::NT + tid;
                    if (ia < AUXW * (K::CAP + GADAPT_MAXD)) aux[ia] = (ia < AUXW * cnt) ? r.auxv[q * AUXW + w] : 0.f;
                }
            }
        }
        return (r.meta.y > K::CAP || r.meta.z > GADAPT_MAXD) ? -1 : r.meta.z;
    }
};

// Chunk c4 of row `row` of a matrix stored as [N,d] (d <= 4) but read as [N,C] with zeros beyond column d: the top
// layer's upstream gradient (backward of x[:, :dim], GNN.py:299).  Loads are unconditional (see TileCsr::issue).
__device__ __forceinline__ float4 ld_row4_compact(const float* __restrict__ base, int row, int c4, int d) {
    const float* r = base + (size_t)row * d;
    const float v0 = r[0], v1 = r[min(1, d - 1)], v2 = r[min(2, d - 1)], v3 = r[min(3, d - 1)];
    float4 o = make_float4(v0, d > 1 ? v1 : 0.f, d > 2 ? v2 : 0.f, d > 3 ? v3 : 0.f);
    return c4 == 0 ? o : f4zero();
}
// The compact [N,4] layer-0 input assembled on the fly from the caller's node fields instead of read from a matrix (fused training
// step, gadapt_block_forward_loss): row i = [x_comp[i, 0..dim) | f[i] | uu[i] | 0 ...] - the feature concatenation of
// GNN.py:225-239 through the identity (zero-pad) encoder of GNN.py:75-82.  x_comp == nullptr: absent (the matrix is read).
struct FieldSrc { const float* x_comp; const float* f; const float* uu; int dim; };
// Either source of a compact row as FOUR independent 4-byte loads, one per column, from (pointer, row stride, offset) triples fixed
// at kernel entry - the matrix ([N,4]: the same pointer, stride 4, offsets 0..3) and the fields (x_comp columns, then f, then uu;
// columns past the last one masked to zero) run the SAME instruction stream.  A first version branched on the source and on the
// field layout around its loads: correct, but hipcc then cannot count the outstanding loads at the join and waits for nearly all of
// them - in the wide forward that was an s_waitcnt vmcnt(1) in front of the projection, i.e. the whole window prefetch exposed
// (+1.0 us on the head-only launch for ONE extra 8-byte load per node, measured with diagnostic builds: docs/measurements.md K).
struct Cols4 { const float* p[4]; int s[4], o[4], m[4]; };
__device__ __forceinline__ Cols4 make_cols4(const float* base, const FieldSrc& fs) {
    Cols4 c;
    const bool fld = fs.x_comp != nullptr;
    const float* e0 = fs.f ? fs.f : fs.uu;                      // first extra column: f, or uu when there is no f
    const float* e1 = (fs.f && fs.uu) ? fs.uu : nullptr;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool coord = k < fs.dim, x0 = k == fs.dim && e0, x1 = k == fs.dim + 1 && e1;
        c.p[k] = !fld ? base : (coord ? fs.x_comp : (x0 ? e0 : (x1 ? e1 : fs.x_comp)));
        c.s[k] = !fld ? 4 : (coord ? fs.dim : ((x0 || x1) ? 1 : 0));
        c.o[k] = !fld ? k : (coord ? k : 0);
        c.m[k] = (!fld || coord || x0 || x1) ? 1 : 0;
    }
    return c;
}
__device__ __forceinline__ float4 ld_cols4(const Cols4& c, int row) {
    const float v0 = c.p[0][(size_t)row * c.s[0] + c.o[0]], v1 = c.p[1][(size_t)row * c.s[1] + c.o[1]];
    const float v2 = c.p[2][(size_t)row * c.s[2] + c.o[2]], v3 = c.p[3][(size_t)row * c.s[3] + c.o[3]];
    return make_float4(c.m[0] ? v0 : 0.f, c.m[1] ? v1 : 0.f, c.m[2] ? v2 : 0.f, c.m[3] ? v3 : 0.f);
}
// Chunk c4 of row `row` of x: dense [N,C], or (XC) the compact [N,4] whose columns 4.. are zero by construction - the
// output of the identity encoder (zero-pad, GNN.py:75-82) that layer 0 reads without it ever being materialised.
template <int C, bool XC> __device__ __forceinline__ float4 ld_row4x(const float* __restrict__ base, int row, int c4, const Cols4& cx) {
    if constexpr (XC) {
        const float4 t = ld_cols4(cx, row);                        // unconditional (see TileCsr::issue)
        return c4 == 0 ? t : f4zero();
    } else {
        return ld_row4<C>(base, row, c4);
    }
}
// x-tile rows of a tile held in registers between issue and commit (same split as TileCsr)
template <int C> struct TileRows {
    using K = Cfg<C>;
    static constexpr int V = C / 4;
    static constexpr int XQ = (K::TM * V + K::NT - 1) / K::NT;
    float4 v[XQ];
    int node0_;
    // unconditional clamped loads (see TileCsr::issue); rows past N are zeroed at commit
    // NT: non-temporal loads (rows that pass through once, e.g. the target pass's own g rows)
    template <bool NT = false> __device__ __forceinline__ void issue(const float* __restrict__ src, int node0, int n_nodes, int tid) {
        node0_ = node0;
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int idx = min(q * K::NT + tid, K::TM * V - 1), r = idx / V, c4 = idx % V;
            if constexpr (NT) v[q] = ld_row4_nt<C>(src, min(max(node0 + r, 0), n_nodes - 1), c4);
            else v[q] = ld_row4<C>(src, min(max(node0 + r, 0), n_nodes - 1), c4);
        }
    }
    // XC: src is the compact [N,4] matrix (see ld_row4x): one 16-byte load per row (thread t < TM takes row t, in v[0]);
    // commit_sel writes zeros everywhere else
    template <bool XC> __device__ __forceinline__ void issue_sel(const float* __restrict__ src, int node0, int n_nodes, int tid, const Cols4& cx) {
        if constexpr (XC) {
            static_assert(K::TM <= K::NT, "one compact row per thread");
            node0_ = node0;
            v[0] = ld_cols4(cx, min(max(node0 + min(tid, K::TM - 1), 0), n_nodes - 1));
        } else {
            issue(src, node0, n_nodes, tid);
        }
    }
    template <bool XC> __device__ __forceinline__ void commit_sel(float* tile, int n_nodes, int tid) const {
        if constexpr (XC) {
#pragma unroll
            for (int q = 0; q < XQ; ++q) {
                const int idx = q * K::NT + tid, r = idx / V, c4 = idx % V;
                if (idx < K::TM * V && c4 != 0) *reinterpret_cast<float4*>(tile + r * K::LD + 4 * c4) = f4zero();
            }
            if (tid < K::TM)
                *reinterpret_cast<float4*>(tile + tid * K::LD) = (node0_ + tid < n_nodes && node0_ + tid >= 0) ? v[0] : f4zero();
        } else {
            commit(tile, n_nodes, tid);
        }
    }
    // commit() plus a pre-split f16 copy of the rows (layout of lds_put_split) in `ptile`, the row's inverse scale in ptile's
    // first pad column: for a tile whose rows are projected right after staging (forward without the LDS window, hidden 128).
    // A row's V = 32 chunks sit in 32 consecutive threads - half a wave - so its maximum is four DPP steps and one swizzle.
    __device__ __forceinline__ void commit_presplit(float* tile, float* ptile, int n_nodes, int tid) const {
        static_assert(V == 32 && (K::TM * V) % K::NT == 0, "pre-split staging: rows of 32 chunks, whole rows per pass");
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int idx = q * K::NT + tid, r = idx / V, c4 = idx % V;
            const float4 x = (node0_ + r < n_nodes && node0_ + r >= 0) ? v[q] : f4zero();
            *reinterpret_cast<float4*>(tile + r * K::LD + 4 * c4) = x;
            float m = fmaxf(fmaxf(fabsf(x.x), fabsf(x.y)), fmaxf(fabsf(x.z), fabsf(x.w)));
            m = dpp_max<0xB1>(m); m = dpp_max<0x4E>(m); m = dpp_max<0x141>(m); m = dpp_max<0x140>(m);
            m = fmaxf(m, __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, m), 0x401F)));
            const Pow2 s = pow2_scale(m);
            const float t0 = x.x * s.s, t1 = x.y * s.s, t2 = x.z * s.s, t3 = x.w * s.s;
            f16x2 h01, h23, l01, l23;
            h01.x = (_Float16)t0; h01.y = (_Float16)t1; h23.x = (_Float16)t2; h23.y = (_Float16)t3;
            l01.x = (_Float16)(t0 - (float)h01.x); l01.y = (_Float16)(t1 - (float)h01.y);
            l23.x = (_Float16)(t2 - (float)h23.x); l23.y = (_Float16)(t3 - (float)h23.y);
            uint2* grp = reinterpret_cast<uint2*>(ptile + r * K::LD + 8 * (c4 >> 1));
            grp[c4 & 1] = make_uint2(__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h23));
            grp[2 + (c4 & 1)] = make_uint2(__builtin_bit_cast(unsigned, l01), __builtin_bit_cast(unsigned, l23));
            if (c4 == 0) ptile[r * K::LD + C] = s.inv;
        }
    }
    // same for a compact [N,d] source (ld_row4_compact): like the XC form, thread t < TM takes row t (chunk 0, in v[0]) and the
    // commit (commit_sel<true>) writes zeros everywhere else - not XQ chunk loads per thread of which one in V carries data
    __device__ __forceinline__ void issue_compact(const float* __restrict__ src, int d, int node0, int n_nodes, int tid) {
        static_assert(K::TM <= K::NT, "one compact row per thread");
        node0_ = node0;
        v[0] = ld_row4_compact(src, min(max(node0 + min(tid, K::TM - 1), 0), n_nodes - 1), 0, d);
    }
    __device__ __forceinline__ void commit(float* tile, int n_nodes, int tid) const {
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int idx = q * K::NT + tid, r = idx / V, c4 = idx % V;
            if (idx < K::TM * V)
                *reinterpret_cast<float4*>(tile + r * K::LD + 4 * c4) = (node0_ + r < n_nodes && node0_ + r >= 0) ? v[q] : f4zero();
        }
    }
};

// value held for edge `sub` of this lane's node, picked from a group-uniform array (the asm keeps it a
// select chain: hipcc otherwise spills the array to scratch and indexes it)
template <int N> __device__ __forceinline__ float pick(const float (&v)[N], int sub) {
    float r = v[0];
#pragma unroll
    for (int k = 1; k < N; ++k) { r = (sub == k) ? v[k] : r; asm volatile("" : "+v"(r)); }
    return r;
}
// Sum over the node's lanes for N independent values at once, stage by stage, so that consecutive DPP
// instructions are independent (a dependent DPP chain pays 2 wait states per step).
template <int LPN, int N> __device__ __forceinline__ void group_sum_n(float (&v)[N]) {
    if constexpr (LPN >= 2) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = dpp_add<0xB1>(v[k]);
    }
    if constexpr (LPN >= 4) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = dpp_add<0x4E>(v[k]);
    }
    if constexpr (LPN >= 8) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = dpp_add<0x141>(v[k]);
    }
    if constexpr (LPN >= 16) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = dpp_add<0x140>(v[k]);
    }
    if constexpr (LPN >= 32) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v[k]), 0x401F));
    }
}
template <int V> struct IntTag { static constexpr int value = V; };
// Software pipeline over the ITERS node slots of a tile: rows of slot it+1 are requested before slot it
// is consumed.  `before_first` runs after the first request (e.g. the MFMA phase).  The widest row
// bound keeps a single buffer: two would cost a wave of occupancy for every tile shape.
template <int ITERS, typename BufT, bool TWO_BUFFERS = false, typename Fetch, typename Consume, typename Mid>
__device__ __forceinline__ void run_pipeline(Fetch&& fetch, Consume&& consume, Mid&& before_first) {
    if constexpr (sizeof(BufT) <= 128 || TWO_BUFFERS) {         // two buffers only while one stays within 32 VGPRs (or on request)
        BufT b0, b1;
        fetch(b0, 0);
        before_first();
#pragma unroll
        for (int it = 0; it < ITERS; it += 2) {
            if (it + 1 < ITERS) fetch(b1, it + 1);
            __builtin_amdgcn_sched_barrier(0);
            consume(b0, it);
            __builtin_amdgcn_sched_barrier(0);
            if (it + 1 < ITERS) {
                if (it + 2 < ITERS) fetch(b0, it + 2);
                __builtin_amdgcn_sched_barrier(0);
                consume(b1, it + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    } else {
        BufT b0;
        fetch(b0, 0);
        before_first();
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            consume(b0, it);
            __builtin_amdgcn_sched_barrier(0);
            if (it + 1 < ITERS) fetch(b0, it + 1);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}
// Run f with the smallest compiled row-length bound that covers dmax (block-uniform).
template <typename F> __device__ __forceinline__ void dispatch_dmax(int dmax, F&& f) {
    if (dmax <= 2) f(IntTag<2>{});
    else if (dmax <= 6) f(IntTag<6>{});
    else f(IntTag<GADAPT_MAXD>{});
}


// In-kernel phase stamps: diagnostic builds only (-DGADAPT_STAMPS); never compiled into the shipped library.
#ifdef GADAPT_STAMPS
#define GADAPT_STAMP_L(buf, slot_)                                                                 \
    do {                                                                                           \
        if ((buf) && threadIdx.x == 256) {                                                         \
            __builtin_amdgcn_sched_barrier(0);                                                     \
            unsigned long long t_;                                                                 \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");             \
            (buf)[(size_t)blockIdx.x * 32 + (slot_)] = t_;                                         \
            __builtin_amdgcn_sched_barrier(0);                                                     \
        }                                                                                          \
    } while (0)
#define GADAPT_STAMP(buf, slot_)                                                                   \
    do {                                                                                           \
        if ((buf) && threadIdx.x == 0 && (slot_) < 32) {                                           \
            __builtin_amdgcn_sched_barrier(0);                                                     \
            unsigned long long t_;                                                                 \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");             \
            (buf)[(size_t)blockIdx.x * 32 + (slot_)] = t_;                                         \
            __builtin_amdgcn_sched_barrier(0);                                                     \
        }                                                                                          \
    } while (0)
#define GADAPT_STAMP_RT(buf, slot_)                                                                \
    do {                                                                                           \
        if ((buf) && threadIdx.x == 0 && (slot_) < 32) {                                           \
            __builtin_amdgcn_sched_barrier(0);                                                     \
            unsigned long long t_;                                                                 \
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");         \
            (buf)[(size_t)blockIdx.x * 32 + (slot_)] = t_;                                         \
            __builtin_amdgcn_sched_barrier(0);                                                     \
        }                                                                                          \
    } while (0)
#else
#define GADAPT_STAMP(buf, slot_) do { } while (0)
#define GADAPT_STAMP_L(buf, slot_) do { } while (0)
#define GADAPT_STAMP_RT(buf, slot_) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------------
// Per-lane channel vector.  A node's C channels are spread over LPN = C/FPL lanes; a lane owns NV = FPL/4
// float4 chunks: chunk indices sub, sub+LPN, ... so that the LPN lanes of one load instruction read 16*LPN
// contiguous bytes of the row.  FPL = 8 for C >= 32: fewer lanes per node means the per-node scalar work
// (softmax, masks, address arithmetic) and the DPP reduction steps are shared by twice as many nodes per wave.
// ------------------------------------------------------------------------------------------------
template <int NV> struct Vec {
    float4 v[NV];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = f4zero();
    }
};
typedef float pk2f __attribute__((ext_vector_type(2)));
template <int NV> __device__ __forceinline__ float vdot(const Vec<NV>& a, const Vec<NV>& b) {
    // two interleaved partial sums on v_pk_fma_f32 (a scalar fma chain is one instruction per element)
    pk2f s = pk2f{a.v[0].x, a.v[0].y} * pk2f{b.v[0].x, b.v[0].y};
    s += pk2f{a.v[0].z, a.v[0].w} * pk2f{b.v[0].z, b.v[0].w};
#pragma unroll
    for (int i = 1; i < NV; ++i) {
        s += pk2f{a.v[i].x, a.v[i].y} * pk2f{b.v[i].x, b.v[i].y};
        s += pk2f{a.v[i].z, a.v[i].w} * pk2f{b.v[i].z, b.v[i].w};
    }
    return s.x + s.y;
}
template <int NV> __device__ __forceinline__ void vaxpy(Vec<NV>& y, float a, const Vec<NV>& x) {
#pragma unroll
    for (int i = 0; i < NV; ++i) axpy4(y.v[i], a, x.v[i]);
}
template <int C> __device__ __forceinline__ Vec<Cfg<C>::NV> ld_vec(const float* __restrict__ base, int row, int sub) {
    Vec<Cfg<C>::NV> r;
#pragma unroll
    for (int i = 0; i < Cfg<C>::NV; ++i) r.v[i] = ld_row4<C>(base, row, sub + i * Cfg<C>::LPN);
    return r;
}
template <int C, bool XC> __device__ __forceinline__ Vec<Cfg<C>::NV> ld_xsel(const float* __restrict__ base, int row, int sub, const Cols4& cx) {
    Vec<Cfg<C>::NV> r;
#pragma unroll
    for (int i = 0; i < Cfg<C>::NV; ++i) r.v[i] = ld_row4x<C, XC>(base, row, sub + i * Cfg<C>::LPN, cx);
    return r;
}
// Loss fused into the forward launch that writes the head rows x_top4 [N,4] (last layer of a fused training step): the lane that
// holds columns 0..3 of node i also writes seed[i, 0..d) = d loss / d x_top4[i, 0..d) and adds its terms of sum |pred - target|^p
// to a per-lane sum; the workgroup's total goes to partials[blockIdx.x] (fixed order: the loss is bit-reproducible).  F.mse_loss /
// F.l1_loss with reduction 'mean' (run_GNN.py:80-84,106); the seed arithmetic is loss_forward_kernel's (bit-identical gradients).
// target == nullptr: no loss.
struct LossArgs { const float* target; float* seed; float* partials; int d, l1; float inv; };
// target[row, 0..d) (1 <= d <= 4), zero beyond: four unconditional 4-byte loads with clamped column indices (no branch around a
// load: see Cols4).  Kernels that may run without a loss pass some valid matrix and d = 1 (loss_target_base).
__device__ __forceinline__ float4 loss_target4(const float* base, int d, int row) {
    const float* r = base + (size_t)row * d;
    const float t0 = r[0], t1 = r[min(1, d - 1)], t2 = r[min(2, d - 1)], t3 = r[min(3, d - 1)];
    return make_float4(t0, d > 1 ? t1 : 0.f, d > 2 ? t2 : 0.f, d > 3 ? t3 : 0.f);
}
// this node's terms: writes the seed row, returns the updated per-lane sum
__device__ __forceinline__ float loss_node(const LossArgs& L, int row, const float4& pred, const float4& tgt, float lv) {
    const float pv[4] = {pred.x, pred.y, pred.z, pred.w}, tv[4] = {tgt.x, tgt.y, tgt.z, tgt.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < L.d) {
            const float diff = pv[k] - tv[k];
            if (L.l1) { lv += fabsf(diff); L.seed[(size_t)row * L.d + k] = (diff > 0.f ? L.inv : (diff < 0.f ? -L.inv : 0.f)); }
            else      { lv = fmaf(diff, diff, lv); L.seed[(size_t)row * L.d + k] = 2.0f * diff * L.inv; }
        }
    }
    return lv;
}
// per-lane sums -> one partial per WAVE, partials[blockIdx.x * NW + wave]: DPP / lane-swap steps inside the wave (fixed order), no
// LDS, no workgroup barrier (a workgroup-level sum at the end of the launch was two barriers and a dependent store behind six
// ds_bpermute steps: +2 us on the head-only forward launch).  Every wave of the grid calls it exactly once.
__device__ __forceinline__ float wave_sum(float v) {
    v = group_sum<32>(v);                                       // rows of 16 lanes, then xor 16
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));   // xor 32
    return a + b;
}
// Sum over the 64 lanes of the wave for N independent values, result in every lane, in the order of the xor butterfly
//     for (off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
// that the slab partials are defined by - bit for bit, in all 64 lanes - without the LDS crossbar (__shfl_xor lowers to ds_bpermute_b32).
// (wave_sum above adds in ascending order, 1, 2, .., 32: other roundings.)  Stage by stage over the N values, so that an exchange
// is N - 1 instructions away from the one that reads its result:
//     xor 32  v_permlane32_swap_b32 on two copies: lanes 0..31 get own + other, lanes 32..63 other + own (fp32 addition commutes)
//     xor 16  v_permlane16_swap_b32, likewise between rows 2r and 2r + 1
//     xor 8   DPP row_ror:8 - exactly xor 8 inside a row of 16 lanes
//     xor 4   DPP row_ror:4 - lane (i + 4) mod 16 of the row is i ^ 4 or (i ^ 4) ^ 8, which hold the same value after the xor-8 stage
//     xor 2   DPP quad_perm [2,3,0,1]
//     xor 1   DPP quad_perm [1,0,3,2]
// (row_half_mirror / row_mirror, group_sum's steps, pair other lanes: valid in ascending order only.)
// CONTRACT: every lane of the wave is active (no early return, no divergent branch around the call): a swap or a DPP read of an
// inactive lane has no defined value.  The swaps are inline assembly, so their wait states are in the string: s_nop 1 covers a
// vector write of either operand within the two instructions before (a single value; N >= 3 separates them by itself).
template <int N> __device__ __forceinline__ void wave_sum_desc(float (&v)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        float a = v[k], b = v[k];
        asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));   // xor 32
        v[k] = a + b;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        float a = v[k], b = v[k];
        asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));   // xor 16
        v[k] = a + b;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = dpp_add<0x128>(v[k]);    // row_ror:8
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = dpp_add<0x124>(v[k]);    // row_ror:4
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = dpp_add<0x4E>(v[k]);     // quad_perm [2,3,0,1]
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = dpp_add<0xB1>(v[k]);     // quad_perm [1,0,3,2]
}
// The same sums for the 20 slab partials with each total in ONE lane: the partner of every level (32, 16, 8, 4, 2, 1) and the addition
// tree of every value are wave_sum_desc's, so the bits are (fp32 addition commutes; a NaN's payload is not pinned), but an exchange hands
// over half of the values instead of all of them - the lane and its partner each keep the sum of one value and drop the other's:
//     xor 32  v_permlane32_swap_b32 on the pair (e, e + 10): lanes 0..31 go on with entries 0..9, lanes 32..63 with 10..19   20 -> 10
//     xor 16  v_permlane16_swap_b32 on the pair (e, e + 5): even rows go on with the lower five, odd rows with the upper     10 -> 5
//     xor 8   two row_ror:8 adds into one register, banks 0, 1 from the first of a pair and banks 2, 3 from the second; the
//             fifth register is summed whole (both halves of the row then hold its sum)                                       5 -> 3
//     xor 4   row_shl:4 into banks 0, 2 and row_shr:4 into banks 1, 3 (lane i ^ 4 itself: the halves of a row now differ);
//             the fifth register still takes row_ror:4 whole, as in wave_sum_desc                                             3 -> 2
//     xor 2, xor 1  quad_perm on both registers (a quad has no write mask of its own: halving would cost a select per value)
// 42 vector instructions where wave_sum_desc on 20 values is 240.  lane: the lane's index in the wave.  Returns the total of entry wave_sum_scatter_entry(lane) in the
// lanes for which that is >= 0 (20 lanes, each entry once) and something else in the other 44.
// CONTRACT: wave_sum_desc's - every lane of the wave is active.  The masked DPP adds are inline assembly like the swaps: the wait
// states of a DPP or swap operand written by the instruction before are in the strings (s_nop 1), also behind the last string, whose
// results the compiler's own DPP adds read next.
__device__ __forceinline__ int wave_sum_scatter_entry(int lane) {
    const int base = 10 * (lane >> 5) + 5 * ((lane >> 4) & 1), c = lane & 15, b = c >> 2;
    if (c == 1) return base + 4;                                 // the fifth register: every lane of the row has it, lane 1 of the row hands it in
    if (c & 3) return -1;
    return base + 2 * (b & 1) + (b >> 1);                        // banks 0, 1, 2, 3 of the row: entries 0, 2, 1, 3 of its five
}
__device__ __forceinline__ float wave_sum_scatter(float (&v)[20], int lane) {
#pragma unroll
    for (int g = 0; g < 10; g += 5) {
        asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %5\n\tv_permlane32_swap_b32 %1, %6\n\tv_permlane32_swap_b32 %2, %7\n\t"
                     "v_permlane32_swap_b32 %3, %8\n\tv_permlane32_swap_b32 %4, %9"
                     : "+v"(v[g]), "+v"(v[g + 1]), "+v"(v[g + 2]), "+v"(v[g + 3]), "+v"(v[g + 4]),
                       "+v"(v[g + 10]), "+v"(v[g + 11]), "+v"(v[g + 12]), "+v"(v[g + 13]), "+v"(v[g + 14]));   // xor 32
#pragma unroll
        for (int e = g; e < g + 5; ++e) v[e] = v[e] + v[e + 10];
    }
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %5\n\tv_permlane16_swap_b32 %1, %6\n\tv_permlane16_swap_b32 %2, %7\n\t"
                 "v_permlane16_swap_b32 %3, %8\n\tv_permlane16_swap_b32 %4, %9"
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]), "+v"(v[8]), "+v"(v[9]));   // xor 16
#pragma unroll
    for (int e = 0; e < 5; ++e) v[e] = v[e] + v[e + 5];
    float s0, s1, t0;
    asm volatile("s_nop 1\n\t"
                 "v_add_f32_dpp %0, %2, %2 row_ror:8 row_mask:0xf bank_mask:0x3\n\tv_add_f32_dpp %0, %3, %3 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
                 "v_add_f32_dpp %1, %4, %4 row_ror:8 row_mask:0xf bank_mask:0x3\n\tv_add_f32_dpp %1, %5, %5 row_ror:8 row_mask:0xf bank_mask:0xc"
                 : "=&v"(s0), "=&v"(s1) : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]));                                          // xor 8
    float t1 = dpp_add<0x128>(v[4]);
    asm volatile("s_nop 1\n\t"
                 "v_add_f32_dpp %0, %1, %1 row_shl:4 row_mask:0xf bank_mask:0x5\n\tv_add_f32_dpp %0, %2, %2 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
                 "s_nop 1"
                 : "=&v"(t0) : "v"(s0), "v"(s1));                                                                                  // xor 4
    t1 = dpp_add<0x124>(t1);
    t0 = dpp_add<0x4E>(t0); t1 = dpp_add<0x4E>(t1);             // xor 2
    t0 = dpp_add<0xB1>(t0); t1 = dpp_add<0xB1>(t1);             // xor 1
    return (lane & 15) == 1 ? t1 : t0;
}
template <int NW> __device__ __forceinline__ void loss_wave_partial(const LossArgs& L, float lv, int tid) {
    const float t = wave_sum(lv);
    if ((tid & 63) == 0) L.partials[blockIdx.x * NW + (tid >> 6)] = t;
}
template <int C> __device__ __forceinline__ void st_vec(float* __restrict__ base, int row, int sub, const Vec<Cfg<C>::NV>& x) {
#pragma unroll
    for (int i = 0; i < Cfg<C>::NV; ++i) st_row4<C>(base, row, sub + i * Cfg<C>::LPN, x.v[i]);
}
// padded LDS tile [TM][LD]
template <int C> __device__ __forceinline__ Vec<Cfg<C>::NV> lds_vec(const float* tile, int li, int sub) {
    Vec<Cfg<C>::NV> r;
#pragma unroll
    for (int i = 0; i < Cfg<C>::NV; ++i) r.v[i] = *reinterpret_cast<const float4*>(tile + li * Cfg<C>::LD + 4 * (sub + i * Cfg<C>::LPN));
    return r;
}
template <int C> __device__ __forceinline__ void lds_put(float* tile, int li, int sub, const Vec<Cfg<C>::NV>& x) {
#pragma unroll
    for (int i = 0; i < Cfg<C>::NV; ++i) *reinterpret_cast<float4*>(tile + li * Cfg<C>::LD + 4 * (sub + i * Cfg<C>::LPN)) = x.v[i];
}
// Maximum over the LPN lanes that share a node (non-negative values), in every lane: the DPP steps of group_sum.
template <int LPN> __device__ __forceinline__ float group_max(float v) {
    if constexpr (LPN >= 2) v = dpp_max<0xB1>(v);
    if constexpr (LPN >= 4) v = dpp_max<0x4E>(v);
    if constexpr (LPN >= 8) v = dpp_max<0x141>(v);
    if constexpr (LPN >= 16) v = dpp_max<0x140>(v);
    static_assert(LPN <= 16, "group_max: lane groups of at most one DPP row");
    return v;
}
// A row's channels of this lane -> the pre-split f16 layout of the row in an LDS tile (see the PRE-SPLIT note above): chunk c (4
// channels) is half c & 1 of k-group c >> 1, whose 32 bytes hold 8 h pieces then 8 l pieces.  Returns the row's inverse scale.
template <int C> __device__ __forceinline__ float lds_put_split(float* tile, int li, int sub, const Vec<Cfg<C>::NV>& x) {
    using K = Cfg<C>;
    float m = 0.f;
#pragma unroll
    for (int q = 0; q < K::NV; ++q) m = fmaxf(fmaxf(fmaxf(m, fabsf(x.v[q].x)), fabsf(x.v[q].y)), fmaxf(fabsf(x.v[q].z), fabsf(x.v[q].w)));
    const Pow2 s = pow2_scale(group_max<K::LPN>(m));
#pragma unroll
    for (int q = 0; q < K::NV; ++q) {
        const int c = sub + q * K::LPN;
        const float t0 = x.v[q].x * s.s, t1 = x.v[q].y * s.s, t2 = x.v[q].z * s.s, t3 = x.v[q].w * s.s;
        f16x2 h01, h23, l01, l23;
        h01.x = (_Float16)t0; h01.y = (_Float16)t1; h23.x = (_Float16)t2; h23.y = (_Float16)t3;
        l01.x = (_Float16)(t0 - (float)h01.x); l01.y = (_Float16)(t1 - (float)h01.y);
        l23.x = (_Float16)(t2 - (float)h23.x); l23.y = (_Float16)(t3 - (float)h23.y);
        uint2* grp = reinterpret_cast<uint2*>(tile + li * K::LD + 8 * (c >> 1));
        grp[c & 1] = make_uint2(__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h23));
        grp[2 + (c & 1)] = make_uint2(__builtin_bit_cast(unsigned, l01), __builtin_bit_cast(unsigned, l23));
    }
    return s.inv;
}


