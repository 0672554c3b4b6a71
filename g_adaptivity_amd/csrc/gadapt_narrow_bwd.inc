// gadapt_narrow_bwd.inc - fused backward launch of the narrow route (gadapt_block_backward_narrow), included by gadapt_tu_bwd_target.hip
// after gadapt_bwd_target.inc (gfx950 only; see gadapt_internal.h for the translation units).
//
// On the narrow route the target pass of layer l-1 reads, of the upstream gradient, only its own row g_i - and the source pass of layer
// l produces exactly that row, one node per lane.  grand_bwd_target_fused_narrow_kernel runs source(l) and target(l-1) of a node in ONE
// lane: grand_bwd_source_narrow_kernel's arithmetic (same expressions, same order), then bwd_target_compact_body with g_i still in
// registers.  The four dependent memory round trips of the two launches become two: the source half's (row bounds, ELL row, dxd row)
// goes out with the target half's (row bounds, ELL row, x row), and its ({alpha dt, ds} pairs, g rows, x rows) with the target half's
// (alpha, tpos, neighbour x rows).  The backward of an L-layer block is then T_{L-1}, [S_{L-1}+T_{L-2}], ..., [S_1+T_0]: L launches
// instead of 2L - 1.  Results are bit-identical with the pair of launches (tests/test_gpu_narrow_backward.py).
//
// What lanes of one launch share, and why it is safe:
//   - the {alpha dt, ds} pairs: while some lanes still read layer l's pairs in source order, others already scatter layer l-1's
//     through tpos into other nodes' rows.  With one buffer that is a race, so the launches ALTERNATE between two edge buffers
//     (edge_in is read, edge_out written; gadapt_block_backward_narrow carves the second one out of the unused tail of dxd_ws);
//   - dxd[j] is read (layer l's row) and then written (layer l-1's row) by the same lane, and no other lane touches it;
//   - g rows: the launch reads the neighbours' rows of layer l's upstream gradient from one half of g_ws and writes its own row of
//     layer l's result to the other half - the halves alternate from launch to launch as they do for the pair.
//
// L0 = false: the target half is the NARROW form (dxd, the pairs through tpos, the 20 slab partials) and g_out is stored for the
// next launch's neighbours.  L0 = true: the target half is layer 0 (partials only); nothing reads layer 1's result but the lane that
// computed it, so g_out is not stored.
// GC: the source half's upstream gradient is the compact [N,g_cols] top gradient (the first fused launch of a block, whose source
// half belongs to the top layer), else [N,4].
// Registers: 190 - 205, no scratch (two waves per SIMD, which is what the 512-workgroup grid puts there).

// Source half: grand_bwd_source_narrow_kernel's per-node work, split at its two round trips.
template <bool L0, bool GC>
struct FusedNarrowSource {
    static constexpr bool FUSED = true;
    const float* x_in; const float* g_in; const float2* ew; const float* dxd;
    const int32_t* rowptr; const int32_t* col; const int32_t* ell;
    float* g_out;
    int n_edges, g_cols;
    float a4[4][4];                                             // A[c][o], c, o < 4 (this layer's: the one ABOVE the target half's)
    float4 p04;
    struct Regs {
        int e0, deg;
        int4 el0, el1;
        float4 d4;
        float2 ev[8]; float4 gk[8], xk[8];
    };
    __device__ __forceinline__ float4 ld_g4(int i) const {
        if constexpr (GC) return ld_row4_compact(g_in, i, 0, g_cols); else return *reinterpret_cast<const float4*>(g_in + 4 * (size_t)i);
    }
    __device__ __forceinline__ void issue1(Regs& r, int64_t j) const {
        r.e0 = rowptr[j]; r.deg = rowptr[j + 1] - r.e0;
        r.el0 = *reinterpret_cast<const int4*>(ell + 8 * (size_t)j); r.el1 = *reinterpret_cast<const int4*>(ell + 8 * (size_t)j + 4);
        r.d4 = *reinterpret_cast<const float4*>(dxd + 4 * (size_t)j);
    }
    __device__ __forceinline__ void issue2(Regs& r) const {     // (n_edges > 0: an edgeless graph has no pair to clamp to)
        const int last = n_edges - 1;
        const int ej[8] = {r.el0.x, r.el0.y, r.el0.z, r.el0.w, r.el1.x, r.el1.y, r.el1.z, r.el1.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {                            // unconditional, clamped: weight 0 past the row end
            const int i = max(ej[k], 0);
            r.ev[k] = ew[min(r.e0 + k, last)];
            r.gk[k] = ld_g4(i);
            r.xk[k] = *reinterpret_cast<const float4*>(x_in + 4 * (size_t)i);
        }
    }
    __device__ __forceinline__ float4 finish(const Regs& r, int64_t j) const {
        float4 z4 = f4zero(), y = f4zero();
        float sig = 0.f;
        if (r.deg <= 8 && n_edges > 0) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float2 e = k < r.deg ? r.ev[k] : make_float2(0.f, 0.f);
                axpy4(z4, e.x, r.gk[k]); axpy4(y, e.y, r.xk[k]); sig += e.y;
            }
        } else {
            for (int e = r.e0; e < r.e0 + r.deg; ++e) {
                const int i = col[e];
                const float2 ev = ew[e];
                axpy4(z4, ev.x, ld_g4(i)); axpy4(y, ev.y, *reinterpret_cast<const float4*>(x_in + 4 * (size_t)i)); sig += ev.y;
            }
        }
        const float yv[4] = {y.x, y.y, y.z, y.w};
        float t4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int c = 0; c < 4; ++c) t4[c] = fmaf(yv[o], a4[c][o], t4[c]);
        const float4 d4 = r.d4;
        const float4 g = make_float4(d4.x + z4.x + t4[0] + sig * p04.x, d4.y + z4.y + t4[1] + sig * p04.y,
                                     d4.z + z4.z + t4[2] + sig * p04.z, d4.w + z4.w + t4[3] + sig * p04.w);
        if constexpr (!L0) *reinterpret_cast<float4*>(g_out + 4 * (size_t)j) = g;
        return g;
    }
};

// Arguments of the fused launch: t = the target half (layer l-1; t.g_in unused, t.edge_ws = the buffer this launch WRITES), the rest =
// the source half (layer l; edge_in = the buffer the launch above wrote).
struct BwdFusedNarrowArgs {
    BwdTArgs t;
    const float* x_src; const float* g_in; const float* edge_in; const float* A_src; const float* p0_src;
    const int32_t* rowptr_s; const int32_t* col_s; const int32_t* ell_s;
    float* g_out;
    int g_cols;                                                 // GC: columns of g_in
};

template <bool L0, bool GC>
__global__ __launch_bounds__(256) void grand_bwd_target_fused_narrow_kernel(BwdFusedNarrowArgs p) {
    FusedNarrowSource<L0, GC> src;
    src.x_in = p.x_src; src.g_in = p.g_in; src.ew = reinterpret_cast<const float2*>(p.edge_in); src.dxd = p.t.dxd;
    src.rowptr = p.rowptr_s; src.col = p.col_s; src.ell = p.ell_s;
    src.g_out = p.g_out;
    src.n_edges = p.t.n_edges; src.g_cols = p.g_cols;
    const int C = p.t.c;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int o = 0; o < 4; ++o) src.a4[c][o] = p.A_src[c * C + o];
    src.p04 = *reinterpret_cast<const float4*>(p.p0_src);
    bwd_target_compact_body<0, true, !L0, FusedNarrowSource<L0, GC>>(p.t, src);
}
