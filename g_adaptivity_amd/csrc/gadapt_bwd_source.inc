// gadapt_bwd_source.inc - backward source pass grand_bwd_source_kernel<C,...> and its 4-column form (g_out = dxd + sum over out-edges) (gfx950 only; see gadapt_internal.h for the translation units).

// ------------------------------------------------------------------------------------------------
// backward, source pass
// ------------------------------------------------------------------------------------------------
struct BwdSArgs {
    const float* x_in; const float* g_in; const float* edge_ws; const float* dxd;
    const float* A; const float* p0;
    const int32_t* rowptr; const int32_t* col; const int32_t* meta;
    float* g_out;
    int n_nodes, n_tiles, n_edges;
    unsigned long long* stamps;
    int g_cols;                                                 // GC kernels: g_in is [N,g_cols]
    int c;                                                      // hidden size (read by grand_bwd_source_narrow_kernel only) ...
    const int32_t* ell;                                         // ... and the graph's ELL table of out-neighbours (gadapt_graph::ell_s)
};

// Half of one node's out-edge rows: g_i and x_i of HN targets (two halves cover DM edges)
template <int HN_, int NV> struct SBuf {
    static constexpr int N = HN_;
    Vec<NV> g[HN_], x[HN_];
    float2 ev[HN_];
};

// One node's out-edge rows of g (windowed source pass: the x rows come from the LDS ring)
template <int DM_, int NV> struct SBufG {
    static constexpr int N = DM_;
    Vec<NV> g[DM_];
    float2 ev[DM_];
    int e0;
};

// WIN: rolling LDS window of x rows like the target pass (slabs t-1, t, t+1; a workgroup walks consecutive tiles): on
// mesh-ordered graphs the x_i gathers of the out-edge walk are LDS reads and only the g_i rows go through L1 / L2 - the walk is
// bound by the 64 bytes per clock of the CU's vector-memory path (512 B per edge), which this halves.  The projection then
// runs in place in the y tile (window + two tiles would leave one workgroup per CU).
template <int C, bool GC = false, bool WIN = false>
__global__ __launch_bounds__(Cfg<C>::NT, (C >= GADAPT_ONE_WAVE_C ? 1 : GADAPT_WAVES_BWD_S)) void grand_bwd_source_kernel(BwdSArgs p) {
    using K = Cfg<C>;
    using V = Vec<K::NV>;
    static_assert(!WIN || K::MFMA, "windowed source pass: matrix-core sizes");
    extern __shared__ float4 smem4[];
    float* ring = reinterpret_cast<float*>(smem4);              // WIN: three slabs of x rows
    float* ys = ring + (WIN ? 3 * K::TILE_FLOATS : 0);
    float* os = WIN ? ys : ys + K::TILE_FLOATS;
    using CsrT = TileCsr<C, 2, WIN ? 2 : 0>;                    // aux = {alpha*dt, d<P,x>} per out-edge (source order); WIN: ext = ring offsets
    CsrT csr;
    csr.bind(os + K::TILE_FLOATS, p.rowptr, p.col, p.edge_ws, p.meta, p.n_edges);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = tid / K::LPN, sub = tid % K::LPN;

    // row i of the upstream gradient, this lane's chunks (GC: compact [N,g_cols] source)
    auto ld_g = [&](int i) __attribute__((always_inline)) {
        if constexpr (GC) {
            V r;
            r.v[0] = ld_row4_compact(p.g_in, i, sub, p.g_cols);  // chunk `sub` of the row: data in chunk 0 only, zeros elsewhere
#pragma unroll
            for (int q = 1; q < K::NV; ++q) r.v[q] = f4zero();   // chunks sub + q LPN > 0: no load
            return r;
        } else {
            return ld_vec<C>(p.g_in, i, sub);
        }
    };
    // PRE: the y tile is written in the pre-split f16 form by the lanes that sum its rows (lds_put_split); yinv = row scales
    constexpr bool PRE = K::MFMA && TileGemm<C, false>::SPLIT;
    float yinv[K::ITERS];
    TileGemm<C, false, true> gemm;            // os = y A^T
    float arow[K::MFMA ? 1 : 4][K::MFMA ? 1 : C];
    if constexpr (K::MFMA) {
        gemm.init(lane, wave);
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int c = 0; c < C; ++c) arow[t][c] = p.A[(4 * sub + t) * C + c];
    }
    V p0v;
#pragma unroll
    for (int q = 0; q < K::NV; ++q) p0v.v[q] = *reinterpret_cast<const float4*>(p.p0 + 4 * (sub + q * K::LPN));

    // split fragments: built once per launch
    constexpr bool RESIDENT_B = K::MFMA;                          // split fragments: built once per launch
    // this workgroup's tiles: every step-th one (XCD-interleaved), or - WIN - a run of consecutive ones
    // (tb, stp, n_my): first tile, stride, count.  (WIN: walking every other workgroup's run backwards, as the target pass
    // does, was measured at hidden 128: 70.5 -> 72.1 us - the rows this pass shares between workgroups are gathered g rows, not
    // halo slabs.)
    int tb, stp, n_my;
    if constexpr (WIN) {
        const TileChunk ch = tile_chunk(p.n_tiles);
        stp = 1;
        tb = ch.t0;
        n_my = max(ch.t1 - ch.t0, 0);
    } else {
        const TileRange tr = tile_range(p.n_tiles);
        tb = tr.t; stp = tr.step;
        n_my = tr.t < tr.t_end ? (tr.t_end - tr.t + tr.step - 1) / tr.step : 0;
    }
    typename CsrT::Regs sr;
    auto slab_ptr = [&](int s_) __attribute__((always_inline)) { return ring + ((s_ + 3) % 3) * K::TILE_FLOATS; };
    TileRows<C> xr;
    // prologue loads in ONE memory round trip (see the target pass): tile metadata, weight fragments, the window's first slabs (WIN) and -
    // its metadata word through the scalar cache (TileCsr::meta_scalar) - the first tile's CSR slice.  Unconditional, clamped: a
    // workgroup without tiles requests the last tile's and ignores it.
    typename decltype(gemm)::BRaw braw;
    if constexpr (RESIDENT_B) gemm.load_issue(p.A, nullptr, braw);   // the weight rows first (see the target pass)
    if constexpr (WIN) {
        TileRows<C> xr2, xr3;
        xr.template issue<true>(p.x_in, (tb - stp) * K::TM, p.n_nodes, tid);
        xr2.template issue<true>(p.x_in, tb * K::TM, p.n_nodes, tid);
        const int4 mreg = csr.metas_issue(tb, stp, p.n_tiles, tid);
        xr3.template issue<true>(p.x_in, (tb + stp) * K::TM, p.n_nodes, tid);
        const int4 m0 = csr.meta_scalar(tb, p.n_tiles);           // (behind the vector requests above: see TileCsr::meta_scalar)
        csr.issue_meta(sr, m0, min(tb, p.n_tiles - 1) * K::TM, p.n_nodes, tid);
        if constexpr (RESIDENT_B) gemm.load_finish(braw);
        csr.metas_commit(mreg, tid);
        xr.commit(slab_ptr(tb - stp), p.n_nodes, tid);
        xr2.commit(slab_ptr(tb), p.n_nodes, tid);
        xr = xr3;
    } else {
        const int4 mreg = csr.metas_issue(tb, stp, p.n_tiles, tid);
        const int4 m0 = csr.meta_scalar(tb, p.n_tiles);           // (behind the vector requests above: see TileCsr::meta_scalar)
        csr.issue_meta(sr, m0, min(tb, p.n_tiles - 1) * K::TM, p.n_nodes, tid);
        if constexpr (RESIDENT_B) gemm.load_finish(braw);
        csr.metas_commit(mreg, tid);
    }
    __syncthreads();
    int kt = 0;                                                 // index of the tile in this workgroup's sequence
    V zr[K::ITERS];                                             // sum(alpha dt g_i) + sigma p0, kept across the GEMM; then the result rows
    // g_out rows of a finished tile leave the registers only after the NEXT tile's staging (see the target pass)
    auto store_out = [&](int node0) __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < K::ITERS; ++it) {
            const int j = node0 + it * K::SLOTS + slot;
            if (j < p.n_nodes) {
                if constexpr (WIN) {
#pragma unroll
                    for (int q = 0; q < K::NV; ++q) st_row4_nt<C>(p.g_out, j, sub + q * K::LPN, zr[it].v[q]);
                } else {
                    st_vec<C>(p.g_out, j, sub, zr[it]);
                }
            }
        }
    };
    int prev_node0 = -1;
    for (int k = 0; k < n_my; ++k) {
        const int t = tb + k * stp;
        const int node0 = t * K::TM;
        const int tslot = k * 8;
        GADAPT_STAMP(p.stamps, tslot + 0);
        const bool win = WIN && (sr.meta.w & 1) != 0;
        if constexpr (WIN) xr.commit(slab_ptr(t + stp), p.n_nodes, tid);
        const int dmax = WIN ? csr.template commit<3>(sr, tid, node0, win ? t : -1) : csr.commit(sr, tid, node0);
        __syncthreads();
        if (prev_node0 >= 0) store_out(prev_node0);
        prev_node0 = node0;
        {   // request the next tile now (unconditional, clamped past the end: see issue()): it lands during this one
            csr.issue(sr, ++kt, (t + stp) * K::TM, p.n_nodes, tid);
        }
        GADAPT_STAMP(p.stamps, tslot + 1);
        if (dmax >= 0) {
            dispatch_dmax(dmax, [&](auto tag) {
                constexpr int DM = decltype(tag)::value;
                constexpr int HN = (DM + 1) / 2;
                // pipeline steps = (node slot, half): rows of the next half are requested before this one is summed
                auto fetch_w = [&](SBuf<HN, K::NV>& b, int step, auto win_tag) __attribute__((always_inline)) {
                    const int it = step >> 1, half = step & 1;
                    const int li = it * K::SLOTS + slot;
                    const int e0 = csr.rp[li] - csr.ebase + half * HN;
                    const int deg = (node0 + li < p.n_nodes) ? csr.rp[li + 1] - csr.rp[li] : 0;
#pragma unroll
                    for (int k = 0; k < HN; ++k) {
                        const int i = csr.col[e0 + k];               // past the row end: some valid row, weight 0
                        b.ev[k] = *reinterpret_cast<const float2*>(csr.aux + 2 * (e0 + k));
                        if (half * HN + k >= deg) b.ev[k] = make_float2(0.f, 0.f);
                        b.g[k] = ld_g(i);
                        if constexpr (decltype(win_tag)::value != 0) {
                            const float* row = ring + csr.ext[e0 + k];
#pragma unroll
                            for (int q = 0; q < K::NV; ++q) b.x[k].v[q] = *reinterpret_cast<const float4*>(row + 4 * (sub + q * K::LPN));
                        } else {
                            b.x[k] = ld_vec<C>(p.x_in, i, sub);
                        }
                    }
                };
                V z, y; float sig = 0.f;
                auto consume = [&](const SBuf<HN, K::NV>& b, int step) __attribute__((always_inline)) {
                    const int it = step >> 1, half = step & 1;
                    if (half == 0) { z.zero(); y.zero(); sig = 0.f; }
#pragma unroll
                    for (int k = 0; k < HN; ++k) { vaxpy(z, b.ev[k].x, b.g[k]); vaxpy(y, b.ev[k].y, b.x[k]); sig += b.ev[k].y; }
                    if (half == 1) {
                        const int li = it * K::SLOTS + slot;
                        if constexpr (PRE) yinv[it] = lds_put_split<C>(ys, li, sub, y); else lds_put<C>(ys, li, sub, y);
                        vaxpy(z, sig, p0v);
                        zr[it] = z;
                    }
                };
                if constexpr (WIN) {
                    if (win) {
                        // windowed tile: the buffer holds g rows only (x rows are LDS reads at the point of use), so one request
                        // covers a whole node - half as many exposed round trips per tile as the two-matrix half-node steps
                        auto fetch_n = [&](SBufG<DM, K::NV>& b, int it) __attribute__((always_inline)) {
                            const int li = it * K::SLOTS + slot;
                            const int e0 = csr.rp[li] - csr.ebase;
                            const int deg = (node0 + li < p.n_nodes) ? csr.rp[li + 1] - csr.rp[li] : 0;
                            b.e0 = e0;
#pragma unroll
                            for (int k = 0; k < DM; ++k) {
                                const int i = csr.col[e0 + k];
                                b.ev[k] = *reinterpret_cast<const float2*>(csr.aux + 2 * (e0 + k));
                                if (k >= deg) b.ev[k] = make_float2(0.f, 0.f);
                                b.g[k] = ld_g(i);
                            }
                        };
                        auto consume_n = [&](const SBufG<DM, K::NV>& b, int it) __attribute__((always_inline)) {
                            V zz, yy; zz.zero(); yy.zero();
                            float sg = 0.f;
#pragma unroll
                            for (int k = 0; k < DM; ++k) {
                                const float* row = ring + csr.ext[b.e0 + k];
                                V xv;
#pragma unroll
                                for (int q = 0; q < K::NV; ++q) xv.v[q] = *reinterpret_cast<const float4*>(row + 4 * (sub + q * K::LPN));
                                vaxpy(zz, b.ev[k].x, b.g[k]); vaxpy(yy, b.ev[k].y, xv); sg += b.ev[k].y;
                            }
                            const int li = it * K::SLOTS + slot;
                            if constexpr (PRE) yinv[it] = lds_put_split<C>(ys, li, sub, yy); else lds_put<C>(ys, li, sub, yy);
                            vaxpy(zz, sg, p0v);
                            zr[it] = zz;
                        };
                        run_pipeline<K::ITERS, SBufG<DM, K::NV>>(fetch_n, consume_n, [&]() {});
                    } else {
                        run_pipeline<2 * K::ITERS, SBuf<HN, K::NV>>([&](auto& b, int step) { fetch_w(b, step, IntTag<0>{}); }, consume, [&]() {});
                    }
                } else {
                    run_pipeline<2 * K::ITERS, SBuf<HN, K::NV>>([&](auto& b, int step) { fetch_w(b, step, IntTag<0>{}); }, consume, [&]() {});
                }
            });
        } else {
#pragma unroll
            for (int it = 0; it < K::ITERS; ++it) {              // any row length, CSR straight from HBM
                const int li = it * K::SLOTS + slot;
                const int j = node0 + li;
                V z, y; z.zero(); y.zero();
                float sig = 0.f;
                if (j < p.n_nodes) {
                    const int e0 = p.rowptr[j], deg = p.rowptr[j + 1] - e0;
                    for (int k = 0; k < deg; ++k) {
                        const int i = p.col[e0 + k];
                        const float2 ev = *reinterpret_cast<const float2*>(p.edge_ws + 2 * (size_t)(e0 + k));
                        vaxpy(z, ev.x, ld_g(i));
                        vaxpy(y, ev.y, ld_vec<C>(p.x_in, i, sub));
                        sig += ev.y;
                    }
                }
                if constexpr (PRE) yinv[it] = lds_put_split<C>(ys, li, sub, y); else lds_put<C>(ys, li, sub, y);
                vaxpy(z, sig, p0v);
                zr[it] = z;
            }
        }
        GADAPT_STAMP(p.stamps, tslot + 2);
        if constexpr (WIN) xr.template issue<true>(p.x_in, (t + 2 * stp) * K::TM, p.n_nodes, tid);   // slab of the next tile's window (clamped past the end)
        V dpre[K::ITERS];                                       // own dxd rows: requested here, used after the GEMM
#pragma unroll
        for (int it = 0; it < K::ITERS; ++it) {
            const int jr = min(node0 + it * K::SLOTS + slot, p.n_nodes - 1);
            if constexpr (WIN) {
#pragma unroll
                for (int q = 0; q < K::NV; ++q) dpre[it].v[q] = ld_row4_nt<C>(p.dxd, jr, sub + q * K::LPN);
            } else {
                dpre[it] = ld_vec<C>(p.dxd, jr, sub);
            }
        }
        __syncthreads();
        GADAPT_STAMP(p.stamps, tslot + 3);
        if constexpr (K::MFMA) {
            if constexpr (PRE) {
                f32x16 acc[decltype(gemm)::BPW];
                gemm.accumulate_presplit(ys, acc);
                if constexpr (WIN) __syncthreads();             // in place: every wave has read its operand rows
                gemm.store_presplit(os, acc);
            } else if constexpr (WIN) {
                gemm.run_in_place(ys);
            } else {
                gemm.run(ys, os);
            }
            __syncthreads();
        }
        GADAPT_STAMP(p.stamps, tslot + 4);
#pragma unroll
        for (int it = 0; it < K::ITERS; ++it) {
            const int li = it * K::SLOTS + slot;
            const int j = node0 + li;
            if (j >= p.n_nodes) continue;
            V r;
            if constexpr (K::MFMA) {
                r = lds_vec<C>(os, li, sub);
            } else {
                r.zero();
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float yc = ys[li * K::LD + c];
                    r.v[0].x = fmaf(arow[0][c], yc, r.v[0].x); r.v[0].y = fmaf(arow[1][c], yc, r.v[0].y);
                    r.v[0].z = fmaf(arow[2][c], yc, r.v[0].z); r.v[0].w = fmaf(arow[3][c], yc, r.v[0].w);
                }
            }
            const V d = dpre[it];
            const float ri = PRE ? yinv[it] : 1.0f;             // pre-split operand: the row's inverse scale (1: exact either way)
#pragma unroll
            for (int q = 0; q < K::NV; ++q) {
                zr[it].v[q].x = fmaf(r.v[q].x, ri, zr[it].v[q].x) + d.v[q].x; zr[it].v[q].y = fmaf(r.v[q].y, ri, zr[it].v[q].y) + d.v[q].y;
                zr[it].v[q].z = fmaf(r.v[q].z, ri, zr[it].v[q].z) + d.v[q].z; zr[it].v[q].w = fmaf(r.v[q].w, ri, zr[it].v[q].w) + d.v[q].w;
            }
        }
        GADAPT_STAMP(p.stamps, tslot + 5);
        __syncthreads();
        GADAPT_STAMP(p.stamps, tslot + 6);
    }
    if (prev_node0 >= 0) store_out(prev_node0);
}


// give a workgroup more than 64 tiles (Cfg::MAXM: its tile metadata must fit the LDS table).
// ------------------------------------------------------------------------------------------------
// backward, source pass when only columns 0..3 of g_out are wanted (the layer below reads the compact [N,4] encoder output: see
// grand_bwd_target_compact_kernel; the target pass before this launch was the D4 variant and left dxd as [N,4]):
//   g_out[j][c] = dxd[j][c] + sum_i alpha_ij dt g_i[c] + sum_o A[c][o] y_j[o] + sigma_j p0[c],   c = 0..3,
// with y_j = sum_i ds_ij x_i over the out-edges as in grand_bwd_source_kernel.  Of the g rows only the first 16 bytes are
// gathered, A y is four dot products per node on the vector ALU (no y tile, no matrix cores, no barrier between edge walk and
// result), and N C floats of dxd reads and g_out writes become N * 4 each.  GC: the upstream gradient is compact [N,g_cols].
// ------------------------------------------------------------------------------------------------
template <int HN_, int NV> struct SBuf4 {
    static constexpr int N = HN_;
    float4 g4[HN_];
    Vec<NV> x[HN_];
    float2 ev[HN_];
    float4 d4;
};
#ifndef GADAPT_WAVES_BWD_S4
#define GADAPT_WAVES_BWD_S4 3      /* hidden <= 64: 157..166 registers, three workgroups per CU (the launch uses a grid of 768) */
#endif
template <int C, bool GC = false>
__global__ __launch_bounds__(Cfg<C>::NT, (C > 64 ? 2 : GADAPT_WAVES_BWD_S4)) void grand_bwd_source4_kernel(BwdSArgs p) {
    using K = Cfg<C>;
    using V = Vec<K::NV>;
    extern __shared__ float4 smem4[];
    using CsrT = TileCsr<C, 2, 0>;                              // aux = {alpha*dt, d<P,x>} per out-edge (source order)
    CsrT csr;
    csr.bind(reinterpret_cast<float*>(smem4), p.rowptr, p.col, p.edge_ws, p.meta, p.n_edges);
    const int tid = threadIdx.x;
    const int slot = tid / K::LPN, sub = tid % K::LPN;
    float a4[K::NV][4][4];                                      // A[c][o], o = this lane's channels, c = 0..3
#pragma unroll
    for (int q = 0; q < K::NV; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float4 r = *reinterpret_cast<const float4*>(p.A + (size_t)c * C + 4 * (sub + q * K::LPN));
            a4[q][0][c] = r.x; a4[q][1][c] = r.y; a4[q][2][c] = r.z; a4[q][3][c] = r.w;
        }
    const float4 p04 = *reinterpret_cast<const float4*>(p.p0);
    auto ld_g4 = [&](int i) __attribute__((always_inline)) {   // columns 0..3 of row i of the upstream gradient (same address in the group)
        if constexpr (GC) return ld_row4_compact(p.g_in, i, 0, p.g_cols);
        else return *reinterpret_cast<const float4*>(p.g_in + (size_t)i * C);
    };
    // result of one node: the group's sum of the four dot products, lane sub == 0 writes
    auto finish = [&](int j, const float4& d4, const float4& z4, const V& y, float sig) __attribute__((always_inline)) {
        float t4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < K::NV; ++q) {
            const float yv[4] = {y.v[q].x, y.v[q].y, y.v[q].z, y.v[q].w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int c = 0; c < 4; ++c) t4[c] = fmaf(yv[e], a4[q][e][c], t4[c]);
        }
        group_sum_n<K::LPN>(t4);
        if (sub == 0 && j < p.n_nodes) {
            const float4 o = make_float4(d4.x + z4.x + t4[0] + sig * p04.x, d4.y + z4.y + t4[1] + sig * p04.y,
                                         d4.z + z4.z + t4[2] + sig * p04.z, d4.w + z4.w + t4[3] + sig * p04.w);
            *reinterpret_cast<float4*>(p.g_out + 4 * (size_t)j) = o;
        }
    };
    const TileRange tr = tile_range(p.n_tiles);
    const int tb = tr.t, stp = tr.step;
    const int n_my = tr.t < tr.t_end ? (tr.t_end - tr.t + tr.step - 1) / tr.step : 0;
    typename CsrT::Regs sr;
    {   // tile metadata and - its metadata word through the scalar cache (TileCsr::meta_scalar) - the first tile's CSR slice: one round trip
        const int4 mreg = csr.metas_issue(tb, stp, p.n_tiles, tid);
        const int4 m0 = csr.meta_scalar(tb, p.n_tiles);           // (behind the vector requests above: see TileCsr::meta_scalar)
        csr.issue_meta(sr, m0, min(tb, p.n_tiles - 1) * K::TM, p.n_nodes, tid);
        csr.metas_commit(mreg, tid);
    }
    __syncthreads();
    for (int k = 0; k < n_my; ++k) {
        const int t = tb + k * stp;
        const int node0 = t * K::TM;
        const int dmax = csr.commit(sr, tid, node0);
        __syncthreads();
        csr.issue(sr, k + 1, (t + stp) * K::TM, p.n_nodes, tid);   // unconditional, clamped past the end: lands during this tile
        if (dmax >= 0) {
            dispatch_dmax(dmax, [&](auto tag) {
                constexpr int DM = decltype(tag)::value;
                constexpr int HN = (DM + 1) / 2;
                auto fetch = [&](SBuf4<HN, K::NV>& b, int step) __attribute__((always_inline)) {
                    const int it = step >> 1, half = step & 1;
                    const int li = it * K::SLOTS + slot;
                    const int e0 = csr.rp[li] - csr.ebase + half * HN;
                    const int deg = (node0 + li < p.n_nodes) ? csr.rp[li + 1] - csr.rp[li] : 0;
#pragma unroll
                    for (int kk = 0; kk < HN; ++kk) {
                        const int i = csr.col[e0 + kk];              // past the row end: some valid row, weight 0
                        b.ev[kk] = *reinterpret_cast<const float2*>(csr.aux + 2 * (e0 + kk));
                        if (half * HN + kk >= deg) b.ev[kk] = make_float2(0.f, 0.f);
                        b.g4[kk] = ld_g4(i);
                        b.x[kk] = ld_vec<C>(p.x_in, i, sub);
                    }
                    b.d4 = *reinterpret_cast<const float4*>(p.dxd + 4 * (size_t)min(node0 + li, p.n_nodes - 1));
                };
                float4 z4; V y; float sig = 0.f;
                auto consume = [&](const SBuf4<HN, K::NV>& b, int step) __attribute__((always_inline)) {
                    const int it = step >> 1, half = step & 1;
                    if (half == 0) { z4 = f4zero(); y.zero(); sig = 0.f; }
#pragma unroll
                    for (int kk = 0; kk < HN; ++kk) { axpy4(z4, b.ev[kk].x, b.g4[kk]); vaxpy(y, b.ev[kk].y, b.x[kk]); sig += b.ev[kk].y; }
                    if (half == 1) finish(node0 + it * K::SLOTS + slot, b.d4, z4, y, sig);
                };
                run_pipeline<2 * K::ITERS, SBuf4<HN, K::NV>>(fetch, consume, [&]() {});
            });
        } else {
#pragma unroll 1
            for (int it = 0; it < K::ITERS; ++it) {              // any row length, CSR straight from HBM
                const int j = node0 + it * K::SLOTS + slot;
                float4 z4 = f4zero(); V y; y.zero();
                float sig = 0.f;
                float4 d4 = f4zero();
                if (j < p.n_nodes) {
                    d4 = *reinterpret_cast<const float4*>(p.dxd + 4 * (size_t)j);
                    const int e0 = p.rowptr[j], deg = p.rowptr[j + 1] - e0;
                    for (int kk = 0; kk < deg; ++kk) {
                        const int i = p.col[e0 + kk];
                        const float2 ev = *reinterpret_cast<const float2*>(p.edge_ws + 2 * (size_t)(e0 + kk));
                        axpy4(z4, ev.x, ld_g4(i));
                        vaxpy(y, ev.y, ld_vec<C>(p.x_in, i, sub));
                        sig += ev.y;
                    }
                }
                finish(j, d4, z4, y, sig);
            }
        }
        __syncthreads();                                        // every wave is done with the CSR slice of this tile
    }
}

// ------------------------------------------------------------------------------------------------
// backward, source pass of the narrow route (every layer input an [N,4] slot: DESIGN.md section 4): grand_bwd_source4_kernel's
// result, g_out[j][c] = dxd[j][c] + sum_i alpha_ij dt g_i[c] + sum_o A[c][o] y_j[o] + sigma_j p0[c] (c = 0..3), with x_i and y_j
// four columns wide as well.  ONE NODE PER LANE, grid-stride, no LDS: the out-neighbours and the row bounds in the first memory
// round trip (ELL), the {alpha dt, ds} pairs, g and x rows (16 bytes each) in the second.  g_in is [N,4], or the compact
// [N,g_cols] top gradient (g_cols > 0).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grand_bwd_source_narrow_kernel(BwdSArgs p) {
    const int C = p.c;
    float a4[4][4];                                             // A[c][o], c, o < 4
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int o = 0; o < 4; ++o) a4[c][o] = p.A[c * C + o];
    const float4 p04 = *reinterpret_cast<const float4*>(p.p0);
    auto ld_g4 = [&](int i) __attribute__((always_inline)) {
        return p.g_cols ? ld_row4_compact(p.g_in, i, 0, p.g_cols) : *reinterpret_cast<const float4*>(p.g_in + 4 * (size_t)i);
    };
    const float2* ew = reinterpret_cast<const float2*>(p.edge_ws);
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < p.n_nodes; j += (int64_t)gridDim.x * 256) {
        const int e0 = p.rowptr[j], deg = p.rowptr[j + 1] - e0;
        const int4 el0 = *reinterpret_cast<const int4*>(p.ell + 8 * (size_t)j), el1 = *reinterpret_cast<const int4*>(p.ell + 8 * (size_t)j + 4);
        const float4 d4 = *reinterpret_cast<const float4*>(p.dxd + 4 * (size_t)j);
        float4 z4 = f4zero(), y = f4zero();
        float sig = 0.f;
        if (deg <= 8 && p.n_edges > 0) {
            const int last = p.n_edges - 1;
            const int ej[8] = {el0.x, el0.y, el0.z, el0.w, el1.x, el1.y, el1.z, el1.w};
            float2 ev[8]; float4 gk[8], xk[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {                        // unconditional, clamped: weight 0 past the row end
                const int i = max(ej[k], 0);
                ev[k] = ew[min(e0 + k, last)];
                gk[k] = ld_g4(i);
                xk[k] = *reinterpret_cast<const float4*>(p.x_in + 4 * (size_t)i);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float2 e = k < deg ? ev[k] : make_float2(0.f, 0.f);
                axpy4(z4, e.x, gk[k]); axpy4(y, e.y, xk[k]); sig += e.y;
            }
        } else {
            for (int e = e0; e < e0 + deg; ++e) {
                const int i = p.col[e];
                const float2 ev = ew[e];
                axpy4(z4, ev.x, ld_g4(i)); axpy4(y, ev.y, *reinterpret_cast<const float4*>(p.x_in + 4 * (size_t)i)); sig += ev.y;
            }
        }
        const float yv[4] = {y.x, y.y, y.z, y.w};
        float t4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int c = 0; c < 4; ++c) t4[c] = fmaf(yv[o], a4[c][o], t4[c]);
        *reinterpret_cast<float4*>(p.g_out + 4 * (size_t)j) = make_float4(d4.x + z4.x + t4[0] + sig * p04.x, d4.y + z4.y + t4[1] + sig * p04.y,
                                                                          d4.z + z4.z + t4[2] + sig * p04.z, d4.w + z4.w + t4[3] + sig * p04.w);
    }
}
