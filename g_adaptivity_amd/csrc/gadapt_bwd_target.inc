// gadapt_bwd_target.inc - backward target pass grand_bwd_target_kernel<C,...> and the compact layer-0 kernel (autograd of src/GRAND_plus.py:225-343: softmax backward, dP, weight-gradient partials, dxd) (gfx950 only; see gadapt_internal.h for the translation units).

// ------------------------------------------------------------------------------------------------
// backward, target pass
// ------------------------------------------------------------------------------------------------
struct BwdTArgs {
    const float* x_in; const float* g_in; const float* alpha;
    const float* A; const float* lp;
    const int32_t* rowptr; const int32_t* col; const int32_t* tpos; const int32_t* meta;
    float2* edge_ws; float* dxd; float* slab; float* sums_out;   // sums_out: d dt of this layer (one float)
    int n_nodes, n_tiles, accumulate, residual_only, n_edges;
    unsigned long long* stamps;
    int g_cols;                                                 // GC kernels: g_in is [N,g_cols] (zero beyond), else unused
    float* sums_sc_out;                                         // d score_scale of this layer (one float); set with sums_out
    int c;                                                      // hidden size (read by grand_bwd_target_compact_kernel only)
    int g_stride;                                               // ... and the row pitch of its g_in, in floats
    int sums_partials;                                          // 1: sums_out / sums_sc_out are per-workgroup arrays [gridDim.x] (written, not added to)
    const int32_t* ell;                                         // grand_bwd_target_compact_kernel<., true>: gadapt_graph::ell_t ([N_pad][8] in-neighbours, -1 = unused)
    int slab_packed;                                            // bwd_target_compact_body: 1 = rows of GADAPT_NARROW_SLAB_ROW floats (its 20 partials side by side), 0 = rows of C*C + C
};

template <int NROWS, int NV> struct TBuf {
    static constexpr int N = NROWS;
    Vec<NV> r[NROWS];
    int deg, el0;
};

// SUMS: 1 = also reduce d/d(dt) (learn_step), 2 = d/d(dt) and d/d(score_scale) (learnable temperature).  Separate instantiations:
// hipcc otherwise sinks the per-edge log terms behind the pipeline and keeps dozens of registers alive for them.
//
// Rolling window like the forward: a workgroup walks consecutive tiles with slabs t-1, t, t+1 of x in an LDS ring,
// so on mesh-ordered graphs the x_j gathers are LDS reads.  Per tile the fourth LDS tile holds g (staged with the
// ring slab), then dP (written over g row by row by the lanes that read it), then dP A (in place).
// GC: the upstream gradient is compact, [N,g_cols] (top layer: backward of the x[:, :dim] slice) - only its staging differs.
// D4: only columns 0..3 of dxd are wanted (the layer BELOW reads the compact [N,4] encoder output, so its backward contracts
// d alpha = dt <g_i, x_k> over four columns and the source pass that follows this launch produces just those): dxd is written
// as [N,4] and dP A[:, :4] is four dot products per node on the vector ALU - no projection phase on the matrix cores, no
// pre-split copy, two barriers fewer per tile, and the dense dxd matrix (N C floats) is neither written nor read back.
template <int C, int SUMS, bool GC = false, bool D4 = false>
__global__ __launch_bounds__(Cfg<C>::NT, (C >= GADAPT_ONE_WAVE_C ? 1 : GADAPT_WAVES_BWD_T)) void grand_bwd_target_kernel(BwdTArgs p) {
    using K = Cfg<C>;
    using V = Vec<K::NV>;
    constexpr int SLABF = K::TILE_FLOATS;
    extern __shared__ float4 smem4[];
    float* ring = reinterpret_cast<float*>(smem4);
    float* ds = reinterpret_cast<float*>(smem4) + K::RING_T * SLABF;   // g tile -> dP tile -> dP A
    using CsrT = TileCsr<C, 1, 1>;                              // aux = forward alpha (target order), ext = tpos
    CsrT csr;
    csr.bind(ds + K::TILE_FLOATS, p.rowptr, p.col, p.alpha, p.meta, p.n_edges, p.tpos);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    GADAPT_STAMP(p.stamps, 30);                                 // diagnostic: kernel entry
    const int slot = tid / K::LPN, sub = tid % K::LPN;
    // out = base*x + dt*(m - x): Euler step (base 1) or bare residual (base 0, dt 1)
    const float dt = p.residual_only ? 1.0f : p.lp[0], sc = p.lp[1];
    const float w1 = (p.residual_only ? 0.0f : 1.0f) - dt;
    constexpr int ROW = C * C + C;                              // slab row: dA then dp0
    float* xs = ring;                                           // slab of the current tile

    // PRE: dP A takes dP from a pre-split f16 copy (lds_put_split) made after the edge walk in the window slot of slab t-1,
    // which nothing reads between that barrier and the next tile's commit; dinv = its row scales
    constexpr bool PRE = K::MFMA && !D4;
    float dinv[K::ITERS];
    TileGemm<C, true, PRE> gemm;               // dxd = dP A
    float acol[(K::MFMA || D4) ? 1 : 4][(K::MFMA || D4) ? 1 : C];   // VALU: A[o][4sub+t]
    float a4[D4 ? K::NV : 1][4][4];                             // D4: A[o][c], o = this lane's channels, c = 0..3
    if constexpr (D4) {
#pragma unroll
        for (int q = 0; q < K::NV; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float4 r = *reinterpret_cast<const float4*>(p.A + (size_t)(4 * (sub + q * K::LPN) + e) * C);
                a4[q][e][0] = r.x; a4[q][e][1] = r.y; a4[q][e][2] = r.z; a4[q][e][3] = r.w;
            }
        if constexpr (K::MFMA) gemm.init(lane, wave);
    } else if constexpr (K::MFMA) {
        gemm.init(lane, wave);
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int o = 0; o < C; ++o) acol[t][o] = p.A[o * C + 4 * sub + t];
    }
    // dA partial accumulators.  MFMA: NB2 = CB*CB 32x32 blocks of dA; >= NW blocks -> NB2/NW per wave over
    // all TM nodes, 1 block -> the 4 waves split the node range.  VALU: thread owns element tid % C^2 for
    // node subset tid / C^2.
    constexpr int NB2 = K::CB * K::CB;
    constexpr int DPW = K::MFMA ? (NB2 >= K::NW ? NB2 / K::NW : 1) : 1;
    static_assert(!K::MFMA || NB2 >= K::NW || (NB2 == 1 && K::NW == 4), "dA blocks per wave");
    f32x16 dacc[DPW];
    float dav = 0.f;
    if constexpr (K::MFMA) {
#pragma unroll
        for (int b = 0; b < DPW; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) dacc[b][r] = 0.f;
    }
    V dp0acc; dp0acc.zero();
    float sum_ddt = 0.f, sum_dsc = 0.f;
    V gk[K::ITERS];                                             // (base - dt) g_i of this lane's node slots, for the epilogue

    // Dg (SUMS): sum_k alpha_ik <g_i, x_k> of this node (group-uniform)
    auto finish = [&](int li, int i, int it, const V& gi, float Dg, const V& dP) __attribute__((always_inline)) {
        if (i < p.n_nodes) {
            if constexpr (SUMS) {
                // d dt = sum_i <g_i, m_i - x_i>   (GNN.py:288-289 learn_step) with <g_i, m_i> = sum_k alpha_ik <g_i, x_k> = Dg, which
                // the softmax backward has anyway: no aggregated row m_i is formed (it cost 8 registers and 48 fmas per node slot
                // and made these instantiations spill).  One lane of the group adds Dg, every lane its channels of -<g_i, x_i>.
                const V xi = lds_vec<C>(xs, li, sub);
                float own = (sub == 0) ? Dg : 0.f;
#pragma unroll
                for (int q = 0; q < K::NV; ++q)
                    own -= gi.v[q].x * xi.v[q].x + gi.v[q].y * xi.v[q].y + gi.v[q].z * xi.v[q].z + gi.v[q].w * xi.v[q].w;
                sum_ddt += own;
            }
#pragma unroll
            for (int q = 0; q < K::NV; ++q) {
                dp0acc.v[q].x += dP.v[q].x; dp0acc.v[q].y += dP.v[q].y; dp0acc.v[q].z += dP.v[q].z; dp0acc.v[q].w += dP.v[q].w;
            }
        }
        if constexpr (D4) {
            // dxd[i][0..3] = (base - dt) g_i[0..3] + sum_o dP_i[o] A[o][0..3]: this lane's channels, then the group
            float t4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < K::NV; ++q) {
                const float d[4] = {dP.v[q].x, dP.v[q].y, dP.v[q].z, dP.v[q].w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int c = 0; c < 4; ++c) t4[c] = fmaf(d[e], a4[q][e][c], t4[c]);
            }
            group_sum_n<K::LPN>(t4);
            gk[it].v[0] = make_float4(fmaf(w1, gi.v[0].x, t4[0]), fmaf(w1, gi.v[0].y, t4[1]), fmaf(w1, gi.v[0].z, t4[2]), fmaf(w1, gi.v[0].w, t4[3]));   // lane sub == 0 holds columns 0..3
        } else {
#pragma unroll
            for (int q = 0; q < K::NV; ++q) {
                gk[it].v[q].x = w1 * gi.v[q].x; gk[it].v[q].y = w1 * gi.v[q].y; gk[it].v[q].z = w1 * gi.v[q].z; gk[it].v[q].w = w1 * gi.v[q].w;
            }
        }
        lds_put<C>(ds, li, sub, dP);                            // over g_i: only this lane group reads that row
    };
    // SUMS instantiations take the edge dot products with g_i itself and fold dt into the score scale afterwards
    // (d alpha_ik = dt <g_i, x_k>): Dg above is then free, and dt = 0 needs no special case
    const float scl = SUMS ? sc * dt : sc;

    // WIN (compile time): gathers from the LDS ring (col holds ring offsets) or from HBM/L2; see the forward kernel
    auto fetch = [&](auto& b, int node0, int it, auto win_tag) __attribute__((always_inline)) {
        constexpr int DM = std::remove_reference_t<decltype(b)>::N;
        constexpr bool WIN = decltype(win_tag)::value != 0;
        const int li = it * K::SLOTS + slot;
        b.el0 = csr.rp[li] - csr.ebase;
        b.deg = (node0 + li < p.n_nodes) ? csr.rp[li + 1] - csr.rp[li] : 0;
        if constexpr (WIN) {
#pragma unroll
            for (int k = 0; k < DM; ++k) {
                const float* row = ring + csr.col[b.el0 + k];
#pragma unroll
                for (int q = 0; q < K::NV; ++q) b.r[k].v[q] = *reinterpret_cast<const float4*>(row + 4 * (sub + q * K::LPN));
            }
        } else {
#pragma unroll
            for (int k = 0; k < DM; ++k) b.r[k] = ld_vec<C>(p.x_in, csr.col[b.el0 + k], sub);   // k >= deg: some valid row, weight 0
        }
    };

    auto consume = [&](const auto& b, int node0, int it) __attribute__((always_inline)) {
        constexpr int DM = std::remove_reference_t<decltype(b)>::N;
        const int li = it * K::SLOTS + slot;
        const int i = node0 + li;
        const int deg = b.deg, e0 = b.el0;
        const V gi = lds_vec<C>(ds, li, sub);                   // rows past N were staged as zeros
        V dm;
#pragma unroll
        for (int q = 0; q < K::NV; ++q) {
            if constexpr (SUMS) { dm.v[q] = gi.v[q]; continue; }
            dm.v[q].x = dt * gi.v[q].x; dm.v[q].y = dt * gi.v[q].y; dm.v[q].z = dt * gi.v[q].z; dm.v[q].w = dt * gi.v[q].w;
        }
        float a[DM], da[DM];
        // Difference form (round 5, measured first in csrc/gadapt_smallmesh.inc): the softmax backward only uses d alpha_k - D and
        // sum_k ds_k x_k with sum_k ds_k = 0 - differences between the in-neighbours' rows.  Taken on x_k - x_i (exact algebra:
        // sum_k alpha_k = 1), the common part never enters the products, whose rounding otherwise costs |x| / |x_k - x_i| - the mesh
        // resolution - in accuracy:  d alpha_k - D = <dm, x_k - x_i> - sum_j alpha_j <dm, x_j - x_i>,  dP_i = sum_k ds_k (x_k - x_i) +
        // (sum_k ds_k) x_i.  (SUMS instantiations keep the plain form: their D doubles as <g_i, m_i> for d dt.)
        V xi0 = lds_vec<C>(xs, li, sub);
        if constexpr (SUMS != 0) xi0.zero();
#pragma unroll
        for (int k = 0; k < DM; ++k) {
            const float av = csr.aux[e0 + k];
            a[k] = (k < deg) ? av : 0.f;
            V d_ = b.r[k];
#pragma unroll
            for (int q = 0; q < K::NV; ++q) { d_.v[q].x -= xi0.v[q].x; d_.v[q].y -= xi0.v[q].y; d_.v[q].z -= xi0.v[q].z; d_.v[q].w -= xi0.v[q].w; }
            da[k] = vdot(dm, d_);
        }
        group_sum_n<K::LPN>(da);
        float D = 0.f;
#pragma unroll
        for (int k = 0; k < DM; ++k) D = fmaf(a[k], da[k], D);
        V dP; dP.zero();
        float dsum = 0.f;
#pragma unroll
        for (int k = 0; k < DM; ++k) {
            const float dsp = a[k] * (da[k] - D);                   // d(score') [/ dt: SUMS], score' = sc * <P_i,x_j>
            da[k] = dsp * scl;                                      // reuse: d<P_i,x_j>
            dsum += da[k];
            V d_ = b.r[k];
#pragma unroll
            for (int q = 0; q < K::NV; ++q) { d_.v[q].x -= xi0.v[q].x; d_.v[q].y -= xi0.v[q].y; d_.v[q].z -= xi0.v[q].z; d_.v[q].w -= xi0.v[q].w; }
            vaxpy(dP, da[k], d_);
        }
        vaxpy(dP, dsum, xi0);
        // per-edge scratch for the source pass, one edge per lane of the group; SUMS: the same lane adds its edge's term of
        // d/d(score_scale) = (1/sc) sum_e d(score')_e log alpha_e  (the softmax backward sums to zero per target, so the
        // log-partition term drops out) - one log per lane and node slot instead of DM group-uniform ones
        if constexpr (K::LPN >= DM) {
            const float am = pick(a, sub), dm_ = pick(da, sub);
            if constexpr (SUMS > 1) { if (sub < deg && am > 0.f) sum_dsc = fmaf(dm_, __logf(am), sum_dsc); }
            if (sub < deg) p.edge_ws[csr.ext[e0 + sub]] = make_float2(am * dt, dm_);
        } else {
#pragma unroll
            for (int k = 0; k < DM; ++k)
                if (k < deg && (k % K::LPN) == sub) {
                    p.edge_ws[csr.ext[e0 + k]] = make_float2(a[k] * dt, da[k]);
                    if constexpr (SUMS > 1) { if (a[k] > 0.f) sum_dsc = fmaf(da[k], __logf(a[k]), sum_dsc); }
                }
        }
        finish(li, i, it, gi, D, dP);
    };

    auto slow_node = [&](int node0, int it) __attribute__((always_inline)) {
        const int li = it * K::SLOTS + slot;
        const int i = node0 + li;
        V dP; dP.zero();
        float D = 0.f;
        const V gi = lds_vec<C>(ds, li, sub);
        if (i < p.n_nodes) {
            V dm;
#pragma unroll
            for (int q = 0; q < K::NV; ++q) {
                if constexpr (SUMS) { dm.v[q] = gi.v[q]; continue; }
                dm.v[q].x = dt * gi.v[q].x; dm.v[q].y = dt * gi.v[q].y; dm.v[q].z = dt * gi.v[q].z; dm.v[q].w = dt * gi.v[q].w;
            }
            const int e0 = p.rowptr[i], deg = p.rowptr[i + 1] - e0;
            for (int k = 0; k < deg; ++k)
                D = fmaf(p.alpha[e0 + k], group_sum<K::LPN>(vdot(dm, ld_vec<C>(p.x_in, p.col[e0 + k], sub))), D);
            for (int k = 0; k < deg; ++k) {
                const V v = ld_vec<C>(p.x_in, p.col[e0 + k], sub);
                const float ak = p.alpha[e0 + k];
                const float dsp = ak * (group_sum<K::LPN>(vdot(dm, v)) - D);
                const float dss = dsp * scl;
                vaxpy(dP, dss, v);
                if ((k % K::LPN) == sub) {
                    p.edge_ws[p.tpos[e0 + k]] = make_float2(ak * dt, dss);
                    if constexpr (SUMS > 1) { if (ak > 0.f) sum_dsc = fmaf(dss, __logf(ak), sum_dsc); }
                }
            }
        }
        finish(li, i, it, gi, D, dP);
    };

    // dxd rows of a finished tile leave the registers only after the NEXT tile's staging: vmcnt is in-order and hipcc
    // waits vmcnt(0) before the staging reads its prefetch registers, so stores issued just before it would be
    // waited for (a full write round trip per tile).
    auto store_dxd = [&](int node0) __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < K::ITERS; ++it) {
            const int i = node0 + it * K::SLOTS + slot;
            if constexpr (D4) {
                if (i < p.n_nodes && sub == 0) *reinterpret_cast<float4*>(p.dxd + 4 * (size_t)i) = gk[it].v[0];
            } else if (i < p.n_nodes) {
                st_vec<C>(p.dxd, i, sub, gk[it]);
            }
        }
    };
    const TileChunk ch = tile_chunk(p.n_tiles);                 // an empty chunk still flushes its (zero) slab row
    // This workgroup's slab row.  The partials an accumulating launch adds to are requested DURING the last tile, in the registers of that
    // tile's (pointless) prefetch of the tile after it: read in the flush, they were a memory round trip at the very end of every
    // accumulating launch - three of the four target launches of a weight-shared step.  ROWFLUSH (hidden 64: a tile is 64 rows of 64
    // floats, exactly the dA block): the x prefetch registers take dA row-wise - the pointer and the row count are wave-uniform
    // selects, no branch around a load - and the flush goes through LDS into that layout (16-byte stores of whole rows instead of
    // 4-byte stores); the dp0 entry rides in one more register, requested in every tile.
    float* row = p.slab + (size_t)blockIdx.x * ROW;
    constexpr bool ROWFLUSH = K::MFMA && NB2 >= K::NW && DPW == 1 && K::TM == C;
    TileRows<C> oldr;
    float dp0_ld = 0.f;
    if (ch.t0 >= ch.t1) {
        dp0_ld = __builtin_nontemporal_load(row + C * C + min(tid, C - 1));
        if constexpr (ROWFLUSH) oldr.issue(row, 0, C, tid);
    }
    if (ch.t0 < ch.t1) {
        auto slab_ptr = [&](int s_) __attribute__((always_inline)) { return ring + ((s_ + K::RING_T) % K::RING_T) * SLABF; };
        auto n0_of = [&](int t_) __attribute__((always_inline)) { return t_ * K::TM; };   // first node of tile t_
        typename CsrT::Regs sr;
        TileRows<C> xr, gr;
        // prologue loads in ONE memory round trip: the two slabs of the window's start (gr is free until the first g tile),
        // the tile metadata, the weight fragments - all requested before the first use (the fragment split) waits
        // Walk direction: every other workgroup of an XCD walks its chunk BACKWARDS.  Neighbouring chunks then meet at their common
        // boundary at the same time - both at the start or both at the end of the launch - so the halo slab one of them
        // stages is the slab the other one stages for its own tile within the same few microseconds: an L2 hit instead of a
        // second trip to the fabric (with every chunk walked forwards the two reads are a whole launch apart: x came in 1.5x).
        const int dir = (K::RING_T == 3 && ((blockIdx.x >> 3) & 1)) ? -1 : 1;
        const int tb = dir > 0 ? ch.t0 : ch.t1 - 1, n_my = ch.t1 - ch.t0;
        GADAPT_STAMP(p.stamps, 8);
        // the weight rows FIRST: L2-resident, back long before the window rows, and vmcnt is in-order - the split below waits for them
        // alone.  (Requested after the scalar metadata trip, as they were, their own trip and the split ran in series behind it:
        // 2.2k of the prologue's 9.2k cycles in the stamps.)
        typename decltype(gemm)::BRaw braw;
        if constexpr (K::MFMA && !D4) gemm.load_issue(p.A, nullptr, braw);
        if constexpr (K::RING_T == 3) {
            xr.issue(p.x_in, n0_of(tb - dir), p.n_nodes, tid);
            gr.issue(p.x_in, n0_of(tb), p.n_nodes, tid);
        }
        const int4 mreg = csr.metas_issue(tb, dir, p.n_tiles, tid);
        // ... and with them, in the same round trip, everything the FIRST tile needs (every later tile is requested one tile ahead, after
        // the edge walk of the tile before): the slab ahead, the tile's g rows, its CSR slice
        TileRows<C> xr2, gr2;
        xr2.issue(p.x_in, n0_of(tb + dir * K::LEAD_T), p.n_nodes, tid);
        if constexpr (GC) gr2.issue_compact(p.g_in, p.g_cols, n0_of(tb), p.n_nodes, tid); else gr2.template issue<false>(p.g_in, n0_of(tb), p.n_nodes, tid);
        GADAPT_STAMP(p.stamps, 9);
        const int4 m0 = csr.meta_scalar(tb, p.n_tiles);           // (behind the vector requests above: see TileCsr::meta_scalar)
        GADAPT_STAMP(p.stamps, 10);
        csr.issue_meta(sr, m0, n0_of(tb), p.n_nodes, tid);
        if constexpr (K::MFMA && !D4) gemm.load_finish(braw);    // split B fragments: built once, in registers for the whole launch
        GADAPT_STAMP(p.stamps, 11);
        csr.metas_commit(mreg, tid);
        if constexpr (K::RING_T == 3) {
            xr.commit(slab_ptr(tb - dir), p.n_nodes, tid);
            gr.commit(slab_ptr(tb), p.n_nodes, tid);
        }
        xr = xr2; gr = gr2;
        GADAPT_STAMP(p.stamps, 12);
        __syncthreads();                                        // tile metadata visible
        GADAPT_STAMP(p.stamps, 29);                             // diagnostic: prologue done
#pragma unroll 1
        for (int k = 0; k < n_my; ++k) {
            const int t = tb + k * dir;
            auto n0_rel = [&](int d_) __attribute__((always_inline)) { return (t + d_ * dir) * K::TM; };
            const int node0 = n0_rel(0);
            const int tslot = k * 8;
#ifdef GADAPT_STAMPS
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // diagnostic: separates the prefetch wait from the LDS writes
#endif
            GADAPT_STAMP(p.stamps, tslot + 0);
            xs = slab_ptr(t);
            const bool win = K::RING_T == 3 && (sr.meta.w & 1) != 0;
            xr.commit(slab_ptr(t + dir * K::LEAD_T), p.n_nodes, tid);
            gr.template commit_sel<GC>(ds, p.n_nodes, tid);
            const int dmax = csr.template commit<K::RING_T>(sr, tid, node0, win ? t : -1);
            GADAPT_STAMP(p.stamps, tslot + 1);
            __syncthreads();
            if (k > 0) store_dxd(n0_rel(-1));                   // previous tile's result: see store_dxd
            GADAPT_STAMP(p.stamps, tslot + 2);
            // ---- edge phase: dP_i per node -> LDS
            if (dmax >= 0) {
                dispatch_dmax(dmax, [&](auto tag) {
                    auto walk = [&](auto win_tag) __attribute__((always_inline)) {
                        run_pipeline<K::ITERS, TBuf<decltype(tag)::value, K::NV>>(
                            [&](auto& b, int it) { fetch(b, node0, it, win_tag); },
                            [&](const auto& b, int it) { consume(b, node0, it); },
                            [&]() {});
                    };
                    if (win) walk(IntTag<1>{}); else walk(IntTag<0>{});
                });
            } else {
#pragma unroll
                for (int it = 0; it < K::ITERS; ++it) slow_node(node0, it);
            }
            GADAPT_STAMP(p.stamps, tslot + 3);
            // request the next tile (unconditional, clamped past the end: see issue()).  Here rather than at the top
            // of the tile: the edge phase needs every register, and the MFMA phases below cover the round trip.
            csr.issue(sr, k + 1, n0_rel(1), p.n_nodes, tid);
            if constexpr (ROWFLUSH) {
                const bool lastk = k + 1 == n_my;               // the last tile: this slab row's old dA instead (see above)
                xr.issue(lastk ? row : p.x_in, lastk ? 0 : n0_rel(1 + K::LEAD_T), lastk ? C : p.n_nodes, tid);
            } else {
                xr.issue(p.x_in, n0_rel(1 + K::LEAD_T), p.n_nodes, tid);
            }
            if constexpr (GC) gr.issue_compact(p.g_in, p.g_cols, n0_rel(1), p.n_nodes, tid); else gr.template issue<false>(p.g_in, n0_rel(1), p.n_nodes, tid);
            dp0_ld = __builtin_nontemporal_load(row + C * C + min(tid, C - 1));
            __syncthreads();
            GADAPT_STAMP(p.stamps, tslot + 4);
            if constexpr (PRE) {
                float* cv = slab_ptr(t - dir);                  // the slab behind: dead until the next tile's commit puts the slab two ahead there
#pragma unroll
                for (int it = 0; it < K::ITERS; ++it) {
                    const int li = it * K::SLOTS + slot;
                    dinv[it] = lds_put_split<C>(cv, li, sub, lds_vec<C>(ds, li, sub));   // own rows: written by this lane group in finish()
                }
            }
            // ---- dA partial:  dA[o][c] += sum_node dP[node][o] x[node][c]
            if constexpr (K::MFMA && TileGemm<C, true>::SPLIT) {
                // bf16 three-piece form (see split8): k = node, 16 nodes per step; lane (i, h) feeds nodes 8h..8h+7 of the step
                const int h = lane >> 5, r31 = lane & 31;
                constexpr int NODES = (NB2 >= K::NW) ? K::TM : K::TM / 4;   // one 32x32 block: the waves split the nodes
                const int nbase = (NB2 >= K::NW) ? 0 : wave * NODES;
                const int ob = (NB2 >= K::NW) ? (wave * DPW) / K::CB : 0, cb0 = (NB2 >= K::NW) ? (wave * DPW) % K::CB : 0;
#pragma unroll 2
                for (int ks = 0; ks < NODES / 16; ++ks) {
                    const int n0 = nbase + 16 * ks + 8 * h;
                    float av[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) av[e] = ds[(n0 + e) * K::LD + ob * 32 + r31];
                    const Split3 as = split8(av);
                    // several blocks per wave (hidden 128): the x columns of block b + 1 are requested before block b is split
                    // and multiplied
                    float bv[2][8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) bv[0][e] = xs[(n0 + e) * K::LD + cb0 * 32 + r31];
#pragma unroll
                    for (int b = 0; b < DPW; ++b) {
                        if (b + 1 < DPW) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) bv[(b + 1) & 1][e] = xs[(n0 + e) * K::LD + (cb0 + b + 1) * 32 + r31];
                        }
                        const Split3 bs = split8(bv[b & 1]);
                        dacc[b] = mfma_bf16(as.h, bs.l, dacc[b]);
                        dacc[b] = mfma_bf16(as.l, bs.h, dacc[b]);
                        dacc[b] = mfma_bf16(as.m, bs.m, dacc[b]);
                        dacc[b] = mfma_bf16(as.h, bs.m, dacc[b]);
                        dacc[b] = mfma_bf16(as.m, bs.h, dacc[b]);
                        dacc[b] = mfma_bf16(as.h, bs.h, dacc[b]);
                    }
                }
            } else {
                constexpr int C2 = C * C;
                constexpr int NSUB = (256 / C2) > 0 ? (256 / C2) : 1;       // node subsets
                const int el = tid % C2, sb = tid / C2;
                if (sb < NSUB) {
                    const int o = el / C, c = el % C;
                    for (int node = sb; node < K::TM; node += NSUB) dav = fmaf(ds[node * K::LD + o], xs[node * K::LD + c], dav);
                }
            }
            GADAPT_STAMP(p.stamps, tslot + 5);
            // ---- dxd = (base-dt) g + dP A
            if constexpr (!D4) {
            if constexpr (PRE) {
                __syncthreads();                                // the pre-split copy is complete; every wave is done with dP in ds (dA)
                f32x16 acc[decltype(gemm)::BPW];
                gemm.accumulate_presplit(slab_ptr(t - dir), acc);
                gemm.store_presplit(ds, acc);
                __syncthreads();
            } else if constexpr (K::MFMA) {
                gemm.run_in_place(ds);                          // reads dP (like the dA pass), barrier, writes dP A
                __syncthreads();
            }
            GADAPT_STAMP(p.stamps, tslot + 6);
#pragma unroll
            for (int it = 0; it < K::ITERS; ++it) {
                const int li = it * K::SLOTS + slot;
                const int i = node0 + li;
                V r;
                if constexpr (K::MFMA) {
                    r = lds_vec<C>(ds, li, sub);
                } else {
                    r.zero();
#pragma unroll
                    for (int o = 0; o < C; ++o) {
                        const float d = ds[li * K::LD + o];
                        r.v[0].x = fmaf(d, acol[0][o], r.v[0].x); r.v[0].y = fmaf(d, acol[1][o], r.v[0].y);
                        r.v[0].z = fmaf(d, acol[2][o], r.v[0].z); r.v[0].w = fmaf(d, acol[3][o], r.v[0].w);
                    }
                }
                const float ri = PRE ? dinv[it] : 1.0f;         // pre-split operand: the row's inverse scale
#pragma unroll
                for (int q = 0; q < K::NV; ++q) {
                    gk[it].v[q].x = fmaf(r.v[q].x, ri, gk[it].v[q].x); gk[it].v[q].y = fmaf(r.v[q].y, ri, gk[it].v[q].y);
                    gk[it].v[q].z = fmaf(r.v[q].z, ri, gk[it].v[q].z); gk[it].v[q].w = fmaf(r.v[q].w, ri, gk[it].v[q].w);
                }
            }
            }
            __syncthreads();
            GADAPT_STAMP(p.stamps, tslot + 7);
        }
        store_dxd(n0_of(tb + (n_my - 1) * dir));
        if constexpr (ROWFLUSH) oldr = xr;
    }
    xs = ring;                                                  // scratch for the flush below

    // ---- flush partials into this workgroup's slab row (deterministic: one owner per element)
    constexpr int W = 4 * K::NV;
    float* red = xs;                                            // dp0 tree: [NT][W], spans into the dP tile for small C
    auto put_dp0 = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < K::NV; ++q) {
            red[tid * W + 4 * q + 0] = dp0acc.v[q].x; red[tid * W + 4 * q + 1] = dp0acc.v[q].y;
            red[tid * W + 4 * q + 2] = dp0acc.v[q].z; red[tid * W + 4 * q + 3] = dp0acc.v[q].w;
        }
    };
    const float dp0_old = (p.accumulate && tid < C) ? dp0_ld : 0.f;
    if constexpr (K::MFMA) {
        const int h = lane >> 5, r31 = lane & 31;
        if constexpr (ROWFLUSH) {
            // accumulator layout -> LDS [o][c] -> whole rows: thread t holds chunk t % 16 of rows t / 16 + 16 q, where oldr has the old partials
            const int ob = wave / K::CB, cb0 = wave % K::CB;
            float* tr = xs + K::TILE_FLOATS;                    // (the dp0 tree below uses the first slab)
#pragma unroll
            for (int r = 0; r < 16; ++r) tr[(ob * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * K::LD + cb0 * 32 + r31] = dacc[0][r];
            put_dp0();                                          // (one barrier for both exchanges)
            __syncthreads();
#pragma unroll
            for (int q = 0; q < TileRows<C>::XQ; ++q) {
                const int idx = q * K::NT + tid, r = idx / (C / 4), c4 = idx % (C / 4);
                const float4 v = *reinterpret_cast<const float4*>(tr + r * K::LD + 4 * c4);
                const float4 o4 = p.accumulate ? oldr.v[q] : f4zero();
                *reinterpret_cast<float4*>(row + r * C + 4 * c4) = make_float4(v.x + o4.x, v.y + o4.y, v.z + o4.z, v.w + o4.w);
            }
        } else if constexpr (NB2 >= K::NW) {
            const int ob = (wave * DPW) / K::CB, cb0 = (wave * DPW) % K::CB;
            // read-modify-write of the slab row in two phases: all loads of the old partials in flight at once, then the
            // stores (an interleaved load / add / store per element is one memory round trip per element at the kernel's tail:
            // measured 3.7 us of a 39 us launch at hidden 64, 28 of 128 us at hidden 128)
            float old[DPW][16];
#pragma unroll
            for (int b = 0; b < DPW; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = ob * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, c = (cb0 + b) * 32 + r31;
                    old[b][r] = p.accumulate ? __builtin_nontemporal_load(row + o * C + c) : 0.f;
                }
#pragma unroll
            for (int b = 0; b < DPW; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = ob * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, c = (cb0 + b) * 32 + r31;
                    row[o * C + c] = dacc[b][r] + old[b][r];
                }
        } else {
            float* red = xs;                                    // [4][32*32]
#pragma unroll
            for (int r = 0; r < 16; ++r) red[wave * 1024 + ((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + r31] = dacc[0][r];
            __syncthreads();
            for (int e = tid; e < 1024; e += K::NT) {
                float v = (red[e] + red[1024 + e]) + (red[2048 + e] + red[3072 + e]);
                if (p.accumulate) v += row[e];
                row[e] = v;
            }
            __syncthreads();
        }
    } else {
        constexpr int C2 = C * C;
        constexpr int NSUB = (256 / C2) > 0 ? (256 / C2) : 1;
        float* red = xs;
        if (tid < C2 * NSUB) red[tid] = dav;
        __syncthreads();
        if (tid < C2) {
            float v = 0.f;
            for (int sb = 0; sb < NSUB; ++sb) v += red[sb * C2 + tid];
            if (p.accumulate) v += row[tid];
            row[tid] = v;
        }
        __syncthreads();
    }
    {   // dp0 and the two scalars: tree over the node slots.  Thread (slot, sub) holds channels 4*(sub+q*LPN)+comp.
        if constexpr (!(K::MFMA && ROWFLUSH)) {
            put_dp0();
            __syncthreads();
        }
        if (tid < C) {
            const int c4 = tid / 4, comp = tid % 4;
            const int sb = c4 % K::LPN, q = c4 / K::LPN;
            float v = 0.f;
            for (int s = 0; s < K::SLOTS; ++s) v += red[(s * K::LPN + sb) * W + 4 * q + comp];
            row[C * C + tid] = v + dp0_old;
        }
        if constexpr (SUMS != 0) {
            // the two scalars: butterfly inside each wave, then the wave sums in order (a serial walk over the NT threads'
            // values by two threads was 256 dependent LDS reads at the tail of every workgroup: +3.6 us per launch)
            float v0 = sum_ddt, v1 = sum_dsc;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { v0 += __shfl_xor(v0, off, 64); if (SUMS > 1) v1 += __shfl_xor(v1, off, 64); }
            __syncthreads();                                    // the dp0 tree has read red[]
            if (lane == 0) { red[2 * wave] = v0; red[2 * wave + 1] = v1; }
            __syncthreads();
            if (p.sums_out && tid < (SUMS > 1 ? 2 : 1)) {
                float v = 0.f;
                for (int w_ = 0; w_ < K::NW; ++w_) v += red[2 * w_ + tid];
                if (tid == 1) v = v / (sc * sc);                // d/d(score_scale) = sum d(score') <P,x> = (1/sc) sum d(score') log alpha; the terms carry one more sc
                float* dst = tid == 0 ? p.sums_out : p.sums_sc_out;
                if (p.sums_partials) dst[blockIdx.x] = v;       // one slot per workgroup, summed in fixed order by layer_params_reduce_kernel
                else atomicAdd(dst, v);
            }
        }
    }
    GADAPT_STAMP(p.stamps, 31);                                 // diagnostic: slab row flushed
}

// ------------------------------------------------------------------------------------------------
// backward, target pass of a layer whose INPUT is the compact [N,4] encoder output (layer 0 behind the identity encoder,
// GNN.py:75-82: x0 = [features | 0]).  No source pass follows such a launch (d x0 is not wanted), so all it owes is the
// weight-gradient partial - and with x zero beyond column 3 that partial lives in a 4 x 4 corner:
//   d alpha_ik = dt <g_i, x_k>          touches the first four columns of g_i only,
//   dP_i = sum_k ds_ik x_k              is zero beyond column 3,
//   dA[o][c] += dP_i[o] x_i[c], dp0[o] += dP_i[o]     are non-zero for o, c < 4 only.
// So the launch reads 16 bytes of each g row, the [N,4] matrix and alpha, and adds 20 numbers per workgroup to the slab: one
// NODE PER LANE, no LDS tiles, no matrix cores.  (The generic kernel with the XC staging did the full-width edge walk, the dA
// phase and the flush of a 64 x 64 block for the same 20 numbers: 25.6 us per launch at hidden 64 on the metric workload.)
// Same arithmetic as grand_bwd_target_kernel, SUMS included; summation order: per lane over its nodes (grid-stride, ascending),
// wave butterfly, the four waves in order - fixed for a given grid, so runs stay bit-reproducible.
// ------------------------------------------------------------------------------------------------
// ELL: the neighbour indices come from the graph's ELL table (gadapt_graph::ell_t: entry k of row i = col[rowptr[i] + k]) with the row
// bounds, in the FIRST round trip, so the alpha entries and the neighbour rows share the second: two trips per node instead of three.
//
// NARROW (grand_bwd_target_narrow_kernel): the same pass for a layer above layer 0 on the narrow route, where every layer's input is
// an [N,4] slot (the zero-pad encoder's columns 4.. stay zero through every GRAND_plus layer: DESIGN.md section 4).  On top of the 20
// partials it owes the source pass what grand_bwd_target_kernel<64, 0, ., true> (D4) writes: the per-edge pair {alpha dt, ds} in
// source order (through tpos) and dxd[i][0..3] = (1 - dt) g_i[0..3] + sum_o dP_i[o] A[o][0..3].  g_in is [N,4], or the compact
// [N,g_cols] top gradient (g_cols > 0).
//
// SRC (gadapt_narrow_bwd.inc: the fused narrow backward): where g_i comes from.  NoFusedSource: from p.g_in.  A fused source computes it
// in this lane - the source pass of the layer ABOVE on the same node - and its loads ride in this pass's two round trips: issue1() goes
// out with the row bounds, the ELL row and x_i, issue2() with the alpha entries and the neighbour rows (both unconditional here, ahead
// of the degree branch), finish() returns g_i before the first use.
struct NoFusedSource { static constexpr bool FUSED = false; struct Regs {}; };
template <int SUMS, bool ELL, bool NARROW, class SRC = NoFusedSource>
__device__ __forceinline__ void bwd_target_compact_body(const BwdTArgs& p, const SRC& src = SRC()) {
    static_assert(!NARROW || (SUMS == 0 && ELL), "narrow route: fixed steps and temperature, ELL graphs");
    static_assert(!SRC::FUSED || (SUMS == 0 && ELL), "fused source pass: the narrow route");
    __shared__ float red[4][24];
    const int C = p.c;
    const int gs = p.g_stride;                                  // floats between g rows: C, or 4 when the layer above ran the D4 / source4 pair
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float dt = p.lp[0], sc = p.lp[1];
    const float scl = SUMS ? sc * dt : sc;
    const float w1 = 1.0f - dt;
    float a4[NARROW ? 4 : 1][4];                                // NARROW: A[o][c], o, c < 4
#pragma unroll
    for (int o = 0; o < (NARROW ? 4 : 0); ++o)
#pragma unroll
        for (int c = 0; c < 4; ++c) a4[o][c] = p.A[o * C + c];
    float acc[22];                                              // dA[o][c] (16), dp0[o] (4), d dt, d score_scale
#pragma unroll
    for (int k = 0; k < 22; ++k) acc[k] = 0.f;
    // this workgroup's slab row (layout of the tiled kernel: dA [C][C], then dp0 [C]).  The entry this thread adds to at the end of an
    // accumulating launch is requested HERE, with the first node's rows (unconditionally): read where it is added, it was one more
    // memory round trip at the very end of the launch
    // Packed rows (p.slab_packed; gadapt_block_backward_narrow_packed): GADAPT_NARROW_SLAB_ROW = 32 floats, one 128-byte line per
    // workgroup - entry 4 o + c = dA[o][c], entry 16 + o = dp0[o], entries 20..31 zero.
    float* row = p.slab + (size_t)blockIdx.x * (p.slab_packed ? GADAPT_NARROW_SLAB_ROW : C * C + C);
    const int e_own = p.slab_packed ? min(tid, GADAPT_NARROW_SLAB_ROW - 1)
                                    : (tid < 16 ? (tid >> 2) * C + (tid & 3) : C * C + (min(tid, 19) - 16));
    const float row_old = __builtin_nontemporal_load(row + e_own);
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < p.n_nodes; i += (int64_t)gridDim.x * 256) {
        float4 g4 = f4zero();
        if constexpr (!SRC::FUSED)
            g4 = (NARROW && p.g_cols) ? ld_row4_compact(p.g_in, (int)i, 0, p.g_cols) : *reinterpret_cast<const float4*>(p.g_in + (size_t)i * gs);
        const float4 xi = *reinterpret_cast<const float4*>(p.x_in + 4 * (size_t)i);
        const int e0 = p.rowptr[i], e1 = p.rowptr[i + 1], deg = e1 - e0;
        int4 el0 = make_int4(0, 0, 0, 0), el1 = el0;
        if constexpr (ELL) { el0 = *reinterpret_cast<const int4*>(p.ell + 8 * (size_t)i); el1 = *reinterpret_cast<const int4*>(p.ell + 8 * (size_t)i + 4); }
        [[maybe_unused]] typename SRC::Regs sr;
        if constexpr (SRC::FUSED) {
            src.issue1(sr, i);
            __builtin_amdgcn_sched_barrier(0);                    // every load of the first trip is out before anything waits for one
        }
        int cj[8], tp[8]; float ak[8];
        float4 xk[8];
        // second round trip: 8 column / alpha pairs (and the neighbour rows: ELL), unconditional with clamped indices
        auto issue2 = [&]() __attribute__((always_inline)) {
            const int last = max(p.n_edges - 1, 0);
            const int ej[8] = {el0.x, el0.y, el0.z, el0.w, el1.x, el1.y, el1.z, el1.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int e = min(e0 + k, last);
                if constexpr (ELL) cj[k] = max(ej[k], 0); else cj[k] = p.col[e];
                ak[k] = p.alpha[e];
                if constexpr (NARROW) tp[k] = p.tpos[e];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) xk[k] = *reinterpret_cast<const float4*>(p.x_in + 4 * (size_t)cj[k]);
        };
        if constexpr (SRC::FUSED) {
            if (p.n_edges > 0) {                                 // for every degree: the loads of both halves go out together
                issue2();
                src.issue2(sr);
            }
            __builtin_amdgcn_sched_barrier(0);
            g4 = src.finish(sr, i);
        }
        const float4 dm = SUMS ? g4 : make_float4(dt * g4.x, dt * g4.y, dt * g4.z, dt * g4.w);
        float D = 0.f;
        float4 dP = f4zero();
        if (deg <= 8 && p.n_edges > 0) {                          // (an edgeless graph has no col / alpha entry to clamp to)
            // the usual case, three memory round trips per node: (g row head, x row, row bounds) -> (8 column / alpha pairs,
            // unconditional with clamped indices) -> (8 neighbour rows); a loop over the row would chain them per edge.  (ELL: two.)
            if constexpr (!SRC::FUSED) issue2();
            float da[8];
            // difference form (see consume() of the tiled kernel; SUMS: plain form, D doubles as <g_i, m_i>)
            const float4 x0 = SUMS == 0 ? xi : f4zero();
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                ak[k] = (k < deg) ? ak[k] : 0.f;
                xk[k] = make_float4(xk[k].x - x0.x, xk[k].y - x0.y, xk[k].z - x0.z, xk[k].w - x0.w);
                da[k] = dot4(dm, xk[k]);
                D = fmaf(ak[k], da[k], D);
            }
            float dsum = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float ds = ak[k] * (da[k] - D) * scl;
                dsum += ds;
                axpy4(dP, ds, xk[k]);
                if constexpr (NARROW) { if (k < deg) p.edge_ws[tp[k]] = make_float2(ak[k] * dt, ds); }
                if constexpr (SUMS > 1) { if (ak[k] > 0.f) acc[21] = fmaf(ds, __logf(ak[k]), acc[21]); }
            }
            axpy4(dP, dsum, x0);
        } else {
            for (int e = e0; e < e1; ++e) {
                const float4 xk = *reinterpret_cast<const float4*>(p.x_in + 4 * (size_t)p.col[e]);
                D = fmaf(p.alpha[e], dot4(dm, xk), D);
            }
            for (int e = e0; e < e1; ++e) {
                const float4 xk = *reinterpret_cast<const float4*>(p.x_in + 4 * (size_t)p.col[e]);
                const float ak = p.alpha[e];
                const float ds = ak * (dot4(dm, xk) - D) * scl;
                axpy4(dP, ds, xk);
                if constexpr (NARROW) p.edge_ws[p.tpos[e]] = make_float2(ak * dt, ds);
                if constexpr (SUMS > 1) { if (ak > 0.f) acc[21] = fmaf(ds, __logf(ak), acc[21]); }
            }
        }
        if constexpr (SUMS != 0) acc[20] += D - dot4(g4, xi);    // d dt = sum_i <g_i, m_i - x_i>, <g_i, m_i> = D (see the tiled kernel)
        const float dp[4] = {dP.x, dP.y, dP.z, dP.w}, xv[4] = {xi.x, xi.y, xi.z, xi.w};
        if constexpr (NARROW) {
            float t4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int o = 0; o < 4; ++o)
#pragma unroll
                for (int c = 0; c < 4; ++c) t4[c] = fmaf(dp[o], a4[o][c], t4[c]);
            *reinterpret_cast<float4*>(p.dxd + 4 * (size_t)i) =
                make_float4(fmaf(w1, g4.x, t4[0]), fmaf(w1, g4.y, t4[1]), fmaf(w1, g4.z, t4[2]), fmaf(w1, g4.w, t4[3]));
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[4 * o + c] = fmaf(dp[o], xv[c], acc[4 * o + c]);
            acc[16 + o] += dp[o];
        }
    }
    // the wave butterfly 32, 16, .., 1 over the live entries on DPP / lane swaps (wave_sum_desc: the additions of __shfl_xor in that
    // order, without its LDS-crossbar trips - entry by entry with the store in between, each of the 120 was waited for on its own).
    // The node loop has ended for every lane: the whole wave is here.
    constexpr int LIVE = SUMS == 0 ? 20 : (SUMS > 1 ? 22 : 21);
    float part[LIVE];
#pragma unroll
    for (int k = 0; k < LIVE; ++k) part[k] = acc[k];
    wave_sum_desc(part);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < LIVE; ++k) red[wave][k] = part[k];
    }
    __syncthreads();
    if (!p.accumulate && p.slab_packed) {                       // accumulate = 0: the row is written whole - packed: its 12 spare entries
        if (tid >= 20 && tid < GADAPT_NARROW_SLAB_ROW) row[e_own] = 0.f;
    } else if (!p.accumulate) {
        for (int e = tid; e < C * C + C; e += 256) {
            const int o = e / C, c = e % C;
            const bool live = (e < C * C) ? (o < 4 && c < 4) : (e - C * C < 4);
            if (!live) row[e] = 0.f;
        }
    }
    if (tid < 20) {
        const float v = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        row[e_own] = p.accumulate ? row_old + v : v;
    }
    if constexpr (SUMS != 0) {
        if (p.sums_out && tid >= 20 && tid < (SUMS > 1 ? 22 : 21)) {
            float v = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
            if (tid == 21) v = v / (sc * sc);
            float* dst = tid == 20 ? p.sums_out : p.sums_sc_out;
            if (p.sums_partials) dst[blockIdx.x] = v; else atomicAdd(dst, v);
        }
    }
}
template <int SUMS, bool ELL = false>
__global__ __launch_bounds__(256) void grand_bwd_target_compact_kernel(BwdTArgs p) { bwd_target_compact_body<SUMS, ELL, false>(p); }
__global__ __launch_bounds__(256) void grand_bwd_target_narrow_kernel(BwdTArgs p) { bwd_target_compact_body<0, true, true>(p); }
