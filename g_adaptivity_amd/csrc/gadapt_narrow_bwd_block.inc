// gadapt_narrow_bwd_block.inc - the narrow route's backward layers below the top in ONE launch (grand_bwd_narrow_block_kernel), included by
// gadapt_tu_bwd_target.hip after gadapt_narrow_bwd.inc (gfx950 only; see gadapt_internal.h for the translation units).
//
// The fused launches [S_l + T_{l-1}] of gadapt_narrow_bwd.inc are local: S_l of node j reads the g rows, x rows and {alpha dt, ds} pairs of
// j's OUT-neighbours, T_{l-1} of node j reads g_j from the same lane and x rows the forward left in global memory.  So K <= 3 of them run as
// the stages of one launch by halo recompute, the block forward's method (gadapt_block_plan.h): a workgroup of eight waves owns
// GADAPT_NARROW_TILE = 512 consecutive nodes and runs stage s on its owned range widened by (K - 1 - s) halo on each side, for itself - no
// workgroup waits for another, the stages are separated by workgroup barriers only.  halo: of the SOURCE-ordered CSR
// (gadapt_narrow_block_register_source).
//
// Frame: row r holds node frame0 + r, frame0 = 512 t - margin, margin = (K - 1) halo rounded up to 64 (at most 128: 768 rows).  Thread tid
// keeps frame rows tid and tid + 512 at every stage (wave w: the 64-node blocks w and w + 8), so dxd[j] stays in a register from stage to
// stage and exactly one of a wave's two blocks is owned, whole.  A block wholly outside a stage's range leaves at a wave-uniform
// `continue`; a lane whose node is outside the range (or >= N) computes on clamped, finite operands and stores nothing.
//
// What a stage hands the next goes through LDS, never through global memory (100 224 bytes of dynamic LDS, one workgroup per CU):
//   grow  [2][768] float4   the g rows of the stage's range by frame row; stage s writes half s & 1, stage s + 1 reads it      24 576 B
//   pairA [5120] float2     the pairs stage 0 leaves for stage 1: those whose SOURCE lies in stage 1's range, at their position
//                           in source order relative to rowptr_s[lo of stage 1] (at most 640 rows of at most 8)                40 960 B
//   pairB [4096] float2     the same from stage 1 for stage 2 (512 owned rows)                                                 32 768 B
//   tred  [3][8][20] float  the wave sums of the 20 slab partials, by stage and owned block in node order                       1 920 B
// A target-half lane keeps a pair only when tpos[e] falls into the next stage's window; every position of that window belongs to an edge
// whose target is an out-neighbour of a node of the next range, hence in this stage's range: all of it is written.  Buffers alternate
// (grow) or are distinct (pairA / pairB), so one barrier per stage boundary is enough.
//
// Global reads.  Stage 0 reads what the launch above left: g rows (GC: the compact [N,g_cols] top gradient), the pairs, dxd.  Every stage
// reads the row bounds and ELL rows of both orientations, x rows of both layers, alpha and tpos, all requested before the first wait on
// any of them in two trips (sched_barriers), as the fused kernel does.  The ELL rows are re-read per stage (L2 hits that ride in the first
// trip): 40 registers that the two nodes' rows would otherwise hold for the whole launch.
//
// Statements.  Source half: FusedNarrowSource::finish, deg <= 8 branch; target half: the NARROW / SUMS = 0 / deg <= 8 branch of
// bwd_target_compact_body - COPIES of those statements (as narrow_top_target is), same expressions in the same order, fmaf where those
// call it, the translation unit's default contraction: the existing kernels keep their text and with it their instruction streams, and
// this kernel needs neither their longer-row loops nor their global stores.  Unused ELL entries (-1) read the lane's own g row from LDS
// where the fused kernel reads row 0 of the global buffer: weight 0 on a finite value either way.  Eligibility (narrow_bwd_block_eligible)
// refuses rows longer than 8 in either table.
//
// Slab rows.  Only owned nodes contribute.  The wave of an owned block runs wave_sum_scatter on its 20 partials after each stage (the whole
// wave: the branch is on the wave index; wave_sum_desc's additions, each total ending in one lane) and parks them in tred with one store
// from those 20 lanes; at the end 64 threads form, per stage, (b0 + b1) + (b2 + b3) for rows 2 t and 2 t + 1 and add them to the row read at the top of the launch in launch order, ((row_old + v0) + v1) + v2 - the sequence of
// accumulating launches this replaces, whose workgroup r sums nodes 256 r .. 256 r + 255 the same way (N <= 256 rows: one node per lane).
// Rows from 2 n_tiles on are not touched: no node maps to them, T_{L-1} wrote +0 there and each launch this replaces adds
// (+0 + +0) + (+0 + +0) = +0 to it, which leaves +0 (tests/test_gpu_narrow_block_backward.py compares all 32 entries of every row).
// Entries 20..31 of a row are not written either: an accumulating launch leaves them as they are.
//
// L0: the last stage's target half is layer 0 - partials only, nothing else stored.  !L0 (a group that is not the last, L >= 6): the last
// stage stores g_out, dxd_out and the pairs through tpos into edge_out for OWNED nodes only; dxd_out is NOT the buffer stage 0 reads
// (other workgroups read dxd_in rows of their halo nodes while the owner stores), nor is edge_out edge_in or g_out g_in.

constexpr int NBB_NT = GADAPT_NARROW_TILE;                       // threads per workgroup = nodes a workgroup owns
constexpr int NBB_FRAME = NBB_NT + 2 * 128;                      // frame rows at most
constexpr int NBB_PAIR_A = 8 * (NBB_NT + 128), NBB_PAIR_B = 8 * NBB_NT;
constexpr int NBB_LDS_BYTES = 2 * NBB_FRAME * 16 + (NBB_PAIR_A + NBB_PAIR_B) * 8 + GADAPT_NARROW_BWD_BLOCK_STAGES * 8 * 20 * 4;

struct BwdBlockArgs {
    const float* x_src0; long long slot_stride;                 // [N,4] rows of stage 0's source layer; stage s: - s slot_stride, its target layer one more
    const float* alpha0; long long alpha_stride;                // alpha of stage 0's TARGET layer; stage s: - s alpha_stride
    const float* lp0;                                           // {dt, scale} of stage 0's target layer; stage s: - 2 s
    const float* A; const float* p0;                            // the shared conv
    const float* g_in; const float2* edge_in; const float* dxd_in;   // what the launch above left (stage 0)
    float* g_out; float2* edge_out; float* dxd_out;             // !L0: the last stage's stores, owned nodes
    const int32_t* rowptr_t; const int32_t* ell_t; const int32_t* tpos; const int32_t* rowptr_s; const int32_t* ell_s;
    float* slab;
    int n_nodes, n_edges, K, halo, c, g_cols, slab_rows;
};

template <bool L0, bool GC>
__global__ __launch_bounds__(NBB_NT) void grand_bwd_narrow_block_kernel(BwdBlockArgs q) {
    extern __shared__ float4 nbb_smem[];
    float4* const grow = nbb_smem;
    float2* const pairA = reinterpret_cast<float2*>(grow + 2 * NBB_FRAME);
    float2* const pairB = pairA + NBB_PAIR_A;
    float* const tred = reinterpret_cast<float*>(pairB + NBB_PAIR_B);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = q.n_nodes, K = q.K, C = q.c, last = q.n_edges - 1;
    const int margin = gadapt_bwd_block_margin(q.halo, K);
    const int frame0 = NBB_NT * blockIdx.x - margin, last_row = NBB_NT + 2 * margin - 1;
    const int so = 64 * wave < margin ? 1 : 0;                   // which of this wave's two blocks is owned
    const int ob = gadapt_block_owned_block(margin, wave);

    // ---- the slab entry this thread adds to at the end, requested with the first loads (rows 2 t, 2 t + 1: gadapt_block_slab_plan)
    const gadapt_block_slab sp = gadapt_block_slab_plan(N, margin, blockIdx.x);
    const int sj = (tid >> 5) & 1, se = tid & 31, srow = sj ? sp.rows[1] : sp.rows[0];
    const bool slab_lane = tid < 64 && se < 20 && srow < q.slab_rows;
    float row_old = 0.f;
    if (slab_lane) row_old = __builtin_nontemporal_load(q.slab + (size_t)srow * GADAPT_NARROW_SLAB_ROW + se);
    float a4[4][4];                                              // A[o][c], o, c < 4: the source half reads it as [c][o], the target half as [o][c]
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int c = 0; c < 4; ++c) a4[o][c] = q.A[o * C + c];
    const float4 p04 = *reinterpret_cast<const float4*>(q.p0);
    float dts[GADAPT_NARROW_BWD_BLOCK_STAGES], scs[GADAPT_NARROW_BWD_BLOCK_STAGES];
#pragma unroll
    for (int s = 0; s < GADAPT_NARROW_BWD_BLOCK_STAGES; ++s) { dts[s] = q.lp0[-2 * min(s, K - 1)]; scs[s] = q.lp0[-2 * min(s, K - 1) + 1]; }
    // an owned block past ceil32(N) runs no stage: its partials are zeros (the same wave writes them again: LDS operations complete in order)
    if (lane < 20) {
#pragma unroll
        for (int s = 0; s < GADAPT_NARROW_BWD_BLOCK_STAGES; ++s) tred[(s * 8 + ob) * 20 + lane] = 0.f;
    }

    const int pe = wave_sum_scatter_entry(lane), park = pe < 0 ? -1 : ob * 20 + pe;   // where this lane parks the total it ends with, in a stage's [8][20]

    float4 dreg[2] = {f4zero(), f4zero()};                       // dxd of this lane's two nodes, from stage to stage
    int wb = 0, wlast = 0;                                      // this stage's pair window in LDS: first position in source order, last index
#pragma unroll 1
    for (int s = 0; s < K; ++s) {
        int64_t lo64, hi64;
        gadapt_block_range(N, q.halo, K, blockIdx.x, s, &lo64, &hi64);
        const int slo = (int)lo64, shi = (int)hi64;
        const bool fin = s == K - 1;
        int wb_n = 0, wn_n = 0;                                  // the next stage's window: first position, entries
        if (!fin) {
            gadapt_block_range(N, q.halo, K, blockIdx.x, s + 1, &lo64, &hi64);
            wb_n = q.rowptr_s[min((int)lo64, N)];
            wn_n = min(q.rowptr_s[min((int)hi64, N)] - wb_n, gadapt_bwd_block_pair_cap(K, s + 1));
        }
        const float dt = s == 0 ? dts[0] : (s == 1 ? dts[1] : dts[2]);
        const float sc = s == 0 ? scs[0] : (s == 1 ? scs[1] : scs[2]);
        const float w1 = 1.0f - dt;
        const float* x_src = q.x_src0 - s * q.slot_stride;
        const float* x_tgt = x_src - q.slot_stride;
        const float* alpha = q.alpha0 - s * q.alpha_stride;
        const float4* g_rd = grow + ((s + 1) & 1) * NBB_FRAME;   // (s >= 1: the half stage s - 1 wrote)
        float4* g_wr = grow + (s & 1) * NBB_FRAME;
        const float2* p_rd = s == 1 ? pairA : pairB;
        float2* p_wr = s == 0 ? pairA : pairB;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const int b0 = frame0 + 64 * wave + NBB_NT * s2;     // this wave's block: nodes b0 .. b0 + 63
            if (b0 + 64 <= slo || b0 >= shi) continue;           // (workgroup barriers stay outside: every wave runs all of them)
            const int r = tid + NBB_NT * s2, j = frame0 + r;     // this lane's frame row and node
            const bool valid = j >= slo && j < shi && j < N;
            const bool owned = s2 == so;
            const int jc = min(max(j, 0), N - 1);
            // ---- first trip: row bounds and ELL rows of both orientations, the own x row, dxd (stage 0)
            const int e0s = q.rowptr_s[jc], degs = q.rowptr_s[jc + 1] - e0s;
            const int4 es0 = *reinterpret_cast<const int4*>(q.ell_s + 8 * (size_t)jc), es1 = *reinterpret_cast<const int4*>(q.ell_s + 8 * (size_t)jc + 4);
            const int e0t = q.rowptr_t[jc], degt = q.rowptr_t[jc + 1] - e0t;
            const int4 et0 = *reinterpret_cast<const int4*>(q.ell_t + 8 * (size_t)jc), et1 = *reinterpret_cast<const int4*>(q.ell_t + 8 * (size_t)jc + 4);
            const float4 xi = *reinterpret_cast<const float4*>(x_tgt + 4 * (size_t)jc);
            float4 d4 = dreg[s2];
            if (s == 0) d4 = *reinterpret_cast<const float4*>(q.dxd_in + 4 * (size_t)jc);
            __builtin_amdgcn_sched_barrier(0);                    // every load of the first trip is out before anything waits for one
            // ---- second trip: the source half's pairs, g rows, x rows; the target half's alpha, tpos, neighbour x rows
            float2 ev[8]; float4 gk[8], xs[8];
            float ak[8]; int tp[8]; float4 xk[8];
            const int ejs[8] = {es0.x, es0.y, es0.z, es0.w, es1.x, es1.y, es1.z, es1.w};
            const int ejt[8] = {et0.x, et0.y, et0.z, et0.w, et1.x, et1.y, et1.z, et1.w};
            if (s == 0) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {                    // unconditional, clamped: weight 0 past the row end
                    const int i = max(ejs[k], 0);
                    ev[k] = q.edge_in[min(e0s + k, last)];
                    if constexpr (GC) gk[k] = ld_row4_compact(q.g_in, i, 0, q.g_cols); else gk[k] = *reinterpret_cast<const float4*>(q.g_in + 4 * (size_t)i);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) {                    // (an index outside the window / the frame - never on an eligible graph - is clamped into it)
                    ev[k] = p_rd[min(max(e0s + k - wb, 0), wlast)];
                    gk[k] = g_rd[ejs[k] < 0 ? r : min(max(ejs[k] - frame0, 0), last_row)];
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) xs[k] = *reinterpret_cast<const float4*>(x_src + 4 * (size_t)max(ejs[k], 0));
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int e = min(e0t + k, last);
                ak[k] = alpha[e];
                tp[k] = q.tpos[e];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) xk[k] = *reinterpret_cast<const float4*>(x_tgt + 4 * (size_t)max(ejt[k], 0));
            __builtin_amdgcn_sched_barrier(0);

            // ---- source half of layer l (FusedNarrowSource::finish, rows of at most 8)
            float4 g4;
            {
                float4 z4 = f4zero(), y = f4zero();
                float sig = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float2 e = k < degs ? ev[k] : make_float2(0.f, 0.f);
                    axpy4(z4, e.x, gk[k]); axpy4(y, e.y, xs[k]); sig += e.y;
                }
                const float yv[4] = {y.x, y.y, y.z, y.w};
                float t4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int o = 0; o < 4; ++o)
#pragma unroll
                    for (int c = 0; c < 4; ++c) t4[c] = fmaf(yv[o], a4[c][o], t4[c]);
                g4 = make_float4(d4.x + z4.x + t4[0] + sig * p04.x, d4.y + z4.y + t4[1] + sig * p04.y,
                                 d4.z + z4.z + t4[2] + sig * p04.z, d4.w + z4.w + t4[3] + sig * p04.w);
            }
            if (!fin) { if (valid) g_wr[r] = g4; }
            else if constexpr (!L0) { if (valid && owned) *reinterpret_cast<float4*>(q.g_out + 4 * (size_t)j) = g4; }

            // ---- target half of layer l - 1 (bwd_target_compact_body, NARROW, rows of at most 8)
            const float4 dm = make_float4(dt * g4.x, dt * g4.y, dt * g4.z, dt * g4.w);
            float D = 0.f;
            float4 dP = f4zero();
            float da[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                ak[k] = (k < degt) ? ak[k] : 0.f;
                xk[k] = make_float4(xk[k].x - xi.x, xk[k].y - xi.y, xk[k].z - xi.z, xk[k].w - xi.w);
                da[k] = dot4(dm, xk[k]);
                D = fmaf(ak[k], da[k], D);
            }
            float dsum = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float ds = ak[k] * (da[k] - D) * sc;
                dsum += ds;
                axpy4(dP, ds, xk[k]);
                if (!fin) {                                      // for the next stage: only the pairs whose source it runs
                    if (valid && k < degt && (unsigned)(tp[k] - wb_n) < (unsigned)wn_n) p_wr[tp[k] - wb_n] = make_float2(ak[k] * dt, ds);
                } else if constexpr (!L0) {
                    if (valid && owned && k < degt) q.edge_out[tp[k]] = make_float2(ak[k] * dt, ds);
                }
            }
            axpy4(dP, dsum, xi);
            const float dp[4] = {dP.x, dP.y, dP.z, dP.w}, xv[4] = {xi.x, xi.y, xi.z, xi.w};
            if (!fin || !L0) {
                float t4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int o = 0; o < 4; ++o)
#pragma unroll
                    for (int c = 0; c < 4; ++c) t4[c] = fmaf(dp[o], a4[o][c], t4[c]);
                dreg[s2] = make_float4(fmaf(w1, g4.x, t4[0]), fmaf(w1, g4.y, t4[1]), fmaf(w1, g4.z, t4[2]), fmaf(w1, g4.w, t4[3]));
                if constexpr (!L0) { if (fin && valid && owned) *reinterpret_cast<float4*>(q.dxd_out + 4 * (size_t)j) = dreg[s2]; }
            }
            if (!owned) continue;                                // a halo block owes the slab nothing (wave-uniform)
            // ---- the 20 partials of the owned block: the sums start at +0 and ADD their one node (the standalone kernel's loop: not folded)
            float zero = 0.f;
            asm volatile("" : "+v"(zero));
            float part[20];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
#pragma unroll
                for (int c = 0; c < 4; ++c) part[4 * o + c] = valid ? fmaf(dp[o], xv[c], zero) : 0.f;
                part[16 + o] = valid ? zero + dp[o] : 0.f;
            }
            const float tot = wave_sum_scatter(part, lane);            // every lane of the owned block's wave is here
            if (park >= 0) tred[s * 160 + park] = tot;           // each total from the lane it ended in: one LDS store
        }
        wb = wb_n; wlast = max(wn_n - 1, 0);
        if (!fin) __syncthreads();                               // stage s is in LDS
    }
    // ---- the slab rows this tile owes: per stage (b0 + b1) + (b2 + b3) over the row's blocks in node order, added in launch order
    __syncthreads();
    if (slab_lane) {
        float v = row_old;
        for (int s = 0; s < K; ++s) {
            const float* t = tred + (s * 8 + 4 * sj) * 20 + se;
            v = v + ((t[0] + t[20]) + (t[40] + t[60]));
        }
        q.slab[(size_t)srow * GADAPT_NARROW_SLAB_ROW + se] = v;
    }
}
