// gadapt_small.inc - per-step small kernels: composite coefficients and their chain rule, encoder, slab reductions, loss, Adam (gfx950 only; see gadapt_internal.h for the translation units).

// ------------------------------------------------------------------------------------------------
// small kernels
// ------------------------------------------------------------------------------------------------
// C is a compile-time trip count so that every load of a dot product is in flight at once (a runtime-length loop
// pays one L2 round trip per unrolled group).
template <int C>
__device__ __forceinline__ void coeffs_fwd_body(const float* __restrict__ wq, const float* __restrict__ bq, const float* __restrict__ wk,
                                                float* __restrict__ a, float* __restrict__ p0, int e) {
    if (e < C * C) {                    // A[o][cc] = sum_r wk[r][o] wq[r][cc]
        const int o = e / C, cc = e % C;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < C; ++r) v[r & 3] = fmaf(wk[r * C + o], wq[r * C + cc], v[r & 3]);
        a[e] = (v[0] + v[1]) + (v[2] + v[3]);
    } else if (e < C * C + C) {
        const int o = e - C * C;
        float v = 0.f;
#pragma unroll
        for (int r = 0; r < C; ++r) v = fmaf(wk[r * C + o], bq[r], v);
        p0[o] = v;
    }
}
template <int C>
__global__ void coeffs_fwd_kernel(const float* __restrict__ wq, const float* __restrict__ bq, const float* __restrict__ wk,
                                  float* __restrict__ a, float* __restrict__ p0) {
    coeffs_fwd_body<C>(wq, bq, wk, a, p0, blockIdx.x * blockDim.x + threadIdx.x);
}

template <int C>
__global__ void coeffs_bwd_kernel(const float* __restrict__ wq, const float* __restrict__ bq, const float* __restrict__ wk,
                                  const float* __restrict__ d_a, const float* __restrict__ d_p0,
                                  float* __restrict__ d_wq, float* __restrict__ d_bq, float* __restrict__ d_wk, float* __restrict__ d_bk) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    constexpr int c2 = C * C;
    if (e < c2) {                       // d_wq[r][cc] = sum_o wk[r][o] dA[o][cc]
        const int r = e / C, cc = e % C;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int o = 0; o < C; ++o) v[o & 3] = fmaf(wk[r * C + o], d_a[o * C + cc], v[o & 3]);
        d_wq[e] = (v[0] + v[1]) + (v[2] + v[3]);
    } else if (e < 2 * c2) {            // d_wk[r][o] = sum_cc wq[r][cc] dA[o][cc] + bq[r] dp0[o]
        const int f = e - c2, r = f / C, o = f % C;
        float v[4] = {bq[r] * d_p0[o], 0.f, 0.f, 0.f};
#pragma unroll
        for (int cc = 0; cc < C; ++cc) v[cc & 3] = fmaf(wq[r * C + cc], d_a[o * C + cc], v[cc & 3]);
        d_wk[f] = (v[0] + v[1]) + (v[2] + v[3]);
    } else if (e < 2 * c2 + C) {        // d_bq[r] = sum_o wk[r][o] dp0[o]
        const int r = e - 2 * c2;
        float v = 0.f;
#pragma unroll
        for (int o = 0; o < C; ++o) v = fmaf(wk[r * C + o], d_p0[o], v);
        d_bq[r] = v;
    } else if (e < 2 * c2 + 2 * C) {
        d_bk[e - 2 * c2 - C] = 0.f;
    }
}

// x0[i][4q..4q+3] = sum_k feats[i][k] w[4q+t][k] (+ b).  W^T sits in LDS as float4 per (k, q); C/4 consecutive
// threads write one 4*C-byte row, and a thread keeps its q while it strides over nodes.
#define GADAPT_ENC_MAX_WORDS 4096      /* C * F floats of LDS */
struct EncArgs {
    const float* feats; int f0; const float* e1; const float* e2; const float* w; const float* b; float* x0;
    int64_t n_nodes; int f, c;
};
// block `bid` of `nblocks` encoder blocks (the merged encoder + coefficient launch runs more blocks than that)
__device__ __forceinline__ void encode_body(const EncArgs& p, float4* wl, int bid, int nblocks) {
    const float* __restrict__ feats = p.feats; const float* __restrict__ e1 = p.e1; const float* __restrict__ e2 = p.e2;
    const float* __restrict__ w = p.w; const float* __restrict__ b = p.b; float* __restrict__ x0 = p.x0;
    const int f0 = p.f0, f = p.f, c = p.c; const int64_t n_nodes = p.n_nodes;
    const int c4 = c >> 2;
    for (int idx = threadIdx.x; idx < f * c4; idx += blockDim.x) {
        const int k = idx / c4, q = idx % c4;
        wl[idx] = make_float4(w[(4 * q + 0) * f + k], w[(4 * q + 1) * f + k], w[(4 * q + 2) * f + k], w[(4 * q + 3) * f + k]);
    }
    __syncthreads();
    const int q = threadIdx.x % c4;
    const int rows_per_block = blockDim.x / c4;
    const float4 bias = b ? *reinterpret_cast<const float4*>(b + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    // features of node i: the f0 columns of feats [N,f0], then the per-node scalars e1, e2 (GNN.py:227-239 concat).
    // Four rows per thread and iteration, every load of the four issued before the first use (the kernel is a pure
    // HBM write stream: what limits it is how many stores a wave keeps in flight).
    constexpr int R = 4;
    const int64_t stride = (int64_t)nblocks * rows_per_block;
    for (int64_t i0 = (int64_t)bid * rows_per_block + threadIdx.x / c4; i0 < n_nodes; i0 += R * stride) {
        float xv[R][4], x1[R], x2[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t i = min(i0 + r * stride, n_nodes - 1);
#pragma unroll
            for (int k = 0; k < 4; ++k) xv[r][k] = feats[i * f0 + min(k, f0 - 1)];
            x1[r] = e1 ? e1[i] : 0.f;
            x2[r] = e2 ? e2[i] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t i = i0 + r * stride;
            if (i >= n_nodes) break;
            float4 v = bias;
            if (f0 <= 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k < f0) {
                        const float4 wv = wl[k * c4 + q];
                        v.x = fmaf(xv[r][k], wv.x, v.x); v.y = fmaf(xv[r][k], wv.y, v.y); v.z = fmaf(xv[r][k], wv.z, v.z); v.w = fmaf(xv[r][k], wv.w, v.w);
                    }
                }
            } else {
                for (int k = 0; k < f0; ++k) {
                    const float xk = feats[i * f0 + k];
                    const float4 wv = wl[k * c4 + q];
                    v.x = fmaf(xk, wv.x, v.x); v.y = fmaf(xk, wv.y, v.y); v.z = fmaf(xk, wv.z, v.z); v.w = fmaf(xk, wv.w, v.w);
                }
            }
            if (e1) {
                const float4 wv = wl[f0 * c4 + q];
                v.x = fmaf(x1[r], wv.x, v.x); v.y = fmaf(x1[r], wv.y, v.y); v.z = fmaf(x1[r], wv.z, v.z); v.w = fmaf(x1[r], wv.w, v.w);
            }
            if (e2) {
                const float4 wv = wl[(f - 1) * c4 + q];
                v.x = fmaf(x2[r], wv.x, v.x); v.y = fmaf(x2[r], wv.y, v.y); v.z = fmaf(x2[r], wv.z, v.z); v.w = fmaf(x2[r], wv.w, v.w);
            }
            *reinterpret_cast<float4*>(x0 + i * c + 4 * q) = v;
        }
    }
}
__global__ __launch_bounds__(256) void encode_linear_kernel(EncArgs p) {
    __shared__ float4 wl[GADAPT_ENC_MAX_WORDS / 4];
    encode_body(p, wl, blockIdx.x, gridDim.x);
}
// The encoder and the composite coefficients (A, p0) of the shared conv are independent and both precede layer 0: one
// launch, the first `enc_blocks` workgroups encode, the rest compute coefficients (a dependent dispatch costs ~4.5 us).
template <int C>
__global__ __launch_bounds__(256) void encode_coeffs_kernel(EncArgs p, int enc_blocks, const float* __restrict__ wq, const float* __restrict__ bq,
                                                            const float* __restrict__ wk, float* __restrict__ a, float* __restrict__ p0) {
    __shared__ float4 wl[GADAPT_ENC_MAX_WORDS / 4];
    if ((int)blockIdx.x < enc_blocks) { encode_body(p, wl, blockIdx.x, enc_blocks); return; }
    coeffs_fwd_body<C>(wq, bq, wk, a, p0, ((int)blockIdx.x - enc_blocks) * 256 + threadIdx.x);
}

// g_top[i][:] = {g_phys[i][0..d), 0, ...}: backward of the x[:, :dim] slice (GNN.py:299) in one pass
__global__ void pad_columns_kernel(const float* __restrict__ g_phys, float* __restrict__ g_top, int64_t n_nodes, int d, int c) {
    const int c4 = c >> 2;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_nodes * c4) return;
    const int64_t i = e / c4;
    const int o = (int)(e % c4) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (o < d) {
        v.x = g_phys[i * d + o];
        if (o + 1 < d) v.y = g_phys[i * d + o + 1];
        if (o + 2 < d) v.z = g_phys[i * d + o + 2];
        if (o + 3 < d) v.w = g_phys[i * d + o + 3];
    }
    *reinterpret_cast<float4*>(g_top + i * c + o) = v;
}

// slab [n_rows][row_len] -> part [CHUNKS][row_len]
// d dt_l / d score_scale_l: the per-workgroup partials of the SUMS target-pass launches (gadapt_block_backward) summed in a
// fixed order - one workgroup per (kind, layer): four interleaved partial sums per thread, wave butterfly, the four waves in
// order.  Replaces float atomics on one address per layer (512 of them per launch: +5 us on the compact-input launch) and
// makes the step / temperature gradients bit-reproducible like everything else.
__device__ __forceinline__ void layer_params_reduce_block(const float* __restrict__ partials, int n_rows, int n_layers, int want_scale,
                                                          float* __restrict__ out, int slot /* kind * L + l */) {
    __shared__ float red[4];
    float v = 0.f;
    if (slot < n_layers || want_scale) {
        const float* src = partials + (size_t)slot * n_rows;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
        for (int r = threadIdx.x; r < n_rows; r += 1024) {
            v0 += src[r];
            if (r + 256 < n_rows) v1 += src[r + 256];
            if (r + 512 < n_rows) v2 += src[r + 512];
            if (r + 768 < n_rows) v3 += src[r + 768];
        }
        v = (v0 + v1) + (v2 + v3);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) out[slot] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void layer_params_reduce_kernel(const float* __restrict__ partials, int n_rows, int n_layers, int want_scale,
                                                                  float* __restrict__ out) {
    layer_params_reduce_block(partials, n_rows, n_layers, want_scale, out, blockIdx.x);
}
// Workgroups past the row's column blocks (blockIdx.x >= nbx, first chunk row only) sum the d dt / d score_scale partials of the
// same backward instead (lp_*: optional; see layer_params_reduce_block) - they ride in this launch rather than in one of their own.
// ... and one more (the last of the row; fused training step, gadapt_step_tail) advances the optimizer's device step count
// (step_state) and sums the loss partials of the step's forward (loss_*: optional; LossArgs in
// gadapt_common.inc): loss_out[0] = loss_scale * sum, four interleaved partial sums per thread, wave butterfly, the four waves in order.
__global__ void slab_reduce1_kernel(const float* slab, float* part, int n_rows, int row_len, int nbx = 1 << 30,
                                    const float* lp_partials = nullptr, int n_layers = 0, int want_scale = 0, float* lp_out = nullptr,
                                    const float* loss_partials = nullptr, int n_loss = 0, float loss_scale = 0.f, float* loss_out = nullptr,
                                    int* step_state = nullptr) {
    if ((int)blockIdx.x >= nbx) {
        const int extra = (int)blockIdx.x - nbx, n_lp = lp_partials ? 2 * n_layers : 0;
        if (blockIdx.y != 0) return;
        if (extra < n_lp) { layer_params_reduce_block(lp_partials, n_rows, n_layers, want_scale, lp_out, extra); return; }
        if (extra == n_lp && step_state && threadIdx.x == 0) step_state[0] += 1;   // fused step: the count step_tail_kernel reads (one thread of the launch)
        if (loss_partials && extra == n_lp) {
            __shared__ float lred[4];
            float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
            for (int r = threadIdx.x; r < n_loss; r += 1024) {
                v0 += loss_partials[r];
                if (r + 256 < n_loss) v1 += loss_partials[r + 256];
                if (r + 512 < n_loss) v2 += loss_partials[r + 512];
                if (r + 768 < n_loss) v3 += loss_partials[r + 768];
            }
            float v = (v0 + v1) + (v2 + v3);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if ((threadIdx.x & 63) == 0) lred[threadIdx.x >> 6] = v;
            __syncthreads();
            if (threadIdx.x == 0) loss_out[0] = ((lred[0] + lred[1]) + (lred[2] + lred[3])) * loss_scale;
        }
        return;
    }
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= row_len) return;
    const int per = (n_rows + GADAPT_SLAB_CHUNKS - 1) / GADAPT_SLAB_CHUNKS;
    const int r0 = blockIdx.y * per, r1 = min(n_rows, r0 + per);
    // 32 rows in flight per thread, four partial sums (fixed order): the kernel is a handful of memory round trips long
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    int r = r0;
    for (; r + 32 <= r1; r += 32) {
        float t[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) t[k] = slab[(size_t)(r + k) * row_len + e];
#pragma unroll
        for (int k = 0; k < 32; k += 4) { v0 += t[k]; v1 += t[k + 1]; v2 += t[k + 2]; v3 += t[k + 3]; }
    }
    for (; r < r1; ++r) v0 += slab[(size_t)r * row_len + e];
    part[(size_t)blockIdx.y * row_len + e] = (v0 + v1) + (v2 + v3);
}
__global__ void slab_reduce2_kernel(const float* part, float* d_a, float* d_p0, int c) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int row_len = c * c + c;
    if (e >= row_len) return;
    float v = 0.f;
    for (int k = 0; k < GADAPT_SLAB_CHUNKS; ++k) v += part[(size_t)k * row_len + e];
    if (e < c * c) d_a[e] = v; else d_p0[e - c * c] = v;
}

// part [CHUNKS][C*C+C] -> (dA, dp0) in LDS -> dWq | dbq | dWk | dbk: the second level of the slab reduction and the chain
// rule of coeffs_bwd_kernel in ONE launch.  Every workgroup adds the CHUNKS partial rows itself (fixed order, so all
// workgroups hold bit-identical sums; 0.5 MB of L2-resident reads per workgroup at C = 64) and then produces its share
// of the 2 C^2 + 2 C outputs.  dA rows are padded by one float: the dWk sum walks a column of dA^T.
template <int C>
__global__ __launch_bounds__(1024) void reduce2_coeffs_bwd_kernel(const float* __restrict__ part, const float* __restrict__ wq,
                                                                  const float* __restrict__ bq, const float* __restrict__ wk,
                                                                  float* __restrict__ d_wq, float* __restrict__ d_bq,
                                                                  float* __restrict__ d_wk, float* __restrict__ d_bk) {
    extern __shared__ float4 smem4[];
    float* da = reinterpret_cast<float*>(smem4);                 // [C][C+1]
    float* dp = da + C * (C + 1);                                // [C]
    constexpr int ROW = C * C + C, c2 = C * C;
    // 1024 threads, the CHUNKS loads of an element all in flight: the sums are an L2 round trip per element and thread,
    // not per load (a 256-thread version with an 8-wide unroll took 26.8 us at C = 64: 64 dependent round trips)
    for (int e = threadIdx.x; e < ROW; e += 1024) {
        float t[GADAPT_SLAB_CHUNKS];
#pragma unroll
        for (int k = 0; k < GADAPT_SLAB_CHUNKS; ++k) t[k] = part[(size_t)k * ROW + e];
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < GADAPT_SLAB_CHUNKS; ++k) v += t[k];  // same order as slab_reduce2_kernel
        if (e < c2) da[(e / C) * (C + 1) + (e % C)] = v; else dp[e - c2] = v;
    }
    __syncthreads();
    for (int e = blockIdx.x * 1024 + threadIdx.x; e < 2 * c2 + 2 * C; e += gridDim.x * 1024) {
        if (e < c2) {                       // d_wq[r][cc] = sum_o wk[r][o] dA[o][cc]
            const int r = e / C, cc = e % C;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int o = 0; o < C; ++o) v[o & 3] = fmaf(wk[r * C + o], da[o * (C + 1) + cc], v[o & 3]);
            d_wq[e] = (v[0] + v[1]) + (v[2] + v[3]);
        } else if (e < 2 * c2) {            // d_wk[r][o] = sum_cc wq[r][cc] dA[o][cc] + bq[r] dp0[o]
            const int f = e - c2, r = f / C, o = f % C;
            float v[4] = {bq[r] * dp[o], 0.f, 0.f, 0.f};
#pragma unroll
            for (int cc = 0; cc < C; ++cc) v[cc & 3] = fmaf(wq[r * C + cc], da[o * (C + 1) + cc], v[cc & 3]);
            d_wk[f] = (v[0] + v[1]) + (v[2] + v[3]);
        } else if (e < 2 * c2 + C) {        // d_bq[r] = sum_o wk[r][o] dp0[o]
            const int r = e - 2 * c2;
            float v = 0.f;
#pragma unroll
            for (int o = 0; o < C; ++o) v = fmaf(wk[r * C + o], dp[o], v);
            d_bq[r] = v;
        } else {
            d_bk[e - 2 * c2 - C] = 0.f;     // softmax shift invariance: d/d lin_key.bias vanishes identically
        }
    }
}

// Adam update of one element (torch.optim.Adam: L2 weight decay added to the gradient, bias-corrected moments, eps outside the
// sqrt) - ONE definition for adam_step_kernel, adam_step_dev_kernel and step_tail_kernel, so the three produce the same bits.
__device__ __forceinline__ float adam_update(float pv, float g, float& m, float& v, float lr, float b1, float b2, float eps, float wd,
                                             float bc1, float bc2_sqrt) {
    if (wd != 0.f) g = fmaf(wd, pv, g);
    const float mn = fmaf(b1, m, (1.f - b1) * g);
    const float vn = fmaf(b2, v, (1.f - b2) * g * g);
    m = mn; v = vn;
    const float denom = sqrtf(vn) / bc2_sqrt + eps;
    return pv - (lr / bc1) * (mn / denom);
}

// Tail of a fused training step (run_GNN.py:128-131): second level of the slab sums + chain rule (reduce2_coeffs_bwd_kernel's
// arithmetic) + Adam (adam_step_dev_kernel's arithmetic, step count on the device) in ONE launch WITHOUT any exchange between its
// workgroups: a workgroup owns ROWS r of the parameters - Wq[r][:], Wk[r][:], bq[r], bk[r], one entry per thread - and the chain rule
// of exactly those entries reads row r of the OTHER matrix and bq[r], i.e. entries the same workgroup owns:
//     d Wq[r][cc] = sum_o Wk[r][o] dA[o][cc]      d Wk[r][o] = sum_cc Wq[r][cc] dA[o][cc] + bq[r] dp0[o]      d bq[r] = sum_o Wk[r][o] dp0[o]
// so every workgroup stages its rows in LDS, computes its gradient entries, and overwrites its own rows: nothing it reads is written
// by anyone else (dA / dp0 come from `part`).  The next step's composite coefficients need ALL the new weights - a second grid-wide
// exchange - and are a launch of their own (gadapt_step_tail).
// Measured and dropped (MI355X, hidden 64): the same work with the coefficients in the same launch behind grid-wide hand-overs - the
// workgroup that takes the last ticket finishes alone: 22.0 us; two counter barriers between resident workgroups: 28.7 us - against
// 6.2 (sums + chain rule) + 4.2 (Adam) + ~3.5 us (coefficients) as separate launches.  A launch's workgroups are dealt round-robin
// to the eight XCDs, each with its own L2: a device-scope release / acquire inside a kernel writes back and invalidates those L2s and
// costs about what a kernel boundary costs, without a kernel boundary's parallel ramp.
// part == nullptr: the gradient is given (data parallel: the all-reduce ran between the chain rule and this launch).
// state[0] = steps taken INCLUDING this one: advanced by the launch before this one (slab_reduce1_kernel's extra workgroup, or
// step_count_kernel when the gradient is given); an exit ticket here, as in adam_step_dev_kernel, is a device-scope fence per workgroup.
struct TailArgs {
    const float* part; float* param; float* grad; float* m; float* v;
    float lr, b1, b2, eps, wd, gscale;
    int* state;
};
// rows per workgroup: as many as 1024 threads hold (2 C + 2 entries per row), rounded down so that the Wq entries - and with them
// the Wk entries - fill whole waves where they can (hidden 32: 14 rows = 7 waves each): the threads of a wave then all run the SAME
// chain-rule branch (a first layout, row after row, left most waves straddling two or three branches: 10.1 us per launch at hidden 64)
template <int C> static constexpr int tail_rows_per_block() {
    int r = (1024 / (2 * C + 2)) < C ? (1024 / (2 * C + 2)) : C;
    while (r > 1 && C < 64 && (r * C) % 64 != 0 && (r - 1) * C >= 64) --r;
    return r;
}
template <int C> static constexpr int tail_blocks() { return (C + tail_rows_per_block<C>() - 1) / tail_rows_per_block<C>(); }
template <int C> static constexpr int tail_lds_floats() { return C * (C + 1) + C + tail_rows_per_block<C>() * (2 * C + 1); }
template <int C>
__global__ __launch_bounds__(1024) void step_tail_kernel(TailArgs p) {
    extern __shared__ float4 smem4[];
    float* da = reinterpret_cast<float*>(smem4);                 // [C][C+1]
    float* dp = da + C * (C + 1);                                // [C]
    constexpr int R = tail_rows_per_block<C>(), W = 2 * C + 2, c2 = C * C, ROW = c2 + C;
    float* rows = dp + C;                                        // [R][2C+1]: this workgroup's Wq rows, Wk rows, bq entries (old values)
    // thread -> (row of the workgroup, entry of the row): the R C entries of Wq first, then those of Wk, then bq, then bk
    const int t_ = threadIdx.x;
    const int role = t_ < R * C ? 0 : (t_ < 2 * R * C ? 1 : (t_ < 2 * R * C + R ? 2 : 3));
    const int tr = t_ - (role == 0 ? 0 : (role == 1 ? R * C : (role == 2 ? 2 * R * C : 2 * R * C + R)));
    const int ri = role < 2 ? tr / C : tr;
    const int k = role < 2 ? role * C + tr % C : (role == 2 ? 2 * C : 2 * C + 1);
    const int r = blockIdx.x * R + ri;
    const bool live = t_ < 2 * R * C + 2 * R && r < C;
    // this thread's entry of the flat layout [Wq | bq | Wk | bk]
    const int e = !live ? 0 : (k < C ? r * C + k : (k < 2 * C ? c2 + C + r * C + (k - C) : (k == 2 * C ? c2 + r : 2 * c2 + C + r)));
    // Every request of the launch goes out before the first wait (a first version read the step count through one thread and LDS - two
    // dependent scalar trips in front of wave 0's loads - and the partial rows in a loop whose iterations each waited for their own
    // eight loads: five round trips in series, half of the launch's 8.2 us at hidden 64)
    const int step_now = p.state[0];                            // already advanced for this step (slab_reduce1_kernel / step_count_kernel)
    const float pv = p.param[e];
    float mm = p.m[e], vv = p.v[e];
    float g = 0.f;
    float bc1 = 0.f, bc2_sqrt = 0.f;
    auto bias_corrections = [&]() __attribute__((always_inline)) {
        const float stepf = (float)step_now;
        bc1 = 1.0f - powf(p.b1, stepf); bc2_sqrt = sqrtf(1.0f - powf(p.b2, stepf));
    };
    if (p.part) {
        constexpr int NIT = (ROW + 1023) / 1024, NB = 8;           // NB iterations' loads (8 each) in flight: 64 registers at most
#pragma unroll
        for (int it0 = 0; it0 < NIT; it0 += NB) {
            float t[NB][GADAPT_SLAB_CHUNKS];
#pragma unroll
            for (int it = it0; it < it0 + NB && it < NIT; ++it) {
                const int k0 = min(it * 1024 + (int)threadIdx.x, ROW - 1);
#pragma unroll
                for (int q = 0; q < GADAPT_SLAB_CHUNKS; ++q) t[it - it0][q] = p.part[(size_t)q * ROW + k0];
            }
            if (it0 == 0) {                                      // behind the requests, in front of their wait:
                bias_corrections();                              // two powf - 400 instructions that ran after the chain rule, in series
                asm volatile("" : "+v"(bc1), "+v"(bc2_sqrt));    // (... and that hipcc otherwise sinks to their use)
                if (live && k <= 2 * C) rows[ri * (2 * C + 1) + k] = pv;
            }
#pragma unroll
            for (int it = it0; it < it0 + NB && it < NIT; ++it) {
                const int k0 = it * 1024 + (int)threadIdx.x;
                float v = 0.f;
#pragma unroll
                for (int q = 0; q < GADAPT_SLAB_CHUNKS; ++q) v += t[it - it0][q];  // same order as slab_reduce2_kernel
                if (k0 < c2) da[(k0 / C) * (C + 1) + (k0 % C)] = v; else if (k0 < ROW) dp[k0 - c2] = v;
            }
        }
        __syncthreads();
        const float* wq_r = rows + ri * (2 * C + 1);             // Wq[r][:]
        const float* wk_r = wq_r + C;                            // Wk[r][:]
        if (!live) {
        } else if (k < C) {                     // d_wq[r][cc] = sum_o wk[r][o] dA[o][cc]
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int o = 0; o < C; ++o) v[o & 3] = fmaf(wk_r[o], da[o * (C + 1) + k], v[o & 3]);
            g = (v[0] + v[1]) + (v[2] + v[3]);
        } else if (k < 2 * C) {                 // d_wk[r][o] = sum_cc wq[r][cc] dA[o][cc] + bq[r] dp0[o]
            const int o = k - C;
            float v[4] = {wq_r[2 * C] * dp[o], 0.f, 0.f, 0.f};
#pragma unroll
            for (int cc = 0; cc < C; ++cc) v[cc & 3] = fmaf(wq_r[cc], da[o * (C + 1) + cc], v[cc & 3]);
            g = (v[0] + v[1]) + (v[2] + v[3]);
        } else if (k == 2 * C) {                // d_bq[r] = sum_o wk[r][o] dp0[o]
            float v = 0.f;
#pragma unroll
            for (int o = 0; o < C; ++o) v = fmaf(wk_r[o], dp[o], v);
            g = v;
        }                                       // k == 2C+1: d_bk = 0 (softmax shift invariance: d/d lin_key.bias vanishes identically)
        if (live) p.grad[e] = g;
    } else {
        g = p.grad[e];
        bias_corrections();
    }
    if (live) {
        const float pn = adam_update(pv, g * p.gscale, mm, vv, p.lr, p.b1, p.b2, p.eps, p.wd, bc1, bc2_sqrt);
        p.m[e] = mm; p.v[e] = vv; p.param[e] = pn;
    }
}
__global__ void step_count_kernel(int* state) { if (blockIdx.x == 0 && threadIdx.x == 0) state[0] += 1; }

// Tail of a fused training step on the NARROW route (hidden 64; gadapt_step_tail_narrow): what slab_reduce1_kernel + step_tail_kernel<64>
// (or reduce2_coeffs_bwd_kernel<64>: p.m == nullptr, the flat gradient only) compute from a full-width slab whose rows are zero outside
// the 4 x 4 corner of dA and dp0[0..3], from the PACKED slab [n_rows][GADAPT_NARROW_SLAB_ROW] - the same bits (up to the sign of a zero) in one launch:
//   workgroup 0 (1024 threads): both levels of the slab sums in the two-launch tail's order, the chain-rule terms whose dA / dp0 factor
//     can be non-zero (a dropped term is fmaf(w, 0, v) = v for finite w), Adam on all 2 C^2 + 2 C entries (NE = 9 per thread) and the
//     step count - read, and advanced by thread 0, inside this one workgroup;
//   workgroup 1 (only with loss partials): the loss sum of slab_reduce1_kernel's extra workgroup on its first 256 threads.
// The two share nothing, so the launch has no exchange between workgroups.
// First level: thread (j, q, e) owns interleaved sum v_j of entry e over chunk q's groups of 32 rows (rows j, j+4, .. of each group in
// order; leftover rows one by one into v_0), the four meet in LDS as (v0 + v1) + (v2 + v3); second level: the chunks in ascending order.
struct TailNarrowArgs {
    const float* slab; int n_rows;
    float* param; float* grad; float* m; float* v;
    float lr, b1, b2, eps, wd, gscale;
    int* state;
    const float* loss_partials; int n_loss; float loss_scale; float* loss_out;
};
__global__ __launch_bounds__(1024) void step_tail_narrow_kernel(TailNarrowArgs p) {
    constexpr int C = 64, c2 = C * C, NPAR = 2 * c2 + 2 * C, NE = (NPAR + 1023) / 1024, RW = GADAPT_NARROW_SLAB_ROW, Q = GADAPT_SLAB_CHUNKS;
    static_assert(Q * RW * 4 == 1024, "one thread per (interleaved sum, chunk, entry)");
    __shared__ float part[4][Q * RW];                           // v_j of (chunk, entry)
    __shared__ float sums[RW];                                  // dA[o][c] at 4 o + c, dp0[o] at 16 + o
    __shared__ float wq4[C][4], wk4[C][4], bqs[C];              // old Wq[r][0..3], Wk[r][0..3], bq[r]
    __shared__ float lred[4];
    const int tid = threadIdx.x;
    if (blockIdx.x == 1) {                                      // the loss value: slab_reduce1_kernel's order (256 threads)
        float v = 0.f;
        if (tid < 256) {
            float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
            for (int r = tid; r < p.n_loss; r += 1024) {
                v0 += p.loss_partials[r];
                if (r + 256 < p.n_loss) v1 += p.loss_partials[r + 256];
                if (r + 512 < p.n_loss) v2 += p.loss_partials[r + 512];
                if (r + 768 < p.n_loss) v3 += p.loss_partials[r + 768];
            }
            v = (v0 + v1) + (v2 + v3);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if ((tid & 63) == 0) lred[tid >> 6] = v;
        }
        __syncthreads();
        if (tid == 0) p.loss_out[0] = ((lred[0] + lred[1]) + (lred[2] + lred[3])) * p.loss_scale;
        return;
    }
    const bool adam = p.m != nullptr;
    // Every request of the launch goes out before the first wait (see step_tail_kernel): the step count, this thread's NE entries of
    // param / m / v and the first group of slab rows; the two powf run behind them
    const int step_now = adam ? p.state[0] + 1 : 1;            // steps taken INCLUDING this one
    float pv[NE], mm[NE], vv[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const int e = min(tid + 1024 * i, NPAR - 1);
        pv[i] = p.param[e];
        mm[i] = adam ? p.m[e] : 0.f;
        vv[i] = adam ? p.v[e] : 0.f;
    }
    const int j = tid >> 8, q = (tid >> 5) & (Q - 1), en = tid & (RW - 1);
    const int per = (p.n_rows + Q - 1) / Q;
    const int r0 = q * per, r1 = min(p.n_rows, r0 + per);
    const float* src = p.slab + en;
    float t[8];
    int r = r0;
    const bool first = r + 32 <= r1;
    if (first) {
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = src[(size_t)(r + 4 * k + j) * RW];
    }
    float bc1 = 0.f, bc2_sqrt = 0.f;
    if (adam) {
        const float stepf = (float)step_now;
        bc1 = 1.0f - powf(p.b1, stepf); bc2_sqrt = sqrtf(1.0f - powf(p.b2, stepf));
        asm volatile("" : "+v"(bc1), "+v"(bc2_sqrt));           // (hipcc otherwise sinks them to their use, behind the sums)
    }
    // the rows of the flat bucket the chain rule reads, staged before anyone overwrites them: [Wq | bq | Wk | bk]
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const int e = tid + 1024 * i;
        if (e < c2) { if ((e & (C - 1)) < 4) wq4[e >> 6][e & 3] = pv[i]; }
        else if (e < c2 + C) bqs[e - c2] = pv[i];
        else if (e < 2 * c2 + C) { const int f = e - c2 - C; if ((f & (C - 1)) < 4) wk4[f >> 6][f & 3] = pv[i]; }
    }
    float vj = 0.f;
    if (first) {
#pragma unroll
        for (int k = 0; k < 8; ++k) vj += t[k];
        r += 32;
    }
    for (; r + 32 <= r1; r += 32) {
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = src[(size_t)(r + 4 * k + j) * RW];
#pragma unroll
        for (int k = 0; k < 8; ++k) vj += t[k];
    }
    if (j == 0) for (; r < r1; ++r) vj += src[(size_t)r * RW];
    part[j][q * RW + en] = vj;
    __syncthreads();
    if (tid < Q * RW) part[0][tid] = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    __syncthreads();
    if (tid < RW) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < Q; ++k) v += part[0][k * RW + tid];   // same order as slab_reduce2_kernel
        sums[tid] = v;
    }
    __syncthreads();
    const float* da = sums;                                     // dA[o][cc] = da[4 o + cc]
    const float* dp = sums + 16;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const int e = tid + 1024 * i;
        if (e >= NPAR) break;
        float g = 0.f;
        if (e < c2) {                           // d_wq[r][cc] = sum_o wk[r][o] dA[o][cc]
            const int rr = e >> 6, cc = e & (C - 1);
            if (cc < 4) {
                float v[4];
#pragma unroll
                for (int o = 0; o < 4; ++o) v[o] = fmaf(wk4[rr][o], da[4 * o + cc], 0.f);
                g = (v[0] + v[1]) + (v[2] + v[3]);
            }
        } else if (e < c2 + C) {                // d_bq[r] = sum_o wk[r][o] dp0[o]
            const int rr = e - c2;
            float v = 0.f;
#pragma unroll
            for (int o = 0; o < 4; ++o) v = fmaf(wk4[rr][o], dp[o], v);
            g = v;
        } else if (e < 2 * c2 + C) {            // d_wk[r][o] = sum_cc wq[r][cc] dA[o][cc] + bq[r] dp0[o]
            const int f = e - c2 - C, rr = f >> 6, o = f & (C - 1);
            if (o < 4) {
                float v[4] = {bqs[rr] * dp[o], 0.f, 0.f, 0.f};
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) v[cc] = fmaf(wq4[rr][cc], da[4 * o + cc], v[cc]);
                g = (v[0] + v[1]) + (v[2] + v[3]);
            }
        }                                       // d_bk = 0 (softmax shift invariance: d/d lin_key.bias vanishes identically)
        p.grad[e] = g;
        if (adam) {
            const float pn = adam_update(pv[i], g * p.gscale, mm[i], vv[i], p.lr, p.b1, p.b2, p.eps, p.wd, bc1, bc2_sqrt);
            p.m[e] = mm[i]; p.v[e] = vv[i]; p.param[e] = pn;
        }
    }
    if (adam && tid == 0) p.state[0] = step_now;
}

// The same tail SPREAD over row-owning workgroups (gadapt_tail_plan.h; gadapt_debug_set_narrow_tail_spread): the same bits as
// step_tail_narrow_kernel from gadapt_narrow_tail_wgs() parameter workgroups of T threads and, with loss partials, the loss workgroup as
// the LAST one.  One workgroup ran Adam on all 8320 entries there, nine per thread behind two powf on each of sixteen waves, while 255
// CUs stood idle; here
//   - every parameter workgroup computes the 20 sums itself from the whole packed slab (64 KB at 512 rows, served by L2 / MALL), in
//     step_tail_narrow_kernel's order: thread (chunk q, entry en) of the first 256 holds all four interleaved sums v_j of its chunk
//     (rows r0 + j + 4 m of the full 32-row groups, ascending; leftover rows one by one into v_0), (v0 + v1) + (v2 + v3), then the
//     chunks in ascending order onto +0 - so all workgroups hold bit-identical sums and exchange nothing;
//   - it owns R whole rows of the bucket (one or two entries per thread): the old Wq[r][0..3], Wk[r][0..3], bq[r] its chain rule reads
//     are entries its own threads loaded - staged in LDS - and nothing it reads is written by another workgroup;
//   - the step count: every workgroup reads state[0] with its first loads and uses state[0] + 1.  Behind the barriers that follow
//     the sums - every thread of the workgroup has its count by then - ONE thread takes a ticket in state[1] (adam_step_dev_kernel's);
//     the workgroup whose ticket is the last stores state[1] = 0 and state[0] = step_now.  Every other workgroup took its ticket after
//     its reads, so none reads the new count; nothing is handed from workgroup to workgroup (the ticket orders a READ before a WRITE
//     of one word), so there is no fence, no spin and no barrier across workgroups.  hipcc waits for a returned atomic where it is
//     issued, so the ticket is the LAST thread's: its wave holds the fewest entries (none at the shipped geometry) and waits for the
//     answer while the other waves run the chain rule and Adam.  Gradient only (p.m == nullptr): neither word is touched.
// n_rows <= 512 (at most 64 rows per chunk): all 64 row loads of a thread go out before the first wait, with the step count and the
// param / m / v loads, and the two powf run behind them - once per SIMD at T = 256; more rows: groups of 32 in a loop.
template <int T, int R>
__global__ __launch_bounds__(T) void step_tail_narrow_spread_kernel(TailNarrowArgs p) {
    constexpr int C = 64, RW = GADAPT_NARROW_SLAB_ROW, Q = GADAPT_SLAB_CHUNKS, NS = gadapt_narrow_tail_slots(), NWG = gadapt_narrow_tail_wgs();
    static_assert(C == GADAPT_NARROW_TAIL_C && T == GADAPT_NARROW_TAIL_THREADS && R == GADAPT_NARROW_TAIL_ROWS, "the plan's geometry");
    static_assert(Q * RW == 256 && T % 256 == 0 && T <= 1024, "the first 256 threads: one per (chunk, entry)");
    static_assert(NS >= 1 && NS <= 2, "one or two entries per thread");
    __shared__ float part[Q * RW];                              // (chunk, entry)
    __shared__ float sums[RW];                                  // dA[o][c] at 4 o + c, dp0[o] at 16 + o
    __shared__ float wq4[R][4], wk4[R][4], bqs[R];              // old Wq[r][0..3], Wk[r][0..3], bq[r] of this workgroup's rows
    __shared__ float lred[4];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x == NWG) {                               // the loss value: slab_reduce1_kernel's order (256 threads)
        float v = 0.f;
        if (tid < 256) {
            float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
            for (int r = tid; r < p.n_loss; r += 1024) {
                v0 += p.loss_partials[r];
                if (r + 256 < p.n_loss) v1 += p.loss_partials[r + 256];
                if (r + 512 < p.n_loss) v2 += p.loss_partials[r + 512];
                if (r + 768 < p.n_loss) v3 += p.loss_partials[r + 768];
            }
            v = (v0 + v1) + (v2 + v3);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if ((tid & 63) == 0) lred[tid >> 6] = v;
        }
        __syncthreads();
        if (tid == 0) p.loss_out[0] = ((lred[0] + lred[1]) + (lred[2] + lred[3])) * p.loss_scale;
        return;
    }
    const bool adam = p.m != nullptr;
    const int wg = blockIdx.x;
    // Every request of the launch goes out before the first wait: the step count, this thread's slab rows, its entries of param / m / v.
    // No request sits in a branch of its own (a wait would close the branch): gradient only reads the count and the moments from words
    // that are there - the slab, the parameters - and drops them.  The count is a uniform read of a word nothing has written yet in
    // this launch: it travels on the scalar path and returns on its own counter, not behind the 70 vector requests in front of it.
    const int step_read = *(adam ? const_cast<const int*>(p.state) : reinterpret_cast<const int*>(p.slab));
    const bool summer = tid < Q * RW;
    const int q = (tid >> 5) & (Q - 1), en = tid & (RW - 1);
    const int per = (p.n_rows + Q - 1) / Q;
    const int r0 = q * per, r1 = min(p.n_rows, r0 + per), len = max(r1 - r0, 0);
    const float* src = p.slab + en;
    const bool flat = per <= 64;                                // (uniform) every row of the chunk in flight at once
    float t[64];
    if (summer && flat) {
#pragma unroll
        for (int k = 0; k < 64; ++k) t[k] = src[(size_t)min(r0 + k, p.n_rows - 1) * RW];   // (rows past the chunk: loaded, not added)
    }
    gadapt_tail_entry ent[NS];
    float pv[NS], mm[NS], vv[NS];
    const float* m_src = adam ? p.m : p.param;
    const float* v_src = adam ? p.v : p.param;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        ent[i] = gadapt_narrow_tail_entry(wg, tid, i);
        const int e = ent[i].e >= 0 ? ent[i].e : wg * R * C;   // (a slot that holds nothing reads the workgroup's first entry)
        pv[i] = p.param[e];
        mm[i] = m_src[e];
        vv[i] = v_src[e];
    }
    const int step_now = adam ? step_read + 1 : 1;              // steps taken INCLUDING this one
    float bc1 = 0.f, bc2_sqrt = 0.f;
    if (adam) {
        const float stepf = (float)step_now;
        bc1 = 1.0f - powf(p.b1, stepf); bc2_sqrt = sqrtf(1.0f - powf(p.b2, stepf));
        asm volatile("" : "+v"(bc1), "+v"(bc2_sqrt));           // (hipcc otherwise sinks them to their use, behind the sums)
    }
    if (summer && flat) asm volatile("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]));   // (... and hoists the first additions, with their wait, in front of them)
    // the entries of its rows the chain rule reads, staged before anyone overwrites them
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int k = ent[i].k, ri = ent[i].ri;
        if (ent[i].e < 0) continue;
        if (k < 4) wq4[ri][k] = pv[i];
        else if (k == C) bqs[ri] = pv[i];
        else if (k > C && k < C + 5) wk4[ri][k - C - 1] = pv[i];
    }
    if (summer) {
        float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
        if (flat) {
            if (len == 64) {                                    // two full groups
#pragma unroll
                for (int k = 0; k < 64; k += 4) { v0 += t[k]; v1 += t[k + 1]; v2 += t[k + 2]; v3 += t[k + 3]; }
            } else {                                            // at most one full group, then the leftover rows into v0
                const bool full = len >= 32;
#pragma unroll
                for (int k = 0; k < 32; k += 4) {
                    if (full) { v0 += t[k]; v1 += t[k + 1]; v2 += t[k + 2]; v3 += t[k + 3]; }
                    else {
#pragma unroll
                        for (int kk = k; kk < k + 4; ++kk) if (kk < len) v0 += t[kk];
                    }
                }
#pragma unroll
                for (int k = 32; k < 64; ++k) if (k < len) v0 += t[k];
            }
        } else {
            int r = r0;
            for (; r + 32 <= r1; r += 32) {
#pragma unroll
                for (int k = 0; k < 32; ++k) t[k] = src[(size_t)(r + k) * RW];
#pragma unroll
                for (int k = 0; k < 32; k += 4) { v0 += t[k]; v1 += t[k + 1]; v2 += t[k + 2]; v3 += t[k + 3]; }
            }
            for (; r < r1; ++r) v0 += src[(size_t)r * RW];
        }
        part[tid] = (v0 + v1) + (v2 + v3);
    }
    __syncthreads();
    if (tid < RW) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < Q; ++k) v += part[k * RW + tid];     // same order as slab_reduce2_kernel
        sums[tid] = v;
    }
    __syncthreads();
    int ticket = -1;
    if (adam && tid == T - 1) ticket = __hip_atomic_fetch_add(p.state + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float* da = sums;                                     // dA[o][cc] = da[4 o + cc]
    const float* dp = sums + 16;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int e = ent[i].e, k = ent[i].k, ri = ent[i].ri;
        if (e < 0) continue;
        float g = 0.f;
        if (k < C) {                            // d_wq[r][cc] = sum_o wk[r][o] dA[o][cc]
            if (k < 4) {
                float v[4];
#pragma unroll
                for (int o = 0; o < 4; ++o) v[o] = fmaf(wk4[ri][o], da[4 * o + k], 0.f);
                g = (v[0] + v[1]) + (v[2] + v[3]);
            }
        } else if (k == C) {                    // d_bq[r] = sum_o wk[r][o] dp0[o]
            float v = 0.f;
#pragma unroll
            for (int o = 0; o < 4; ++o) v = fmaf(wk4[ri][o], dp[o], v);
            g = v;
        } else if (k < 2 * C + 1) {             // d_wk[r][o] = sum_cc wq[r][cc] dA[o][cc] + bq[r] dp0[o]
            const int o = k - C - 1;
            if (o < 4) {
                float v[4] = {bqs[ri] * dp[o], 0.f, 0.f, 0.f};
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) v[cc] = fmaf(wq4[ri][cc], da[4 * o + cc], v[cc]);
                g = (v[0] + v[1]) + (v[2] + v[3]);
            }
        }                                       // d_bk = 0 (softmax shift invariance: d/d lin_key.bias vanishes identically)
        p.grad[e] = g;
        if (adam) {
            const float pn = adam_update(pv[i], g * p.gscale, mm[i], vv[i], p.lr, p.b1, p.b2, p.eps, p.wd, bc1, bc2_sqrt);
            p.m[e] = mm[i]; p.v[e] = vv[i]; p.param[e] = pn;
        }
    }
    if (ticket == NWG - 1) {                                    // every parameter workgroup has read the count: advance it
        __hip_atomic_store(p.state + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(p.state, step_now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void mesh_loss_seed_kernel(const float* x_top, const float* target, float* x_phys, float* g_top, float* loss_out,
                                      int64_t n_nodes, int d, int c, int l1, float gscale) {
    __shared__ float red[256];
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float lv = 0.f;
    if (e < n_nodes * c) {
        const int64_t i = e / c;
        const int k = (int)(e % c);
        float g = 0.f;
        if (k < d) {
            const float xv = x_top[e];
            const float diff = xv - target[i * d + k];
            x_phys[i * d + k] = xv;
            const float inv = 1.0f / (float)(n_nodes * d);
            if (l1) { lv = fabsf(diff) * inv; g = (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f)) * inv * gscale; }
            else    { lv = diff * diff * inv; g = 2.0f * diff * inv * gscale; }
        }
        g_top[e] = g;
    }
    red[threadIdx.x] = lv;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0 && red[0] != 0.f) atomicAdd(loss_out, red[0]);
}

// loss = mean((pred - target)^2) or mean(|pred - target|) and seed = d loss / d pred in one launch.  Deterministic:
// per-block partials, then the block that takes the last ticket adds them in index order.  scratch[0] is the ticket
// counter (left at zero), scratch[1..] the partials.
#ifndef GADAPT_LOSS_BLOCKS
#define GADAPT_LOSS_BLOCKS 128      /* every block costs one ticket atomic: 64 / 128 / 256 / 512 blocks measured 10.1 / 8.9 / 10.5 / 15.3 us */
#endif
__global__ __launch_bounds__(256) void loss_forward_kernel(const float* __restrict__ pred, int64_t pred_stride,
                                                           const float* __restrict__ target, int64_t n_rows, int d, int l1,
                                                           float* __restrict__ seed, float* __restrict__ loss_out, float* scratch) {
    __shared__ float red[4];
    __shared__ unsigned ticket;
    const int64_t total = n_rows * d;
    const float inv = 1.0f / (float)total;
    float lv = 0.f;
    // one row per thread and slot, four slots per iteration with every load issued before the first use (rows of `pred`
    // are pred_stride floats apart: each read is its own cache line, so the kernel lives on loads in flight)
    constexpr int R = 4;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x; i0 < n_rows; i0 += R * stride) {
        float pv[R][4], tv[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t i = min(i0 + r * stride, n_rows - 1);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < d) { pv[r][k] = pred[i * pred_stride + k]; tv[r][k] = target[i * d + k]; }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t i = i0 + r * stride;
            if (i >= n_rows) break;
            if (d <= 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k < d) {
                        const float diff = pv[r][k] - tv[r][k];
                        if (l1) { lv += fabsf(diff); seed[i * d + k] = (diff > 0.f ? inv : (diff < 0.f ? -inv : 0.f)); }
                        else    { lv = fmaf(diff, diff, lv); seed[i * d + k] = 2.0f * diff * inv; }
                    }
                }
            } else {
                for (int k = 0; k < d; ++k) {
                    const float diff = pred[i * pred_stride + k] - target[i * d + k];
                    if (l1) { lv += fabsf(diff); seed[i * d + k] = (diff > 0.f ? inv : (diff < 0.f ? -inv : 0.f)); }
                    else    { lv = fmaf(diff, diff, lv); seed[i * d + k] = 2.0f * diff * inv; }
                }
            }
        }
    }
    // fixed-shape tree: butterfly inside each wave, then the four wave sums in order (one barrier instead of eight)
    auto block_sum = [&](float v) __attribute__((always_inline)) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        __syncthreads();                                         // red[] of an earlier call has been read
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        return (red[0] + red[1]) + (red[2] + red[3]);
    };
    const float bsum = block_sum(lv);
    if (threadIdx.x == 0) {
        __hip_atomic_store(scratch + 1 + blockIdx.x, bsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        ticket = atomicAdd(reinterpret_cast<unsigned*>(scratch), 1u);
    }
    __syncthreads();
    if (ticket != gridDim.x - 1) return;
    __threadfence();
    float v = 0.f;
    for (unsigned k = threadIdx.x; k < gridDim.x; k += 256)      // fixed order per thread, then the fixed tree
        v += __hip_atomic_load(scratch + 1 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float total_sum = block_sum(v);
    if (threadIdx.x == 0) {
        loss_out[0] = total_sum * inv;
        *reinterpret_cast<unsigned*>(scratch) = 0u;            // ready for the next launch
    }
}

__global__ void adam_step_kernel(float* param, const float* grad, float* m, float* v, int64_t n, float lr, float b1, float b2,
                                 float eps, float wd, float bc1, float bc2_sqrt, float gscale) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    float mm = m[e], vv = v[e];
    const float pn = adam_update(param[e], grad[e] * gscale, mm, vv, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
    m[e] = mm; v[e] = vv; param[e] = pn;
}

// Same update with the step count kept on the device (state[0] = steps taken, state[1] = exit ticket), so that the
// launch carries no host-side value that changes from step to step and can sit inside a captured hipGraph.  Every
// workgroup reads the count when it starts; the workgroup that exits last (all others have read by then) advances it.
__global__ __launch_bounds__(256) void adam_step_dev_kernel(float* param, const float* grad, float* m, float* v, int64_t n, float lr, float b1,
                                                            float b2, float eps, float wd, int* state, float gscale) {
    __shared__ int s_step;
    if (threadIdx.x == 0) s_step = __hip_atomic_load(state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
    __syncthreads();
    const float stepf = (float)s_step;
    const float bc1 = 1.0f - powf(b1, stepf), bc2_sqrt = sqrtf(1.0f - powf(b2, stepf));
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) {
        float mm = m[e], vv = v[e];
        const float pn = adam_update(param[e], grad[e] * gscale, mm, vv, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
        m[e] = mm; v[e] = vv; param[e] = pn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(state + 1, 1) == (int)gridDim.x - 1) {
            __hip_atomic_store(state + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(state, s_step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
