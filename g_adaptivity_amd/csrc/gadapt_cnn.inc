// gadapt_cnn.inc - the global CNN features of a field (src/feature_extractors.py:6-34: u / max|u|, four 3-tap / 3x3-tap convolutions
// with SELU, average pool) as ONE launch forward and ONE launch backward, one workgroup per mesh, fp32.  Included by gadapt_tu_cnn.hip
// only.  Sizes, LDS layout and limits: gadapt_cnn_plan.h.
//
// LDS images are channel-major planes of (n0 + 2) x (n1 + 2) floats whose border stays zero from the first pass on: a tap that leaves
// the image reads a zero, so no lane tests a bound.  Behind the images lies one table of n0 n1 ints, pixel -> offset of the pixel in a
// plane, filled once: the loops over pixels look their offset up instead of dividing by n1.  A wave works on a UNIT: 64 consecutive pixels (one per lane) x COT output
// channels.  The unit index comes from the wave index through readfirstlane, so every weight address is provably wave-uniform and
// the weights arrive through scalar loads from the caller's parameter tensors ([out][in][taps], Conv1d and Conv2d alike).
//
// Order of operations of one output value: bias, then input channels ascending, then taps ascending (row-major), one fmaf each.
// Every sum over pixels is walked in a fixed order: the bias and weight gradients by ONE lane in ascending order (fp64 accumulator,
// rounded to fp32 once), the pool by the 64 lanes of one wave over strided pixels with a fixed xor butterfly.  No floating-point
// atomics: the same bits on every run and in every batch.
namespace cnn {

constexpr float SELU_ALPHA = 1.6732632423543772848170429916717f;
constexpr float SELU_SCALE = 1.0507009873554804934193349852946f;
constexpr int COT = 4;                                          // output channels of a unit
constexpr int L = GADAPT_CNN_LAYERS;

__device__ __forceinline__ float selu(float z) { return z > 0.0f ? SELU_SCALE * z : (SELU_SCALE * SELU_ALPHA) * expm1f(z); }
// d selu / dz from the ACTIVATION a = selu(z): scale where a > 0, else scale alpha e^z = a + scale alpha
__device__ __forceinline__ float selu_slope(float a) { return a > 0.0f ? SELU_SCALE : a + SELU_SCALE * SELU_ALPHA; }

struct Params { const float* w[L]; const float* b[L]; };
struct FwdArgs { const float* u; const float* umax; Params p; float* feat; float* acts; int n_meshes, n0, n1, mid, out; };
struct BwdArgs {
    const float* u; const float* umax; const float* acts; const float* d_feat; Params p; float* partials;
    int n_meshes, n0, n1, mid, out, poff[L], n_params;
};

template <int DIM> __device__ __forceinline__ int tap_offset(int t, int w2) {
    if constexpr (DIM == 1) return t - 1;
    else return (t / 3 - 1) * w2 + (t % 3 - 1);
}
// The parameters are read-only for the whole launch (the gradients go to buffers of their own): as pointers to the constant address
// space, loads at wave-uniform addresses become scalar loads although the kernel also stores to global memory.
typedef const float __attribute__((address_space(4))) * ConstF;
__device__ __forceinline__ ConstF read_only(const float* p) { return (ConstF)(uintptr_t)p; }
__device__ __forceinline__ int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ int wave_count() { return (int)(blockDim.x >> 6); }

// Zeroes the n_img images at the start of LDS and fills the offset table behind them; the caller's barrier follows.
__device__ __forceinline__ int* clear_images(float* lds, int n_img, int img, int n0, int n1) {
    int* at = reinterpret_cast<int*>(lds + n_img * img);
    for (int i = threadIdx.x; i < n_img * img; i += blockDim.x) lds[i] = 0.0f;
    for (int p = threadIdx.x; p < n0 * n1; p += blockDim.x) {
        const int y = p / n1, x = p - y * n1;
        at[p] = (y + 1) * (n1 + 2) + x + 1;
    }
    return at;
}
// The image of one mesh, normalised, into plane 0 (interior) of img.  One division per pixel by the batch maximum the caller computed.
__device__ __forceinline__ void load_field(float* img, const int* at, const float* u, float umax, int P) {
    for (int p = threadIdx.x; p < P; p += blockDim.x) img[at[p]] = u[p] / umax;
}
// C planes [C][n0 n1] of global memory into the interiors of img's planes
__device__ __forceinline__ void load_planes(float* img, const int* at, const float* src, int C, int P, int p2) {
    for (int c = 0; c < C; ++c)
        for (int p = threadIdx.x; p < P; p += blockDim.x) img[c * p2 + at[p]] = src[(int64_t)c * P + p];
}

// One layer: dst[co] = selu(b[co] + sum_ci sum_t w[co][ci][t] src[ci][p + t]), optionally saved to global memory (save: [cout][P]).
template <int DIM> __device__ __forceinline__ void conv_selu(const float* src, float* dst, const int* at_of, ConstF w, ConstF b, int cin, int cout, int n0, int n1,
                                                             float* save) {
    constexpr int T = DIM == 1 ? 3 : 9;
    const int w2 = n1 + 2, P = n0 * n1, p2 = (n0 + 2) * w2, lane = threadIdx.x & 63;
    const int groups = (cout + COT - 1) / COT, units = groups * ((P + 63) / 64);
    for (int unit = wave_index(); unit < units; unit += wave_count()) {
        const int co0 = __builtin_amdgcn_readfirstlane((unit % groups) * COT), p = (unit / groups) * 64 + lane;
        const bool live = p < P;
        const int at = at_of[live ? p : 0];
        int co[COT];
        float acc[COT];
#pragma unroll
        for (int j = 0; j < COT; ++j) { co[j] = min(co0 + j, cout - 1); acc[j] = b[co[j]]; }
        for (int ci = 0; ci < cin; ++ci) {
            const float* in = src + ci * p2 + at;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const float v = in[tap_offset<DIM>(t, w2)];
#pragma unroll
                for (int j = 0; j < COT; ++j) acc[j] = fmaf(w[(co[j] * cin + ci) * T + t], v, acc[j]);
            }
        }
        if (live) {
#pragma unroll
            for (int j = 0; j < COT; ++j)
                if (co0 + j < cout) {
                    const float a = selu(acc[j]);
                    dst[co[j] * p2 + at] = a;
                    if (save) save[(int64_t)co[j] * P + p] = a;
                }
        }
    }
}

template <int DIM> __global__ void __launch_bounds__(1024) cnn_forward_kernel(const FwdArgs a) {
    extern __shared__ float lds[];
    const int n0 = a.n0, n1 = a.n1, mid = a.mid, out = a.out, mesh = blockIdx.x;
    const int P = n0 * n1, p2 = (n0 + 2) * (n1 + 2), img = p2 * max(mid, out);
    float* src = lds;
    float* dst = lds + img;
    const int* at = clear_images(lds, 2, img, n0, n1);
    __syncthreads();
    load_field(src, at, a.u + (int64_t)mesh * P, a.umax[0], P);
    __syncthreads();
    int64_t saved = 0;
#pragma unroll 1
    for (int l = 0; l < L; ++l) {
        const int cin = l == 0 ? 1 : mid, cout = l == L - 1 ? out : mid;
        float* save = a.acts ? a.acts + saved + (int64_t)mesh * cout * P : nullptr;
        conv_selu<DIM>(src, dst, at, read_only(a.p.w[l]), read_only(a.p.b[l]), cin, cout, n0, n1, save);
        saved += (int64_t)a.n_meshes * cout * P;
        __syncthreads();
        float* t = src; src = dst; dst = t;
    }
    // average pool: one wave per output channel walks the whole plane (the border adds zeros), 64 strided partial sums and a fixed
    // xor butterfly; the same order whatever the batch
    const int lane = threadIdx.x & 63;
    for (int co = wave_index(); co < out; co += wave_count()) {
        float s = 0.0f;
        for (int i = lane; i < p2; i += 64) s += src[co * p2 + i];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) a.feat[(int64_t)mesh * out + co] = s / (float)P;
    }
}

// Backward of one mesh, layers 4 down to 1: X = A_{l-1}, G = dZ_l, N = dA_{l-1} -> dZ_{l-1} (the next layer's G).
template <int DIM> __global__ void __launch_bounds__(1024) cnn_backward_kernel(const BwdArgs a) {
    constexpr int T = DIM == 1 ? 3 : 9;
    extern __shared__ float lds[];
    const int n0 = a.n0, n1 = a.n1, mid = a.mid, out = a.out, mesh = blockIdx.x, lane = threadIdx.x & 63;
    const int w2 = n1 + 2, P = n0 * n1, p2 = (n0 + 2) * w2, img = p2 * max(mid, out);
    float* X = lds;
    float* G = lds + img;
    float* N = lds + 2 * img;
    float* grads = a.partials + (int64_t)mesh * a.n_params;
    const int* at_of = clear_images(lds, 3, img, n0, n1);
    __syncthreads();
    // the pool's backward and the top layer's SELU: dZ_4 = d feat / P * selu'(A_4)
    const int64_t B = a.n_meshes;
    const float* a_top = a.acts + 3 * B * mid * P + (int64_t)mesh * out * P;
    for (int co = 0; co < out; ++co) {
        const float g = a.d_feat[(int64_t)mesh * out + co] / (float)P;
        for (int p = threadIdx.x; p < P; p += blockDim.x) G[co * p2 + at_of[p]] = g * selu_slope(a_top[(int64_t)co * P + p]);
    }
#pragma unroll 1
    for (int l = L - 1; l >= 0; --l) {
        const int cin = l == 0 ? 1 : mid, cout = l == L - 1 ? out : mid;
        if (l == 0) load_field(X, at_of, a.u + (int64_t)mesh * P, a.umax[0], P);
        else load_planes(X, at_of, a.acts + (int64_t)(l - 1) * B * mid * P + (int64_t)mesh * mid * P, mid, P, p2);
        __syncthreads();
        // weight and bias gradients: entry e = (co, ci, tap) of w_l, then co of b_l - the order of the packed parameters.  One lane per
        // entry walks the pixels row by row, with an fp64 accumulator: a serial fp32 sum of several hundred like-signed terms (half of the
        // top layer's dZ are ONE value, d feat / P * scale) drifts by a fraction of an ulp per term - measured 7.5e-6 on the bias
        // gradient at 23 x 23 - where the fp64 sum rounds once.
        const int n_w = cout * cin * T;
        for (int e = threadIdx.x; e < n_w + cout; e += blockDim.x) {
            double s = 0.0;
            if (e < n_w) {
                const int co = e / (cin * T), r = e - co * (cin * T), ci = r / T, t = r - ci * T;
                const float* g = G + co * p2 + w2 + 1;
                const float* x = X + ci * p2 + w2 + 1 + tap_offset<DIM>(t, w2);
                for (int y = 0; y < n0; ++y)
                    for (int xx = 0; xx < n1; ++xx) s = fma((double)g[y * w2 + xx], (double)x[y * w2 + xx], s);
            } else {
                const float* g = G + (e - n_w) * p2 + w2 + 1;
                for (int y = 0; y < n0; ++y)
                    for (int xx = 0; xx < n1; ++xx) s += (double)g[y * w2 + xx];
            }
            grads[a.poff[l] + e] = (float)s;
        }
        // dA_{l-1}[ci][q] = sum_co sum_t w[co][ci][t] dZ[co][q - t], times selu'(A_{l-1}): the next layer's dZ.  No gradient wrt the field.
        if (l > 0) {
            const ConstF w = read_only(a.p.w[l]);
            const int groups = (cin + COT - 1) / COT, units = groups * ((P + 63) / 64);
            for (int unit = wave_index(); unit < units; unit += wave_count()) {
                const int ci0 = __builtin_amdgcn_readfirstlane((unit % groups) * COT), p = (unit / groups) * 64 + lane;
                const bool live = p < P;
                const int at = at_of[live ? p : 0];
                int ci[COT];
                float acc[COT];
#pragma unroll
                for (int j = 0; j < COT; ++j) { ci[j] = min(ci0 + j, cin - 1); acc[j] = 0.0f; }
                for (int co = 0; co < cout; ++co) {
                    const float* g = G + co * p2 + at;
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        const float v = g[-tap_offset<DIM>(t, w2)];
#pragma unroll
                        for (int j = 0; j < COT; ++j) acc[j] = fmaf(w[(co * cin + ci[j]) * T + t], v, acc[j]);
                    }
                }
                if (live) {
#pragma unroll
                    for (int j = 0; j < COT; ++j)
                        if (ci0 + j < cin) N[ci[j] * p2 + at] = acc[j] * selu_slope(X[ci[j] * p2 + at]);
                }
            }
        }
        __syncthreads();
        float* t = G; G = N; N = t;
    }
}

// d_params[j] = sum over meshes of partials[mesh][j], meshes ascending: the fixed-order pass behind the backward launch
__global__ void __launch_bounds__(256) cnn_reduce_kernel(const float* __restrict__ partials, float* __restrict__ d_params, int n_meshes, int n_params) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_params) return;
    float s = partials[j];
    for (int m = 1; m < n_meshes; ++m) s += partials[(int64_t)m * n_params + j];
    d_params[j] = s;
}

}  // namespace cnn
