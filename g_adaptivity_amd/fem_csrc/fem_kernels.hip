// fem_kernels.hip - differentiable P1 FEM tail of loss_type='pde_loss' for gfx950 (include/gadapt_fem.h).
//
// Forward (three launches): load vector, banded Cholesky solve (one wave per mesh, band in LDS), evaluation on the lattice;
// the modular loss adds a fourth, the per-mesh lattice loss and its derivative.  The error norms of an evaluation
// (gadapt_fem_eval_errors) fuse the lattice evaluation with their reduction: sol is never written.
// Backward (four launches): d L / d c from the evaluation, adjoint solve on the kept factor, per-triangle chain rule
// (stiffness, load vector, evaluation), per-node gather.  Every sum runs in a fixed order: results are bit-reproducible.
#include <stdio.h>
#include <string.h>
#include <initializer_list>
#include "fem_common.h"
#include "fem_host.h"

#pragma clang fp contract(off)

using fem::V2;
using fem::ld2;

static thread_local char g_err[256] = "";

// every translation unit of the library reports through this message slot (fem_host.h)
int fem_fail(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

// "<who>: <what>", who being the entry point that refuses
int fem_fail_as(int code, const char* who, const char* what) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return fem_fail(code, msg);
}

int fem_launched(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
        return GADAPT_FEM_E_LAUNCH;
    }
    return GADAPT_FEM_OK;
}

extern "C" int gadapt_fem_abi_version(void) { return GADAPT_FEM_ABI; }
extern "C" const char* gadapt_fem_last_error(void) { return g_err; }
extern "C" int gadapt_fem_simpson_points(void) { return FEM_SIMPSON_N; }
extern "C" int gadapt_fem_lds_budget(void) { return GADAPT_FEM_LDS_BUDGET; }

// ---------------------------------------------------------------------------------------------------- triangle bins
// The evaluation locates lattice points with a per-mesh bin grid over the lattice's square, rebuilt on every call from the
// current coordinates: bit t of bin (i,j) is set when triangle t's bounding box, widened by one bin, overlaps the bin.  A
// point scans the triangles of its bin in increasing id, so overlapping (tangled) triangles are all found, in a fixed order.
#define FEM_NB 16

__host__ __device__ inline int64_t eval_words(int n_tris) { return (n_tris + 31) / 32; }

extern "C" int64_t gadapt_fem_eval_lds_bytes(int n_tris) { return (int64_t)FEM_NB * FEM_NB * eval_words(n_tris) * 4; }

__device__ inline int bin_of(float v, float lo, float scale) {
    float f = floorf((v - lo) * scale);
    f = fminf(fmaxf(f, 0.0f), (float)(FEM_NB - 1));           // NaN -> 0
    return (int)f;
}

// lattice index range [i0, i1] that may hold points of [lo_v, hi_v] (one index of slack each side); empty if i0 > i1
__device__ inline void lattice_range(float lo_v, float hi_v, float lo, float hi, int nlat, int& i0, int& i1) {
    const float inv = (float)(nlat - 1) / (hi - lo);
    float a = floorf((lo_v - lo) * inv) - 1.0f, b = ceilf((hi_v - lo) * inv) + 1.0f;
    a = fminf(fmaxf(a, 0.0f), (float)(nlat - 1));
    b = fminf(fmaxf(b, 0.0f), (float)(nlat - 1));
    i0 = (int)a;
    i1 = (int)b;
}

// ---------------------------------------------------------------------------------------------------- load vector
// RHS_m = u_true(x_m) on the boundary; inside, the 9 x 9 Simpson rule of phim(., m) f over the bounding box of the vertices of
// m's incident triangles (difFEM_2d.py:159-203, :298-309), nested as torchquad applies it: the y rule per x row, then x.
__device__ inline void simpson_box(int m, const int32_t* __restrict__ nt_ptr, const int32_t* __restrict__ nt_idx,
                                   const int32_t* __restrict__ cells, const float* __restrict__ x, float& x0, float& x1,
                                   float& y0, float& y1) {
    x0 = y0 = INFINITY;
    x1 = y1 = -INFINITY;
    for (int e = nt_ptr[m]; e < nt_ptr[m + 1]; ++e) {
        const int t = nt_idx[e] >> 2;
        for (int k = 0; k < 3; ++k) {
            const V2 p = ld2(x, cells[3 * t + k]);
            x0 = fminf(x0, p.x); x1 = fmaxf(x1, p.x);
            y0 = fminf(y0, p.y); y1 = fmaxf(y1, p.y);
        }
    }
}

__global__ void __launch_bounds__(256) fem_rhs_kernel(int n_nodes, const int32_t* __restrict__ cells, const int32_t* __restrict__ node_mesh,
                                                      const int32_t* __restrict__ int_idx, const int32_t* __restrict__ nt_ptr,
                                                      const int32_t* __restrict__ nt_idx, const int32_t* __restrict__ gptr,
                                                      const float* __restrict__ gpar, const float* __restrict__ x, float* __restrict__ rhs) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_nodes) return;
    const int b = node_mesh[m];
    const int g0 = gptr[b], g1 = gptr[b + 1];
    const V2 xm = ld2(x, m);
    if (int_idx[m] < 0) {
        rhs[m] = fem::u_true(xm.x, xm.y, gpar, g0, g1);
        return;
    }
    constexpr int n = FEM_SIMPSON_N;
    float bx0, bx1, by0, by1;
    simpson_box(m, nt_ptr, nt_idx, cells, x, bx0, bx1, by0, by1);
    const float hx3 = (bx1 - bx0) / (float)(n - 1) / 3.0f, hy3 = (by1 - by0) / (float)(n - 1) / 3.0f;
    float row[n];
    for (int i = 0; i < n; ++i) {
        const float px = fem::linspace_at(bx0, bx1, n, i);
        float f[n];
        for (int j = 0; j < n; ++j) {
            const float py = fem::linspace_at(by0, by1, n, j);
            float out;
            const float div = fem::phim_parts(px, py, m, nt_ptr, nt_idx, cells, x, &out);
            f[j] = out / div * fem::forcing(px, py, gpar, g0, g1);
        }
        float s = 0.0f;
        for (int k = 0; k + 2 < n; k += 2) s = s + hy3 * (f[k] + 4.0f * f[k + 1] + f[k + 2]);
        row[i] = s;
    }
    float s = 0.0f;
    for (int k = 0; k + 2 < n; k += 2) s = s + hx3 * (row[k] + 4.0f * row[k + 1] + row[k + 2]);
    rhs[m] = s;
}

// ---------------------------------------------------------------------------------------------------- banded Cholesky
// P_II (= -A_II, SPD: a sum of PSD element terms with |area|) in band storage, row r holding P[r][r-d] at r*(w+1)+d.  One
// wave per mesh; the rank-1 update of column k touches w(w+1)/2 entries, spread over the lanes by a pair table in LDS.
#define FEM_SOLVE_THREADS 64

__device__ inline void band_factor(float* __restrict__ A, const int32_t* __restrict__ pairs, int n, int w) {
    const int lane = threadIdx.x, ld = w + 1, np = w * (w + 1) / 2;
    for (int k = 0; k < n; ++k) {
        const float d = sqrtf(A[k * ld]);
        for (int i = 1 + lane; i <= w && k + i < n; i += FEM_SOLVE_THREADS) A[(k + i) * ld + i] = A[(k + i) * ld + i] / d;
        __syncthreads();
        if (lane == 0) A[k * ld] = d;
        for (int p = lane; p < np; p += FEM_SOLVE_THREADS) {
            const int i = pairs[p] >> 16, j = pairs[p] & 0xffff;
            if (k + i < n) A[(k + i) * ld + (i - j)] -= A[(k + i) * ld + i] * A[(k + j) * ld + j];
        }
        __syncthreads();
    }
}

// L L^T y = b in place (column-oriented substitutions)
__device__ inline void band_solve(const float* __restrict__ A, float* __restrict__ b, int n, int w) {
    const int lane = threadIdx.x, ld = w + 1;
    for (int k = 0; k < n; ++k) {
        const float y = b[k] / A[k * ld];
        for (int i = 1 + lane; i <= w && k + i < n; i += FEM_SOLVE_THREADS) b[k + i] -= A[(k + i) * ld + i] * y;
        if (lane == 0) b[k] = y;
        __syncthreads();
    }
    for (int k = n - 1; k >= 0; --k) {
        const float y = b[k] / A[k * ld];
        for (int j = 1 + lane; j <= w && k - j >= 0; j += FEM_SOLVE_THREADS) b[k - j] -= A[k * ld + j] * y;
        if (lane == 0) b[k] = y;
        __syncthreads();
    }
}

__device__ inline void fill_pairs(int32_t* pairs, int w) {
    for (int i = 1, p = 0; i <= w; ++i)
        for (int j = 1; j <= i; ++j, ++p)
            if ((p % FEM_SOLVE_THREADS) == (int)threadIdx.x) pairs[p] = (i << 16) | j;
}

// element matrix row: P_T[l][k] = area grad(phi_l).grad(phi_k) = r_l.r_k / (2 |D|)  (difFEM_2d.py:66-111)
__device__ inline void tri_geometry(V2 p0, V2 p1, V2 p2, V2 r[3], float& D) {
    r[0] = V2{p1.y - p2.y, p2.x - p1.x};
    r[1] = V2{p2.y - p0.y, p0.x - p2.x};
    r[2] = V2{p0.y - p1.y, p1.x - p0.x};
    D = p0.x * (p1.y - p2.y) + p1.x * (p2.y - p0.y) + p2.x * (p0.y - p1.y);
}

__global__ void __launch_bounds__(FEM_SOLVE_THREADS) fem_factor_kernel(const int32_t* __restrict__ meta, const int32_t* __restrict__ cells,
                                                                       const int32_t* __restrict__ int_idx, const int32_t* __restrict__ int_node,
                                                                       const int32_t* __restrict__ nt_ptr, const int32_t* __restrict__ nt_idx,
                                                                       const float* __restrict__ x, const float* __restrict__ rhs,
                                                                       float* __restrict__ coeffs, float* __restrict__ lfac) {
    extern __shared__ float lds[];
    const int32_t* mt = meta + blockIdx.x * GADAPT_FEM_META;
    const int n = mt[GADAPT_FEM_M_N_INT], w = mt[GADAPT_FEM_M_BAND], io = mt[GADAPT_FEM_M_INT_OFF];
    const int ld = w + 1;
    float* A = lds;
    float* bv = A + n * ld;
    int32_t* pairs = (int32_t*)(bv + n);
    const int lane = threadIdx.x;
    for (int v = mt[GADAPT_FEM_M_NODE_OFF] + lane; v < mt[GADAPT_FEM_M_NODE_OFF] + mt[GADAPT_FEM_M_N_NODES]; v += FEM_SOLVE_THREADS)
        if (int_idx[v] < 0) coeffs[v] = rhs[v];                    // c_B = RHS_B (the identity rows, difFEM_2d.py:358-359)
    fill_pairs(pairs, w);
    // assembly by rows: row r gathers its incident triangles (each lane owns whole rows: no atomics)
    for (int r = lane; r < n; r += FEM_SOLVE_THREADS) {
        for (int d = 0; d < ld; ++d) A[r * ld + d] = 0.0f;
        const int g = int_node[io + r];
        float b = -rhs[g];
        for (int e = nt_ptr[g]; e < nt_ptr[g + 1]; ++e) {
            const int t = nt_idx[e] >> 2, l = nt_idx[e] & 3;
            V2 rr[3];
            float D;
            tri_geometry(ld2(x, cells[3 * t]), ld2(x, cells[3 * t + 1]), ld2(x, cells[3 * t + 2]), rr, D);
            const float inv = 1.0f / (2.0f * fabsf(D));
            for (int k = 0; k < 3; ++k) {
                const int h = cells[3 * t + k];
                const float p = (rr[l].x * rr[k].x + rr[l].y * rr[k].y) * inv;
                const int ih = int_idx[h];
                if (ih < 0) b -= p * rhs[h];
                else if (ih <= r) A[r * ld + (r - ih)] += p;
            }
        }
        bv[r] = b;
    }
    __syncthreads();
    band_factor(A, pairs, n, w);
    band_solve(A, bv, n, w);
    for (int r = lane; r < n; r += FEM_SOLVE_THREADS) coeffs[int_node[io + r]] = bv[r];
    if (!lfac) return;                                             // an evaluation keeps no factor: nothing differentiates through it
    float* out = lfac + mt[GADAPT_FEM_M_BAND_OFF];
    for (int i = lane; i < n * ld; i += FEM_SOLVE_THREADS) out[i] = A[i];
}

// adjoint: P_II mu = gc_I on the kept factor (lambda_I = -mu); mu = 0 on the boundary
__global__ void __launch_bounds__(FEM_SOLVE_THREADS) fem_adjoint_kernel(const int32_t* __restrict__ meta, const int32_t* __restrict__ int_idx,
                                                                        const int32_t* __restrict__ int_node, const float* __restrict__ lfac,
                                                                        const float* __restrict__ gc, float* __restrict__ mu) {
    extern __shared__ float lds[];
    const int32_t* mt = meta + blockIdx.x * GADAPT_FEM_META;
    const int n = mt[GADAPT_FEM_M_N_INT], w = mt[GADAPT_FEM_M_BAND], io = mt[GADAPT_FEM_M_INT_OFF];
    const int ld = w + 1, lane = threadIdx.x;
    float* A = lds;
    float* bv = A + n * ld;
    const float* src = lfac + mt[GADAPT_FEM_M_BAND_OFF];
    for (int i = lane; i < n * ld; i += FEM_SOLVE_THREADS) A[i] = src[i];
    for (int r = lane; r < n; r += FEM_SOLVE_THREADS) bv[r] = gc[int_node[io + r]];
    for (int v = mt[GADAPT_FEM_M_NODE_OFF] + lane; v < mt[GADAPT_FEM_M_NODE_OFF] + mt[GADAPT_FEM_M_N_NODES]; v += FEM_SOLVE_THREADS)
        if (int_idx[v] < 0) mu[v] = 0.0f;
    __syncthreads();
    band_solve(A, bv, n, w);
    for (int r = lane; r < n; r += FEM_SOLVE_THREADS) mu[int_node[io + r]] = bv[r];
}

// ---------------------------------------------------------------------------------------------------- evaluation
#define FEM_EVAL_THREADS 256
#define FEM_EVAL_CHUNKS 8

// the lattice's square and the scale from a coordinate to its bin
struct EvalFrame {
    float lox, hix, loy, hiy, scx, scy;
};

__device__ inline EvalFrame eval_frame(const float* __restrict__ lat_x, const float* __restrict__ lat_y, int nlat) {
    EvalFrame f{lat_x[0], lat_x[nlat - 1], lat_y[0], lat_y[nlat - 1], 0.0f, 0.0f};
    f.scx = (float)FEM_NB / (f.hix - f.lox);
    f.scy = (float)FEM_NB / (f.hiy - f.loy);
    return f;
}

// the bin mask of mesh triangles [t0, t0 + nt) in LDS (W words per bin), by the whole workgroup; ends with a barrier
__device__ inline void build_bin_mask(uint32_t* mask, int W, int t0, int nt, const EvalFrame& f, const int32_t* __restrict__ cells,
                                      const float* __restrict__ x) {
    for (int i = threadIdx.x; i < FEM_NB * FEM_NB * W; i += blockDim.x) mask[i] = 0u;
    __syncthreads();
    for (int t = threadIdx.x; t < nt; t += blockDim.x) {
        const V2 p0 = ld2(x, cells[3 * (t0 + t)]), p1 = ld2(x, cells[3 * (t0 + t) + 1]), p2 = ld2(x, cells[3 * (t0 + t) + 2]);
        const int bx0 = max(bin_of(fminf(fminf(p0.x, p1.x), p2.x), f.lox, f.scx) - 1, 0);
        const int bx1 = min(bin_of(fmaxf(fmaxf(p0.x, p1.x), p2.x), f.lox, f.scx) + 1, FEM_NB - 1);
        const int by0 = max(bin_of(fminf(fminf(p0.y, p1.y), p2.y), f.loy, f.scy) - 1, 0);
        const int by1 = min(bin_of(fmaxf(fmaxf(p0.y, p1.y), p2.y), f.loy, f.scy) + 1, FEM_NB - 1);
        for (int bx = bx0; bx <= bx1; ++bx)
            for (int by = by0; by <= by1; ++by) atomicOr(&mask[(bx * FEM_NB + by) * W + (t >> 5)], 1u << (t & 31));
    }
    __syncthreads();
}

// sol(p) = sum over triangles T containing p, over their vertices v: c_v aux_T(p; v) / repeat(p, v)  (difFEM_2d.py:312-318)
__device__ inline float eval_point(float px, float py, const uint32_t* mask, int W, int t0, const EvalFrame& f,
                                   const int32_t* __restrict__ cells, const int32_t* __restrict__ nt_ptr,
                                   const int32_t* __restrict__ nt_idx, const float* __restrict__ x, const float* __restrict__ coeffs) {
    const uint32_t* bm = mask + (bin_of(px, f.lox, f.scx) * FEM_NB + bin_of(py, f.loy, f.scy)) * W;
    float acc = 0.0f;
    for (int wd = 0; wd < W; ++wd) {
        uint32_t bits = bm[wd];
        while (bits) {
            const int t = t0 + wd * 32 + __builtin_ctz(bits);
            bits &= bits - 1;
            const float ind = fem::inside(px, py, ld2(x, cells[3 * t + 2]), ld2(x, cells[3 * t + 1]), ld2(x, cells[3 * t]));
            if (ind == 0.0f) continue;
            for (int l = 0; l < 3; ++l) {
                int va, vb, vc;
                fem::rotation(cells, t, l, va, vb, vc);
                const float inc = fem::aux_value(px, py, ld2(x, va), ld2(x, vb), ld2(x, vc), ind);
                if (inc == 0.0f) continue;
                const float div = fem::phim_parts(px, py, vc, nt_ptr, nt_idx, cells, x, nullptr);
                acc += coeffs[vc] * (inc / div);
            }
        }
    }
    return acc;
}

__global__ void __launch_bounds__(FEM_EVAL_THREADS) fem_eval_kernel(const int32_t* __restrict__ meta, const int32_t* __restrict__ cells,
                                                                    const int32_t* __restrict__ nt_ptr, const int32_t* __restrict__ nt_idx,
                                                                    const float* __restrict__ x, const float* __restrict__ coeffs,
                                                                    const float* __restrict__ lat_x, const float* __restrict__ lat_y,
                                                                    int nlat, float* __restrict__ sol) {
    extern __shared__ uint32_t mask[];
    const int32_t* mt = meta + blockIdx.x * GADAPT_FEM_META;
    const int t0 = mt[GADAPT_FEM_M_TRI_OFF], nt = mt[GADAPT_FEM_M_N_TRIS];
    const int W = (int)eval_words(nt);
    const EvalFrame f = eval_frame(lat_x, lat_y, nlat);
    build_bin_mask(mask, W, t0, nt, f, cells, x);
    const int Q = nlat * nlat;
    const int q0 = (int)((int64_t)Q * blockIdx.y / gridDim.y), q1 = (int)((int64_t)Q * (blockIdx.y + 1) / gridDim.y);
    for (int q = q0 + threadIdx.x; q < q1; q += FEM_EVAL_THREADS)
        sol[(int64_t)blockIdx.x * Q + q] = eval_point(lat_x[q / nlat], lat_y[q % nlat], mask, W, t0, f, cells, nt_ptr, nt_idx, x, coeffs);
}

// ---------------------------------------------------------------------------------------------------- error norms
// The evaluation fused with the trapezium L1 / L2 norms of e = sol - u_true on the lattice (the reference's
// evaluate_error_np_2d: every cell gives dx dy / 4 to each of its corners, so a lattice point weighs h_x h_y times 1, 1/2 or
// 1/4 inside, on an edge, at a corner).  sol never reaches memory.  Each lane sums its points in increasing index, a wave
// adds its lanes in a fixed butterfly, lane 0 adds the waves in order through LDS and writes the chunk's pair of partial
// sums; fem_err_finish_kernel adds a mesh's chunks in order.  No float atomics: a mesh's result is the same in any batch.
__device__ inline float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(FEM_EVAL_THREADS) fem_eval_err_kernel(const int32_t* __restrict__ meta, const int32_t* __restrict__ cells,
                                                                        const int32_t* __restrict__ nt_ptr, const int32_t* __restrict__ nt_idx,
                                                                        const int32_t* __restrict__ gptr, const float* __restrict__ gpar,
                                                                        const float* __restrict__ x, const float* __restrict__ coeffs,
                                                                        const float* __restrict__ lat_x, const float* __restrict__ lat_y,
                                                                        int nlat, float* __restrict__ partials) {
    extern __shared__ uint32_t mask[];
    const int b = blockIdx.x;
    const int32_t* mt = meta + b * GADAPT_FEM_META;
    const int t0 = mt[GADAPT_FEM_M_TRI_OFF], nt = mt[GADAPT_FEM_M_N_TRIS];
    const int W = (int)eval_words(nt);
    const int g0 = gptr[b], g1 = gptr[b + 1];
    const EvalFrame f = eval_frame(lat_x, lat_y, nlat);
    build_bin_mask(mask, W, t0, nt, f, cells, x);
    const int Q = nlat * nlat;
    const int q0 = (int)((int64_t)Q * blockIdx.y / gridDim.y), q1 = (int)((int64_t)Q * (blockIdx.y + 1) / gridDim.y);
    float s1 = 0.0f, s2 = 0.0f;
    for (int q = q0 + threadIdx.x; q < q1; q += FEM_EVAL_THREADS) {
        const int i = q / nlat, j = q % nlat;
        const float px = lat_x[i], py = lat_y[j];
        const float e = eval_point(px, py, mask, W, t0, f, cells, nt_ptr, nt_idx, x, coeffs) - fem::u_true(px, py, gpar, g0, g1);
        const float w = ((i == 0 || i == nlat - 1) ? 0.5f : 1.0f) * ((j == 0 || j == nlat - 1) ? 0.5f : 1.0f);
        s1 = s1 + w * fabsf(e);
        s2 = s2 + w * (e * e);
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    __syncthreads();                                               // every lane is done with the mask: its first words carry the wave sums
    float* red = reinterpret_cast<float*>(mask);
    constexpr int waves = FEM_EVAL_THREADS / 64;
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = s1;
        red[waves + (threadIdx.x >> 6)] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a1 = red[0], a2 = red[waves];
        for (int k = 1; k < waves; ++k) { a1 = a1 + red[k]; a2 = a2 + red[waves + k]; }
        float* out = partials + ((int64_t)b * gridDim.y + blockIdx.y) * 2;
        out[0] = a1;
        out[1] = a2;
    }
}

__global__ void __launch_bounds__(256) fem_err_finish_kernel(int n_meshes, int chunks, const float* __restrict__ lat_x,
                                                             const float* __restrict__ lat_y, int nlat, const float* __restrict__ partials,
                                                             float* __restrict__ err) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_meshes) return;
    const float hx = (lat_x[nlat - 1] - lat_x[0]) / (float)(nlat - 1), hy = (lat_y[nlat - 1] - lat_y[0]) / (float)(nlat - 1);
    float a1 = 0.0f, a2 = 0.0f;
    for (int k = 0; k < chunks; ++k) {
        a1 = a1 + partials[((int64_t)b * chunks + k) * 2];
        a2 = a2 + partials[((int64_t)b * chunks + k) * 2 + 1];
    }
    err[2 * b] = (hx * hy) * a1;
    err[2 * b + 1] = sqrtf((hx * hy) * a2);
}

// ---------------------------------------------------------------------------------------------------- lattice loss
// The modular loss of mesh b on its lattice, e = sol - u_true (difFEM_2d.py:421-435, :472-476): MSE = mean e^2 (F.mse_loss),
// or torchquad's composite Simpson rule of e^2, nested as it applies it: the y rule along each x row, then the x rule over
// the row sums.  One workgroup per mesh, one lane per lattice row (its sum in column order), lane 0 sums the rows in order.
// g_sol = d loss[b] / d sol for gadapt_fem_backward.
#define FEM_LOSS_THREADS 256

__global__ void __launch_bounds__(FEM_LOSS_THREADS) fem_loss_kernel(const int32_t* __restrict__ gptr, const float* __restrict__ gpar,
                                                                    const float* __restrict__ lat_x, const float* __restrict__ lat_y,
                                                                    int nlat, int reduction, const float* __restrict__ sol,
                                                                    float* __restrict__ loss, float* __restrict__ g_sol) {
    extern __shared__ float rows[];
    const int b = blockIdx.x;
    const int g0 = gptr[b], g1 = gptr[b + 1];
    const int64_t base = (int64_t)b * nlat * nlat;
    const bool simp = reduction == GADAPT_FEM_LOSS_SIMPSON;
    const float hx3 = (lat_x[nlat - 1] - lat_x[0]) / (float)(nlat - 1) / 3.0f;
    const float hy3 = (lat_y[nlat - 1] - lat_y[0]) / (float)(nlat - 1) / 3.0f;
    const float two_over_q = 2.0f / ((float)nlat * (float)nlat);
    for (int i = threadIdx.x; i < nlat; i += FEM_LOSS_THREADS) {
        const float px = lat_x[i];
        const float* s_row = sol + base + (int64_t)i * nlat;
        float* g_row = g_sol + base + (int64_t)i * nlat;
        const float wx = hx3 * fem::simpson_coef(i, nlat);
        float s = 0.0f, f0 = 0.0f, f1 = 0.0f;                  // f0, f1: e^2 at j-2, j-1
        for (int j = 0; j < nlat; ++j) {
            const float e = s_row[j] - fem::u_true(px, lat_y[j], gpar, g0, g1);
            const float f = e * e;
            if (simp) {
                g_row[j] = 2.0f * e * (wx * (hy3 * fem::simpson_coef(j, nlat)));
                if (j > 0 && !(j & 1)) s = s + hy3 * (f0 + 4.0f * f1 + f);
                f0 = f1;
                f1 = f;
            } else {
                g_row[j] = e * two_over_q;
                s = s + f;
            }
        }
        rows[i] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float tot = 0.0f;
        if (simp) {
            for (int k = 0; k + 2 < nlat; k += 2) tot = tot + hx3 * (rows[k] + 4.0f * rows[k + 1] + rows[k + 2]);
        } else {
            for (int i = 0; i < nlat; ++i) tot = tot + rows[i];
            tot = tot / ((float)nlat * (float)nlat);
        }
        loss[b] = tot;
    }
}

// ---------------------------------------------------------------------------------------------------- backward
// gc[v] = g_coeffs[v] + sum_p g_sol[p] phim(p, v): v's incident triangles, the lattice points of each one's bounding box
__global__ void __launch_bounds__(256) fem_gc_kernel(int n_nodes, const int32_t* __restrict__ cells, const int32_t* __restrict__ node_mesh,
                                                     const int32_t* __restrict__ nt_ptr, const int32_t* __restrict__ nt_idx,
                                                     const float* __restrict__ x, const float* __restrict__ lat_x, const float* __restrict__ lat_y,
                                                     int nlat, const float* __restrict__ g_coeffs, const float* __restrict__ g_sol,
                                                     float* __restrict__ gc) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_nodes) return;
    float acc = g_coeffs ? g_coeffs[v] : 0.0f;
    if (g_sol) {
        const float* gs = g_sol + (int64_t)node_mesh[v] * nlat * nlat;
        for (int e = nt_ptr[v]; e < nt_ptr[v + 1]; ++e) {
            const int t = nt_idx[e] >> 2, l = nt_idx[e] & 3;
            int va, vb, vc;
            fem::rotation(cells, t, l, va, vb, vc);
            const V2 a = ld2(x, va), b = ld2(x, vb), c = ld2(x, vc);
            int i0, i1, j0, j1;
            lattice_range(fminf(fminf(a.x, b.x), c.x), fmaxf(fmaxf(a.x, b.x), c.x), lat_x[0], lat_x[nlat - 1], nlat, i0, i1);
            lattice_range(fminf(fminf(a.y, b.y), c.y), fmaxf(fmaxf(a.y, b.y), c.y), lat_y[0], lat_y[nlat - 1], nlat, j0, j1);
            for (int i = i0; i <= i1; ++i)
                for (int j = j0; j <= j1; ++j) {
                    const float px = lat_x[i], py = lat_y[j];
                    const float ind = fem::inside(px, py, a, b, c);
                    if (ind == 0.0f) continue;
                    const float inc = fem::aux_value(px, py, a, b, c, ind);
                    if (inc == 0.0f) continue;
                    const float div = fem::phim_parts(px, py, v, nt_ptr, nt_idx, cells, x, nullptr);
                    acc += gs[i * nlat + j] * (inc / div);
                }
        }
    }
    gc[v] = acc;
}

__device__ inline void add_rot(V2 g[3], int l, V2 ga, V2 gb, V2 gc) {
    g[l].x += gc.x; g[l].y += gc.y;
    g[(l + 2) % 3].x += ga.x; g[(l + 2) % 3].y += ga.y;
    g[(l + 1) % 3].x += gb.x; g[(l + 1) % 3].y += gb.y;
}

// d L / d (vertices of t): stiffness (through slopes and |area|), load vector (through phim at the fixed Simpson points)
// and evaluation (through phim at the lattice points)
__global__ void __launch_bounds__(256) fem_tri_bwd_kernel(int n_tris, const int32_t* __restrict__ cells, const int32_t* __restrict__ tri_mesh,
                                                          const int32_t* __restrict__ int_idx, const int32_t* __restrict__ nt_ptr,
                                                          const int32_t* __restrict__ nt_idx, const int32_t* __restrict__ gptr,
                                                          const float* __restrict__ gpar, const float* __restrict__ x,
                                                          const float* __restrict__ lat_x, const float* __restrict__ lat_y, int nlat,
                                                          const float* __restrict__ coeffs, const float* __restrict__ mu,
                                                          const float* __restrict__ g_sol, float* __restrict__ tgrad) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tris) return;
    const int b = tri_mesh[t];
    const int vtx[3] = {cells[3 * t], cells[3 * t + 1], cells[3 * t + 2]};
    const V2 p[3] = {ld2(x, vtx[0]), ld2(x, vtx[1]), ld2(x, vtx[2])};
    V2 g[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};

    // stiffness: E = sum_ab Abar_ab r_a.r_b / (2|D|), Abar_ab = dL/dP_ab = lambda_a c_b = -mu_a c_b (0 on boundary rows)
    {
        V2 r[3];
        float D;
        tri_geometry(p[0], p[1], p[2], r, D);
        float Ab[3][3];
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) Ab[a][c] = -mu[vtx[a]] * coeffs[vtx[c]];
        float R = 0.0f;
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) R += Ab[a][c] * (r[a].x * r[c].x + r[a].y * r[c].y);
        const float inv = 1.0f / (2.0f * fabsf(D));
        for (int a = 0; a < 3; ++a) {
            V2 s = {0.f, 0.f};
            for (int c = 0; c < 3; ++c) {
                const float w = Ab[a][c] + Ab[c][a];
                s.x += w * r[c].x;
                s.y += w * r[c].y;
            }
            s.x *= inv; s.y *= inv;
            g[(a + 2) % 3].x += s.y; g[(a + 1) % 3].x -= s.y;
            g[(a + 1) % 3].y += s.x; g[(a + 2) % 3].y -= s.x;
        }
        const float sgn = D > 0.0f ? 1.0f : (D < 0.0f ? -1.0f : 0.0f);
        const float coef = -R * sgn * inv * inv * 2.0f;          // -R sign(D) / (2 D^2)
        for (int k = 0; k < 3; ++k) { g[k].x += coef * r[k].x; g[k].y += coef * r[k].y; }
    }

    // load vector: d L / d RHS_m = lambda_m = -mu_m at each interior vertex m of t; Simpson points are constants
    const int g0 = gptr[b], g1 = gptr[b + 1];
    constexpr int n = FEM_SIMPSON_N;
    for (int l = 0; l < 3; ++l) {
        const int m = vtx[l];
        if (int_idx[m] < 0) continue;
        const float lam = -mu[m];
        int va, vb, vc;
        fem::rotation(cells, t, l, va, vb, vc);
        const V2 a = ld2(x, va), bb = ld2(x, vb), c = ld2(x, vc);
        float bx0, bx1, by0, by1;
        simpson_box(m, nt_ptr, nt_idx, cells, x, bx0, bx1, by0, by1);
        const float hx3 = (bx1 - bx0) / (float)(n - 1) / 3.0f, hy3 = (by1 - by0) / (float)(n - 1) / 3.0f;
        V2 ga = {0.f, 0.f}, gb = {0.f, 0.f}, gcv = {0.f, 0.f};
        for (int i = 0; i < n; ++i) {
            const float px = fem::linspace_at(bx0, bx1, n, i);
            for (int j = 0; j < n; ++j) {
                const float py = fem::linspace_at(by0, by1, n, j);
                const float ind = fem::inside(px, py, a, bb, c);
                if (ind == 0.0f) continue;
                const float div = fem::phim_parts(px, py, m, nt_ptr, nt_idx, cells, x, nullptr);
                const float w = lam * (hx3 * fem::simpson_coef(i, n)) * (hy3 * fem::simpson_coef(j, n)) * fem::forcing(px, py, gpar, g0, g1) / div;
                fem::aux_grad(px, py, a, bb, c, ind * w, ga, gb, gcv);
            }
        }
        add_rot(g, l, ga, gb, gcv);
    }

    // evaluation: lattice points in t's bounding box
    if (g_sol) {
        const float* gs = g_sol + (int64_t)b * nlat * nlat;
        int i0, i1, j0, j1;
        lattice_range(fminf(fminf(p[0].x, p[1].x), p[2].x), fmaxf(fmaxf(p[0].x, p[1].x), p[2].x), lat_x[0], lat_x[nlat - 1], nlat, i0, i1);
        lattice_range(fminf(fminf(p[0].y, p[1].y), p[2].y), fmaxf(fmaxf(p[0].y, p[1].y), p[2].y), lat_y[0], lat_y[nlat - 1], nlat, j0, j1);
        for (int i = i0; i <= i1; ++i)
            for (int j = j0; j <= j1; ++j) {
                const float px = lat_x[i], py = lat_y[j];
                const float ind = fem::inside(px, py, p[2], p[1], p[0]);
                if (ind == 0.0f) continue;
                const float gp = gs[i * nlat + j];
                for (int l = 0; l < 3; ++l) {
                    int va, vb, vc;
                    fem::rotation(cells, t, l, va, vb, vc);
                    const float div = fem::phim_parts(px, py, vc, nt_ptr, nt_idx, cells, x, nullptr);
                    V2 ga = {0.f, 0.f}, gb = {0.f, 0.f}, gcv = {0.f, 0.f};
                    fem::aux_grad(px, py, ld2(x, va), ld2(x, vb), ld2(x, vc), ind * (gp * coeffs[vc] / div), ga, gb, gcv);
                    add_rot(g, l, ga, gb, gcv);
                }
            }
    }
    for (int k = 0; k < 3; ++k) {
        tgrad[6 * t + 2 * k] = g[k].x;
        tgrad[6 * t + 2 * k + 1] = g[k].y;
    }
}

// gx[v] = sum over v's incidences (t, l) of tgrad[t][l]: a gather in the CSR's fixed order
__global__ void __launch_bounds__(256) fem_gather_kernel(int n_nodes, const int32_t* __restrict__ nt_ptr, const int32_t* __restrict__ nt_idx,
                                                         const float* __restrict__ tgrad, float* __restrict__ gx) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_nodes) return;
    float sx = 0.0f, sy = 0.0f;
    for (int e = nt_ptr[v]; e < nt_ptr[v + 1]; ++e) {
        const int t = nt_idx[e] >> 2, l = nt_idx[e] & 3;
        sx += tgrad[6 * t + 2 * l];
        sy += tgrad[6 * t + 2 * l + 1];
    }
    gx[2 * v] = sx;
    gx[2 * v + 1] = sy;
}

// The route for meshes beyond the resident band (band='window') is compiled in this translation unit: its solve and slabbed
// evaluation with their launch plan, then its adjoint solve.  Both call this file's device helpers; the entry points of
// both routes follow below.  The wave-parallel forms come last: the backward's two lattice walks (fem_adjoint='wave'), then
// the resident-band forward's load vector and evaluation (fem_forward='wave').
#include "fem_window_kernels.hip"
#include "fem_window_grad_kernels.hip"
#include "fem_wave_grad_kernels.hip"
#include "fem_wave_fwd_kernels.hip"

// ---------------------------------------------------------------------------------------------------- checks
// Every entry point: fill a FemBatch from the arguments, check (check_batch, make_plan and what only it checks, in the
// order its refusals have always had), then the launch sequences.  Nothing is launched before the last check has passed.
enum : unsigned { NEED_TRI_MESH = 1, NEED_MAX_TRIS = 2, NEED_WORK = 4, NLAT_RANGE = 8 };

// Sizes and pointers in one refusal under the entry point's name - the batch, `required` (the entry point's own buffers),
// and with NEED_WORK the fp64 workspace, present and 8-byte aligned - then the lattice, then with NLAT_RANGE nlat * nlat.
static int check_batch(const char* who, const FemBatch& b, unsigned needs, std::initializer_list<const void*> required,
                       const void* work = nullptr) {
    bool bad = b.B <= 0 || b.N <= 0 || b.T <= 0 || !b.meta || !b.cells || !b.node_mesh || !b.int_idx || !b.int_node || !b.nt_ptr ||
               !b.nt_idx || !b.gptr || !b.gpar || !b.x;
    bad |= (needs & NEED_TRI_MESH) && !b.tri_mesh;
    bad |= (needs & NEED_MAX_TRIS) && b.max_tris <= 0;
    bad |= (needs & NEED_WORK) && (!work || ((uintptr_t)work & 7));
    for (const void* p : required) bad |= !p;
    if (bad) return fem_fail_as(GADAPT_FEM_E_BADARG, who, "null pointer or bad size");
    if (!b.lat_x || !b.lat_y || b.nlat < 2) return fem_fail(GADAPT_FEM_E_BADARG, "evaluation lattice: need lat_x, lat_y and nlat >= 2");
    if ((needs & NLAT_RANGE) && b.nlat > 46340) return fem_fail_as(GADAPT_FEM_E_BADARG, who, "nlat * nlat exceeds the int range");
    return GADAPT_FEM_OK;
}

// what a modular forward checks of its loss arguments, before the shared ones
static int check_loss(const char* who, const FemBatch& b, int reduction, const float* loss, const float* g_sol) {
    if (b.B <= 0 || !loss || !g_sol || (reduction != GADAPT_FEM_LOSS_MSE && reduction != GADAPT_FEM_LOSS_SIMPSON))
        return fem_fail_as(GADAPT_FEM_E_BADARG, who, "null output or unknown reduction");
    if (reduction == GADAPT_FEM_LOSS_SIMPSON && (b.nlat < 3 || !(b.nlat & 1)))
        return fem_fail_as(GADAPT_FEM_E_BADARG, who, "the Simpson rule needs an odd nlat >= 3");
    if (b.nlat > 0 && (int64_t)b.nlat * 4 > GADAPT_FEM_LDS_BUDGET)
        return fem_fail_as(GADAPT_FEM_E_LDS, who, "the lattice's row sums exceed the LDS budget");
    return GADAPT_FEM_OK;
}

// The LDS of a route's launches.  eval: the entry point evaluates on the lattice (else only the solve's share is planned).
static int make_plan(Band band, const char* who, const FemBatch& b, int tri_slab, bool eval, FemPlan* P) {
    if (band == Band::window)
        return eval ? win_plan(who, b.nlat, b.max_lds_bytes, b.max_tris, tri_slab, P) : win_ring_plan(b.max_lds_bytes, &P->solve_lds);
    if (b.max_lds_bytes <= 0 || b.max_lds_bytes > GADAPT_FEM_LDS_BUDGET)
        return fem_fail(GADAPT_FEM_E_LDS, "band factor: LDS bytes outside (0, GADAPT_FEM_LDS_BUDGET]");
    P->solve_lds = b.max_lds_bytes;
    P->eval_lds = eval ? gadapt_fem_eval_lds_bytes(b.max_tris) : 0;
    P->slab = 0;
    if (P->eval_lds > GADAPT_FEM_LDS_BUDGET) return fem_fail(GADAPT_FEM_E_LDS, "evaluation: triangle bin mask exceeds the LDS budget");
    return GADAPT_FEM_OK;
}

// ---------------------------------------------------------------------------------------------------- launch sequences
// Each takes the stream as `s` (FEM_LAUNCH) and returns at the first launch that fails.
// load vector and banded Cholesky solve -> coeffs; the factor goes to sc.factor (Band::lds: may be NULL, it is not kept then).
// wave (Band::lds alone): the load vector as a wave per node (fem_wave_fwd_kernels.hip), the same bits
static int launch_solve(Band band, const FemBatch& b, const FemPlan& P, const FemScratch& sc, hipStream_t s, bool wave = false) {
    const int nb = (b.N + 255) / 256;
    if (band == Band::window) {
        FEM_LAUNCH(fem_window_rhs_kernel, nb, 256, 0, b.N, b.cells, b.node_mesh, b.int_idx, b.nt_ptr, b.nt_idx, b.gptr, b.gpar, b.x, sc.rhs);
        FEM_LAUNCH(fem_window_solve_kernel, b.B, FEM_WIN_THREADS, (size_t)P.solve_lds, b.meta, b.cells, b.int_idx, b.int_node, b.nt_ptr, b.nt_idx,
                   b.x, sc.rhs, sc.coeffs, reinterpret_cast<double*>(sc.factor), (int)P.solve_lds);
    } else {
        if (wave)
            FEM_LAUNCH(fem_rhs_wave_kernel, b.N, FEM_WAVE, 0, b.N, b.cells, b.node_mesh, b.int_idx, b.nt_ptr, b.nt_idx, b.gptr, b.gpar, b.x, sc.rhs);
        else
            FEM_LAUNCH(fem_rhs_kernel, nb, 256, 0, b.N, b.cells, b.node_mesh, b.int_idx, b.nt_ptr, b.nt_idx, b.gptr, b.gpar, b.x, sc.rhs);
        FEM_LAUNCH(fem_factor_kernel, b.B, FEM_SOLVE_THREADS, (size_t)P.solve_lds, b.meta, b.cells, b.int_idx, b.int_node, b.nt_ptr, b.nt_idx, b.x,
                   sc.rhs, sc.coeffs, sc.factor);
    }
    return GADAPT_FEM_OK;
}

// the solution on the lattice -> sol.  wave (Band::lds alone): a wave per chunk, two phases per point, the same bits and
// the same LDS (the bin mask)
static int launch_eval(Band band, const FemBatch& b, const FemPlan& P, const float* coeffs, float* sol, hipStream_t s, bool wave = false) {
    const dim3 grid(b.B, FEM_EVAL_CHUNKS);
    if (band == Band::window)
        FEM_LAUNCH(fem_eval_slab_kernel, grid, FEM_EVAL_THREADS, (size_t)P.eval_lds, b.meta, b.cells, b.nt_ptr, b.nt_idx, b.x, coeffs, b.lat_x,
                   b.lat_y, b.nlat, P.slab, sol);
    else if (wave)
        FEM_LAUNCH(fem_eval_wave_kernel, dim3(b.B, eval_wave_chunks(b.B, b.nlat)), FEM_WAVE, (size_t)P.eval_lds, b.meta, b.cells, b.nt_ptr, b.nt_idx,
                   b.x, coeffs, b.lat_x, b.lat_y, b.nlat, sol);
    else
        FEM_LAUNCH(fem_eval_kernel, grid, FEM_EVAL_THREADS, (size_t)P.eval_lds, b.meta, b.cells, b.nt_ptr, b.nt_idx, b.x, coeffs, b.lat_x, b.lat_y,
                   b.nlat, sol);
    return GADAPT_FEM_OK;
}

// the lattice evaluation fused with the two error norms' chunk partials, then their sum -> err.  sol_work (Band::lds alone,
// gadapt_fem_eval_errors_wave): the wave evaluation into it, then the lane kernel's sums read from it, the same partials
static int launch_eval_errors(Band band, const FemBatch& b, const FemPlan& P, const float* coeffs, float* partials, float* err, hipStream_t s,
                              float* sol_work = nullptr) {
    const dim3 grid(b.B, FEM_EVAL_CHUNKS);
    if (band == Band::window)
        FEM_LAUNCH(fem_eval_err_slab_kernel, grid, FEM_EVAL_THREADS, (size_t)P.eval_lds, b.meta, b.cells, b.nt_ptr, b.nt_idx, b.gptr, b.gpar, b.x,
                   coeffs, b.lat_x, b.lat_y, b.nlat, P.slab, partials);
    else if (sol_work) {
        if (int rc = launch_eval(band, b, P, coeffs, sol_work, s, true)) return rc;
        FEM_LAUNCH(fem_err_lattice_kernel, grid, FEM_EVAL_THREADS, 0, b.gptr, b.gpar, b.lat_x, b.lat_y, b.nlat, sol_work, partials);
    } else
        FEM_LAUNCH(fem_eval_err_kernel, grid, FEM_EVAL_THREADS, (size_t)P.eval_lds, b.meta, b.cells, b.nt_ptr, b.nt_idx, b.gptr, b.gpar, b.x, coeffs,
                   b.lat_x, b.lat_y, b.nlat, partials);
    FEM_LAUNCH(fem_err_finish_kernel, (b.B + 255) / 256, 256, 0, b.B, FEM_EVAL_CHUNKS, b.lat_x, b.lat_y, b.nlat, partials, err);
    return GADAPT_FEM_OK;
}

static int launch_forward(Band band, const FemBatch& b, const FemPlan& P, const FemScratch& sc, float* sol, hipStream_t s, bool wave = false) {
    const int rc = launch_solve(band, b, P, sc, s, wave);
    return rc ? rc : launch_eval(band, b, P, sc.coeffs, sol, s, wave);
}

int fem_launch_modular_forward(Band band, const FemBatch& b, const FemPlan& P, const FemScratch& sc, int reduction, float* sol, float* loss,
                               float* g_sol, hipStream_t s, bool wave) {
    const int rc = launch_forward(band, b, P, sc, sol, s, wave);
    if (rc) return rc;
    FEM_LAUNCH(fem_loss_kernel, b.B, FEM_LOSS_THREADS, (size_t)b.nlat * 4, b.gptr, b.gpar, b.lat_x, b.lat_y, b.nlat, reduction, sol, loss, g_sol);
    return GADAPT_FEM_OK;
}

int fem_launch_backward(Band band, const FemBatch& b, const FemPlan& P, const FemScratch& sc, const float* g_coeffs, const float* g_sol,
                        const FemAdjoint& a, hipStream_t s, bool wave) {
    const int nb = (b.N + 255) / 256;
    if (wave)                                                      // a wave per node (fem_wave_grad_kernels.hip): the same bits
        FEM_LAUNCH(fem_gc_wave_kernel, b.N, FEM_WAVE, 0, b.N, b.cells, b.node_mesh, b.nt_ptr, b.nt_idx, b.x, b.lat_x, b.lat_y, b.nlat, g_coeffs,
                   g_sol, a.gc);
    else
        FEM_LAUNCH(fem_gc_kernel, nb, 256, 0, b.N, b.cells, b.node_mesh, b.nt_ptr, b.nt_idx, b.x, b.lat_x, b.lat_y, b.nlat, g_coeffs, g_sol, a.gc);
    if (band == Band::window)
        FEM_LAUNCH(fem_window_adjoint_kernel, b.B, FEM_WIN_THREADS, (size_t)P.solve_lds, b.meta, b.int_idx, b.int_node, a.gc, a.mu,
                   reinterpret_cast<double*>(sc.factor), (int)P.solve_lds);
    else
        FEM_LAUNCH(fem_adjoint_kernel, b.B, FEM_SOLVE_THREADS, (size_t)P.solve_lds, b.meta, b.int_idx, b.int_node, sc.factor, a.gc, a.mu);
    if (wave)                                                      // a wave per triangle
        FEM_LAUNCH(fem_tri_bwd_wave_kernel, b.T, FEM_WAVE, 0, b.T, b.cells, b.tri_mesh, b.int_idx, b.nt_ptr, b.nt_idx, b.gptr, b.gpar, b.x,
                   b.lat_x, b.lat_y, b.nlat, sc.coeffs, a.mu, g_sol, a.tgrad);
    else
        FEM_LAUNCH(fem_tri_bwd_kernel, (b.T + 255) / 256, 256, 0, b.T, b.cells, b.tri_mesh, b.int_idx, b.nt_ptr, b.nt_idx, b.gptr, b.gpar, b.x,
                   b.lat_x, b.lat_y, b.nlat, sc.coeffs, a.mu, g_sol, a.tgrad);
    FEM_LAUNCH(fem_gather_kernel, nb, 256, 0, b.N, b.nt_ptr, b.nt_idx, a.tgrad, a.gx);
    return GADAPT_FEM_OK;
}

// ---------------------------------------------------------------------------------------------------- C-ABI
extern "C" int gadapt_fem_eval_partials_floats(int n_meshes) { return n_meshes > 0 ? n_meshes * FEM_EVAL_CHUNKS * 2 : 0; }

// One function per operation: the checks in the order the entry points' refusals have, then the launch sequence.  A late check
// that only one route reaches (the other has refused the same thing earlier) is written once, without an `if`.
// Band::lds refuses lfac and sol only after the LDS, and puts no upper limit on nlat.
static int check_forward(Band band, const char* who, const FemBatch& b, const FemScratch& sc, int tri_slab, const float* sol, FemPlan* P) {
    int rc = band == Band::window ? check_batch(who, b, NEED_MAX_TRIS | NEED_WORK | NLAT_RANGE, {sc.rhs, sc.coeffs, sol}, sc.factor)
                                  : check_batch(who, b, NEED_MAX_TRIS, {sc.rhs, sc.coeffs});
    if (rc || (rc = make_plan(band, who, b, tri_slab, true, P))) return rc;
    return !sc.factor || !sol ? fem_fail_as(GADAPT_FEM_E_BADARG, who, "null pointer or bad size") : GADAPT_FEM_OK;
}

// wave: the *_wave entry points (Band::lds), the same checks and the wave-parallel load vector and evaluation
static int forward(Band band, const char* who, const FemBatch& b, const FemScratch& sc, int tri_slab, float* sol, hipStream_t s, bool wave = false) {
    FemPlan P;
    const int rc = check_forward(band, who, b, sc, tri_slab, sol, &P);
    return rc ? rc : launch_forward(band, b, P, sc, sol, s, wave);
}

// the loss arguments first; Band::lds has always reported the shared ones under gadapt_fem_forward's name, with `wave` too
static int modular_forward(Band band, const char* who, const FemBatch& b, const FemScratch& sc, int reduction, int tri_slab, float* sol,
                           float* loss, float* g_sol, hipStream_t s, bool wave = false) {
    FemPlan P;
    int rc = check_loss(who, b, reduction, loss, g_sol);
    if (rc || (rc = check_forward(band, band == Band::lds ? "gadapt_fem_forward" : who, b, sc, tri_slab, sol, &P))) return rc;
    return fem_launch_modular_forward(band, b, P, sc, reduction, sol, loss, g_sol, s, wave);
}

// Band::lds takes a NULL lfac (the factor is not kept), refuses partials and err only after the LDS, and nlat's range last.
// wave: gadapt_fem_eval_errors_wave (Band::lds), the same checks, sol_work refused with partials and err, and the
// wave-parallel load vector and evaluation
static int eval_errors(Band band, const char* who, const FemBatch& b, const FemScratch& sc, int tri_slab, float* partials, float* err,
                       hipStream_t s, bool wave = false, float* sol_work = nullptr) {
    FemPlan P;
    int rc = band == Band::window ? check_batch(who, b, NEED_MAX_TRIS | NEED_WORK | NLAT_RANGE, {sc.rhs, sc.coeffs, partials, err}, sc.factor)
                                  : check_batch(who, b, NEED_MAX_TRIS, {sc.rhs, sc.coeffs});
    if (rc || (rc = make_plan(band, who, b, tri_slab, true, &P))) return rc;
    if (!partials || !err || (wave && !sol_work)) return fem_fail_as(GADAPT_FEM_E_BADARG, who, "null pointer or bad size");
    if (b.nlat > 46340) return fem_fail_as(GADAPT_FEM_E_BADARG, who, "nlat * nlat exceeds the int range");
    if ((rc = launch_solve(band, b, P, sc, s, wave))) return rc;
    return launch_eval_errors(band, b, P, sc.coeffs, partials, err, s, wave ? sol_work : nullptr);
}

// sc.coeffs and, on Band::lds, sc.factor are only read; g_coeffs and g_sol may be NULL (no gradient flows in through them).
// wave: the *_wave entry points, the same checks and the wave-parallel lattice walks.
static int backward(Band band, const char* who, const FemBatch& b, const FemScratch& sc, const float* g_coeffs, const float* g_sol,
                    const FemAdjoint& a, hipStream_t s, bool wave = false) {
    FemPlan P;
    int rc = check_batch(who, b, NEED_TRI_MESH | (band == Band::window ? NEED_WORK : 0), {sc.coeffs, sc.factor, a.gc, a.mu, a.tgrad, a.gx},
                         sc.factor);
    if (rc || (rc = make_plan(band, who, b, 0, false, &P))) return rc;
    return fem_launch_backward(band, b, P, sc, g_coeffs, g_sol, a, s, wave);
}

// The entry points fill the batch and the scratch from their positional arguments and do nothing else with them.
extern "C" int gadapt_fem_forward(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                  const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr, const int32_t* nt_idx,
                                  const int32_t* gptr, const float* gpar, const float* x, const float* lat_x, const float* lat_y, int nlat,
                                  int max_lds_bytes, int max_tris, float* rhs, float* coeffs, float* lfac, float* sol, void* stream) {
    return forward(Band::lds, "gadapt_fem_forward", FEM_BATCH(nullptr, max_tris), {rhs, coeffs, lfac}, 0, sol, (hipStream_t)stream);
}

extern "C" int gadapt_fem_forward_window(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                         const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr, const int32_t* nt_idx,
                                         const int32_t* gptr, const float* gpar, const float* x, const float* lat_x, const float* lat_y,
                                         int nlat, int max_lds_bytes, int max_tris, float* rhs, float* coeffs, float* work, int tri_slab,
                                         float* sol, void* stream) {
    return forward(Band::window, "gadapt_fem_forward_window", FEM_BATCH(nullptr, max_tris), {rhs, coeffs, work}, tri_slab, sol, (hipStream_t)stream);
}

extern "C" int gadapt_fem_eval_errors(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                      const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr, const int32_t* nt_idx,
                                      const int32_t* gptr, const float* gpar, const float* x, const float* lat_x, const float* lat_y, int nlat,
                                      int max_lds_bytes, int max_tris, float* rhs, float* coeffs, float* lfac, float* partials, float* err,
                                      void* stream) {
    return eval_errors(Band::lds, "gadapt_fem_eval_errors", FEM_BATCH(nullptr, max_tris), {rhs, coeffs, lfac}, 0, partials, err, (hipStream_t)stream);
}

extern "C" int gadapt_fem_eval_errors_window(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                             const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                                             const int32_t* nt_idx, const int32_t* gptr, const float* gpar, const float* x,
                                             const float* lat_x, const float* lat_y, int nlat, int max_lds_bytes, int max_tris, float* rhs,
                                             float* coeffs, float* work, int tri_slab, float* partials, float* err, void* stream) {
    return eval_errors(Band::window, "gadapt_fem_eval_errors_window", FEM_BATCH(nullptr, max_tris), {rhs, coeffs, work}, tri_slab, partials, err,
                       (hipStream_t)stream);
}

extern "C" int gadapt_fem_modular_forward(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                          const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr, const int32_t* nt_idx,
                                          const int32_t* gptr, const float* gpar, const float* x, const float* lat_x, const float* lat_y,
                                          int nlat, int max_lds_bytes, int max_tris, int reduction, float* rhs, float* coeffs, float* lfac,
                                          float* sol, float* loss, float* g_sol, void* stream) {
    return modular_forward(Band::lds, "gadapt_fem_modular_forward", FEM_BATCH(nullptr, max_tris), {rhs, coeffs, lfac}, reduction, 0, sol, loss, g_sol,
                           (hipStream_t)stream);
}

extern "C" int gadapt_fem_modular_forward_window(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                                 const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                                                 const int32_t* nt_idx, const int32_t* gptr, const float* gpar, const float* x,
                                                 const float* lat_x, const float* lat_y, int nlat, int max_lds_bytes, int max_tris,
                                                 int reduction, float* rhs, float* coeffs, float* work, int tri_slab, float* sol, float* loss,
                                                 float* g_sol, void* stream) {
    return modular_forward(Band::window, "gadapt_fem_modular_forward_window", FEM_BATCH(nullptr, max_tris), {rhs, coeffs, work}, reduction, tri_slab, sol,
                           loss, g_sol, (hipStream_t)stream);
}

extern "C" int gadapt_fem_backward(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                   const int32_t* tri_mesh, const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                                   const int32_t* nt_idx, const int32_t* gptr, const float* gpar, const float* x, const float* lat_x,
                                   const float* lat_y, int nlat, int max_lds_bytes, const float* coeffs, const float* lfac,
                                   const float* g_coeffs, const float* g_sol, float* gc, float* mu, float* tgrad, float* gx, void* stream) {
    return backward(Band::lds, "gadapt_fem_backward", FEM_BATCH(tri_mesh, 0), {nullptr, const_cast<float*>(coeffs), const_cast<float*>(lfac)}, g_coeffs,
                    g_sol, {gc, mu, tgrad, gx}, (hipStream_t)stream);
}

extern "C" int gadapt_fem_backward_window(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                          const int32_t* tri_mesh, const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                                          const int32_t* nt_idx, const int32_t* gptr, const float* gpar, const float* x, const float* lat_x,
                                          const float* lat_y, int nlat, int max_lds_bytes, const float* coeffs, float* work,
                                          const float* g_coeffs, const float* g_sol, float* gc, float* mu, float* tgrad, float* gx,
                                          void* stream) {
    return backward(Band::window, "gadapt_fem_backward_window", FEM_BATCH(tri_mesh, 0), {nullptr, const_cast<float*>(coeffs), work}, g_coeffs, g_sol,
                    {gc, mu, tgrad, gx}, (hipStream_t)stream);
}

extern "C" int gadapt_fem_backward_wave(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                        const int32_t* tri_mesh, const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                                        const int32_t* nt_idx, const int32_t* gptr, const float* gpar, const float* x, const float* lat_x,
                                        const float* lat_y, int nlat, int max_lds_bytes, const float* coeffs, const float* lfac,
                                        const float* g_coeffs, const float* g_sol, float* gc, float* mu, float* tgrad, float* gx,
                                        void* stream) {
    return backward(Band::lds, "gadapt_fem_backward_wave", FEM_BATCH(tri_mesh, 0), {nullptr, const_cast<float*>(coeffs), const_cast<float*>(lfac)},
                    g_coeffs, g_sol, {gc, mu, tgrad, gx}, (hipStream_t)stream, true);
}

extern "C" int gadapt_fem_backward_window_wave(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                               const int32_t* tri_mesh, const int32_t* int_idx, const int32_t* int_node,
                                               const int32_t* nt_ptr, const int32_t* nt_idx, const int32_t* gptr, const float* gpar,
                                               const float* x, const float* lat_x, const float* lat_y, int nlat, int max_lds_bytes,
                                               const float* coeffs, float* work, const float* g_coeffs, const float* g_sol, float* gc,
                                               float* mu, float* tgrad, float* gx, void* stream) {
    return backward(Band::window, "gadapt_fem_backward_window_wave", FEM_BATCH(tri_mesh, 0), {nullptr, const_cast<float*>(coeffs), work}, g_coeffs,
                    g_sol, {gc, mu, tgrad, gx}, (hipStream_t)stream, true);
}

extern "C" int gadapt_fem_forward_wave(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                       const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr, const int32_t* nt_idx,
                                       const int32_t* gptr, const float* gpar, const float* x, const float* lat_x, const float* lat_y,
                                       int nlat, int max_lds_bytes, int max_tris, float* rhs, float* coeffs, float* lfac, float* sol,
                                       void* stream) {
    return forward(Band::lds, "gadapt_fem_forward_wave", FEM_BATCH(nullptr, max_tris), {rhs, coeffs, lfac}, 0, sol, (hipStream_t)stream, true);
}

extern "C" int gadapt_fem_modular_forward_wave(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                               const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr, const int32_t* nt_idx,
                                               const int32_t* gptr, const float* gpar, const float* x, const float* lat_x,
                                               const float* lat_y, int nlat, int max_lds_bytes, int max_tris, int reduction, float* rhs,
                                               float* coeffs, float* lfac, float* sol, float* loss, float* g_sol, void* stream) {
    return modular_forward(Band::lds, "gadapt_fem_modular_forward_wave", FEM_BATCH(nullptr, max_tris), {rhs, coeffs, lfac}, reduction, 0, sol, loss,
                           g_sol, (hipStream_t)stream, true);
}

extern "C" int gadapt_fem_eval_errors_wave(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                           const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr, const int32_t* nt_idx,
                                           const int32_t* gptr, const float* gpar, const float* x, const float* lat_x, const float* lat_y,
                                           int nlat, int max_lds_bytes, int max_tris, float* rhs, float* coeffs, float* lfac, float* sol_work,
                                           float* partials, float* err, void* stream) {
    return eval_errors(Band::lds, "gadapt_fem_eval_errors_wave", FEM_BATCH(nullptr, max_tris), {rhs, coeffs, lfac}, 0, partials, err,
                       (hipStream_t)stream, true, sol_work);
}
