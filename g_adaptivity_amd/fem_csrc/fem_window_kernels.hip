// fem_window_kernels.hip - the FEM route for meshes beyond the resident-band limit (band='window'): here its evaluation
// (gadapt_fem_eval_errors_window in include/gadapt_fem.h; the differentiable tail on the same solve is fem_window_grad_kernels.hip): a banded Cholesky that keeps a ring of band rows in LDS and
// streams the finished factor through a global workspace, and a lattice evaluation that takes the triangles slab by slab.
//
// This file is compiled inside fem_kernels.hip's translation unit (it is #included there, after the last kernel): it calls
// that file's device helpers (tri_geometry, fill_pairs, build_bin_mask, the bin-mask walk's helpers, wave_sum, simpson_box).
// The entry points, their checks and the launch sequences of both routes are at the end of fem_kernels.hip.
//
// Arithmetic.  The order of fem_factor_kernel / band_factor / band_solve: row-wise assembly in increasing incidence,
// column-oriented updates in increasing k, forward substitution in increasing k, back substitution in decreasing k, no FMA
// contraction.  Each band entry is updated by exactly one lane per column, so how the lanes share a column does not show.
// The element terms are those kernels' fp32 expressions; the ring they are summed into, the stored factor and both
// substitutions are fp64.  With everything in fp32 the route was bit-identical to the LDS route where both fit, and 2.6e-4
// from the fp64 yardstick in L1 at 27 x 27 (the evaluation's rule allows 2e-4): the conditioning grows with the mesh.  The
// lattice sum of a point runs over the triangles in increasing id, slab after slab, into one running fp32 accumulator:
// the same chain of additions as eval_point, whatever the slab.
//
// Workgroup: 256 lanes (four waves) per mesh, not one wave.  At w = 62 (64 x 64) a column's rank-1 update has 1953 pairs:
// 8 pair steps per lane instead of 31, and the ring (64 KB with its slack rows at 64 x 64) lets only two workgroups share
// a CU, which one wave each would leave at 2 waves.  The price is a real s_barrier twice per column where a one-wave
// workgroup pays almost nothing; with 3844 columns the column loop is barrier- and LDS-latency-bound either way, and four
// waves cut the LDS work between the barriers by four.  LDS rows are padded to an even length: the pair walk reads
// A[k+j][j] for consecutive j, a stride of (row + 1) doubles, odd, so the 32 lanes of a ds_read_b64 group fall on 32
// different bank pairs; the A[k+i][i] operand is the same address for the lanes of one i (a broadcast) and the written
// A[k+i][i-j] are consecutive.  The pair table itself is read at consecutive words.
//
// Ring.  R = max(w + S, 2 S) rows of the band, S >= 1 "slack" rows (as many as the launch's LDS leaves, at most 64): the
// sweep goes S columns at a time; before a group the rows that enter the window are assembled, one row per lane, after it
// the S finished rows of L go to the workspace in one coalesced pass.  S = 1 is the plain ring of w + 1 rows, assembled by
// one lane per column; gadapt_fem_window_lds_bytes is that minimum.  The back substitution reads the factor back S rows at
// a time through registers into two LDS stages: the loads of the next group are issued before the current group's columns.
//
// Every loop bound that encloses a __syncthreads() (n, w, S, R, the slab count) comes from the mesh's meta row and the
// launch arguments: uniform over the workgroup.  No hand-over between workgroups, no float atomics, no spin waits.

#define FEM_WIN_THREADS 256
#define FEM_WIN_MAX_S 64
#define FEM_WIN_PRE 16                                            // registers per lane of the back substitution's prefetch

struct WinLayout {
    int ld, ldp, np, S, R;                                        // R == 0: the ring does not fit
};

__host__ __device__ inline int win_min_rows(int w) { return w + 1 > 2 ? w + 1 : 2; }

// LDS of one mesh: A [R][ldp] and b [R] in fp64 | pairs [np] int32
__host__ __device__ inline int64_t win_bytes(int w, int rows) {
    const int64_t ld = w + 1, ldp = (ld + 1) & ~(int64_t)1, np = (int64_t)w * (w + 1) / 2;
    return 4 * np + 8 * (int64_t)rows * (ldp + 1);
}

__host__ __device__ inline WinLayout win_layout(int w, int64_t lds_bytes) {
    WinLayout L;
    L.ld = w + 1;
    L.ldp = (L.ld + 1) & ~1;
    L.np = w * (w + 1) / 2;
    const int64_t rows = (lds_bytes - 4 * (int64_t)L.np) / (8 * (int64_t)(L.ldp + 1));
    if (rows < win_min_rows(w)) {
        L.S = L.R = 0;
        return L;
    }
    int64_t S = rows - w < rows / 2 ? rows - w : rows / 2;        // w + S <= rows and 2 S <= rows
    if (S > FEM_WIN_MAX_S) S = FEM_WIN_MAX_S;
    if (S * L.ld > FEM_WIN_PRE * FEM_WIN_THREADS) S = FEM_WIN_PRE * FEM_WIN_THREADS / L.ld;
    if (S < 1) S = 1;
    L.S = (int)S;
    L.R = w + L.S > 2 * L.S ? w + L.S : 2 * L.S;
    return L;
}

extern "C" int64_t gadapt_fem_window_lds_bytes(int n_int, int band) {
    if (n_int <= 0 || band < 0) return 0;
    return win_bytes(band, win_min_rows(band));
}

extern "C" int64_t gadapt_fem_window_workspace_floats(int n_meshes, const int32_t* meta) {
    if (n_meshes <= 0 || !meta) return fem_fail(GADAPT_FEM_E_BADARG, "gadapt_fem_window_workspace_floats: null pointer or bad size");
    int64_t tot = 0;
    for (int b = 0; b < n_meshes; ++b) {
        const int32_t* mt = meta + b * GADAPT_FEM_META;
        tot += (int64_t)mt[GADAPT_FEM_M_N_INT] * (mt[GADAPT_FEM_M_BAND] + 2);   // n_int rows of band + 1 and y, in fp64
    }
    return 2 * tot;
}

// ---------------------------------------------------------------------------------------------------- load vector
// fem_rhs_kernel with the forcing and the two Simpson sums in fp64; the Simpson points, the hat function (its inclusive
// edge tests classify a point as fem_rhs_kernel does) and the boundary values stay its fp32 expressions, and the result is
// stored in fp32.  In fp32 the forcing's polynomial cancels (terms of size s^6 against a sum of size s^4 d^2) and costs 1e-3
// of the 64 x 64 error norm, beyond the evaluation's rule; with this load vector the same solve is within 1e-4.
__device__ inline double win_forcing(double x0, double x1, const float* __restrict__ gpar, int g0, int g1) {
    double sol = 0.0;
    for (int g = g0; g < g1; ++g) {
        const double c0 = gpar[4 * g], c1 = gpar[4 * g + 1], s0 = gpar[4 * g + 2], s1 = gpar[4 * g + 3];
        const double s02 = s0 * s0, s12 = s1 * s1, s04 = s02 * s02, s14 = s12 * s12;
        const double d0 = c0 - x0, d1 = c1 - x1;
        const double e = exp(-(d0 * d0 / s02) - d1 * d1 / s12);
        const double poly = 4.0 * (c1 * c1) * s04 - 2.0 * s02 * s14 + 4.0 * s14 * (d0 * d0) - 8.0 * c1 * s04 * x1
                            - 2.0 * s04 * (s12 - 2.0 * (x1 * x1));
        sol += (1.0 / (s04 * s14)) * e * poly;
    }
    return sol;
}

__global__ void __launch_bounds__(256) fem_window_rhs_kernel(int n_nodes, const int32_t* __restrict__ cells, const int32_t* __restrict__ node_mesh,
                                                             const int32_t* __restrict__ int_idx, const int32_t* __restrict__ nt_ptr,
                                                             const int32_t* __restrict__ nt_idx, const int32_t* __restrict__ gptr,
                                                             const float* __restrict__ gpar, const float* __restrict__ x,
                                                             float* __restrict__ rhs) {
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
    const double hx3 = ((double)bx1 - (double)bx0) / (double)(n - 1) / 3.0, hy3 = ((double)by1 - (double)by0) / (double)(n - 1) / 3.0;
    double row[n];
    for (int i = 0; i < n; ++i) {
        const float px = fem::linspace_at(bx0, bx1, n, i);
        double f[n];
        for (int j = 0; j < n; ++j) {
            const float py = fem::linspace_at(by0, by1, n, j);
            float out;
            const float div = fem::phim_parts(px, py, m, nt_ptr, nt_idx, cells, x, &out);
            f[j] = (double)(out / div) * win_forcing(px, py, gpar, g0, g1);
        }
        double s = 0.0;
        for (int k = 0; k + 2 < n; k += 2) s = s + hy3 * (f[k] + 4.0 * f[k + 1] + f[k + 2]);
        row[i] = s;
    }
    double s = 0.0;
    for (int k = 0; k + 2 < n; k += 2) s = s + hx3 * (row[k] + 4.0 * row[k + 1] + row[k + 2]);
    rhs[m] = (float)s;
}

// ---------------------------------------------------------------------------------------------------- the windowed solve
// row r of P_II and of the right-hand side, as fem_factor_kernel assembles them (one lane owns the whole row)
__device__ inline void win_assemble_row(int r, int g, int ld, double* __restrict__ Arow, double* __restrict__ bslot,
                                        const int32_t* __restrict__ cells, const int32_t* __restrict__ int_idx,
                                        const int32_t* __restrict__ nt_ptr, const int32_t* __restrict__ nt_idx,
                                        const float* __restrict__ x, const float* __restrict__ rhs) {
    for (int d = 0; d < ld; ++d) Arow[d] = 0.0;
    double b = -(double)rhs[g];
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
            if (ih < 0) b -= (double)p * (double)rhs[h];
            else if (ih <= r) Arow[r - ih] += (double)p;
        }
    }
    *bslot = b;
}

// Factor P_II = L L^T through the ring and solve L y = b along the same sweep.  Row k of L goes to Lg[k * ld ..] (ld = w + 1,
// entry d = L[k][k-d]) and y_k to yg[k] as soon as column k is eliminated.  A [R][ldp], bv [R], pairs [np] in LDS.
// Lg and yg are written here and read back by win_back_substitute in the same workgroup: no __restrict__ on them.
__device__ inline void win_factor_forward(int n, int w, int io, const WinLayout& L, double* A, double* bv, const int32_t* pairs,
                                          const int32_t* __restrict__ cells, const int32_t* __restrict__ int_idx,
                                          const int32_t* __restrict__ int_node, const int32_t* __restrict__ nt_ptr,
                                          const int32_t* __restrict__ nt_idx, const float* __restrict__ x,
                                          const float* __restrict__ rhs, double* Lg, double* yg) {
    const int tid = threadIdx.x, ld = L.ld, ldp = L.ldp, R = L.R, S = L.S;
    int hi = 0;                                                   // rows [0, hi) have entered the window
    for (int k0 = 0; k0 < n; k0 += S) {
        const int kend = min(k0 + S, n), need = min(kend + w, n);
        for (int r = hi + tid; r < need; r += FEM_WIN_THREADS) {  // their slots held rows < k0, flushed below
            const int s = r % R;
            win_assemble_row(r, int_node[io + r], ld, A + s * ldp, bv + s, cells, int_idx, nt_ptr, nt_idx, x, rhs);
        }
        hi = need;
        __syncthreads();
        int sk = k0 % R;
        for (int k = k0; k < kend; ++k) {
            double* rowk = A + sk * ldp;
            const double d = sqrt(rowk[0]);
            const double y = bv[sk] / d;
            const int m = min(w, n - 1 - k);                      // rows k + i < n
            for (int i = 1 + tid; i <= m; i += FEM_WIN_THREADS) {
                int s = sk + i;
                if (s >= R) s -= R;
                A[s * ldp + i] = A[s * ldp + i] / d;
            }
            __syncthreads();
            if (tid == 0) {
                rowk[0] = d;
                bv[sk] = y;
            }
            const int npk = m * (m + 1) / 2;                      // the table lists the pairs by increasing i
            for (int p = tid; p < npk; p += FEM_WIN_THREADS) {
                const int i = pairs[p] >> 16, j = pairs[p] & 0xffff;
                int si = sk + i, sj = sk + j;
                if (si >= R) si -= R;
                if (sj >= R) sj -= R;
                A[si * ldp + (i - j)] -= A[si * ldp + i] * A[sj * ldp + j];
            }
            for (int i = 1 + tid; i <= m; i += FEM_WIN_THREADS) {
                int s = sk + i;
                if (s >= R) s -= R;
                bv[s] -= A[s * ldp + i] * y;
            }
            __syncthreads();
            if (++sk == R) sk = 0;
        }
        const int cnt = (kend - k0) * ld;                         // rows k0 .. kend-1 are final: one coalesced pass
        for (int idx = tid; idx < cnt; idx += FEM_WIN_THREADS) {
            const int rr = idx / ld, dd = idx - rr * ld;
            Lg[(int64_t)k0 * ld + idx] = A[((k0 + rr) % R) * ldp + dd];
        }
        for (int k = k0 + tid; k < kend; k += FEM_WIN_THREADS) yg[k] = bv[k % R];
        __syncthreads();
    }
}

__device__ inline void win_prefetch(double (&pre)[FEM_WIN_PRE], const double* Lg, int ld, int k0, int k1) {
    const int cnt = (k1 - k0) * ld;
#pragma unroll
    for (int i = 0; i < FEM_WIN_PRE; ++i) {
        const int idx = threadIdx.x + i * FEM_WIN_THREADS;
        pre[i] = idx < cnt ? Lg[(int64_t)k0 * ld + idx] : 0.0;
    }
}

// L^T c = y on the stored factor, in reverse: y is read from yg [n], c goes to coeffs[int_node[io + k]] rounded to fp32.
// The rows of a group of S columns come through registers into one of two LDS stages (st [2][S][ldp], the ring's space);
// the next group's loads are in flight while the current group's columns run.  A later adjoint kernel can call this on a
// kept workspace.
__device__ inline void win_back_substitute(int n, int w, int io, const WinLayout& L, double* st, double* bv,
                                           const int32_t* __restrict__ int_node, const double* Lg, const double* yg,
                                           float* __restrict__ coeffs) {
    const int tid = threadIdx.x, ld = L.ld, ldp = L.ldp, R = L.R, S = L.S;
    double pre[FEM_WIN_PRE];
    int k1 = n, k0 = max(0, n - S), lo = n, cur = 0;              // entries [lo, k1) of y are in the ring
    win_prefetch(pre, Lg, ld, k0, k1);
    while (k1 > 0) {
        double* stage = st + cur * S * ldp;
        const int cnt = (k1 - k0) * ld;
#pragma unroll
        for (int i = 0; i < FEM_WIN_PRE; ++i) {
            const int idx = tid + i * FEM_WIN_THREADS;
            if (idx < cnt) {
                const int rr = idx / ld, dd = idx - rr * ld;
                stage[rr * ldp + dd] = pre[i];
            }
        }
        const int nlo = max(0, k0 - w);
        for (int m = nlo + tid; m < lo; m += FEM_WIN_THREADS) bv[m % R] = yg[m];
        lo = nlo;
        const int nk1 = k0, nk0 = max(0, k0 - S);
        if (nk1 > 0) win_prefetch(pre, Lg, ld, nk0, nk1);
        __syncthreads();
        int sk = (k1 - 1) % R;
        for (int k = k1 - 1; k >= k0; --k) {
            const double* row = stage + (k - k0) * ldp;
            const double y = bv[sk] / row[0];
            const int m = min(w, k);                              // entries k - j >= 0
            for (int j = 1 + tid; j <= m; j += FEM_WIN_THREADS) {
                int s = sk - j;
                if (s < 0) s += R;
                bv[s] -= row[j] * y;
            }
            __syncthreads();                                      // every lane has read bv[sk]
            if (tid == 0) bv[sk] = y;
            if (--sk < 0) sk = R - 1;
        }
        __syncthreads();
        for (int k = k0 + tid; k < k1; k += FEM_WIN_THREADS) coeffs[int_node[io + k]] = (float)bv[k % R];
        __syncthreads();                                          // the next group's entries take these slots
        k1 = nk1;
        k0 = nk0;
        cur ^= 1;
    }
}

__global__ void __launch_bounds__(FEM_WIN_THREADS) fem_window_solve_kernel(const int32_t* __restrict__ meta, const int32_t* __restrict__ cells,
                                                                           const int32_t* __restrict__ int_idx,
                                                                           const int32_t* __restrict__ int_node,
                                                                           const int32_t* __restrict__ nt_ptr,
                                                                           const int32_t* __restrict__ nt_idx, const float* __restrict__ x,
                                                                           const float* __restrict__ rhs, float* __restrict__ coeffs,
                                                                           double* work, int lds_bytes) {
    extern __shared__ double lds_win[];
    const int32_t* mt = meta + blockIdx.x * GADAPT_FEM_META;
    const int n = mt[GADAPT_FEM_M_N_INT], w = mt[GADAPT_FEM_M_BAND], io = mt[GADAPT_FEM_M_INT_OFF];
    const int v0 = mt[GADAPT_FEM_M_NODE_OFF], v1 = v0 + mt[GADAPT_FEM_M_N_NODES];
    const WinLayout L = win_layout(w, lds_bytes);
    if (L.R == 0) {                                               // the host checks this before it launches: never write past the ring
        for (int v = v0 + threadIdx.x; v < v1; v += FEM_WIN_THREADS) coeffs[v] = NAN;
        return;
    }
    double* A = lds_win;
    double* bv = A + L.R * L.ldp;
    int32_t* pairs = (int32_t*)(bv + L.R);
    for (int v = v0 + threadIdx.x; v < v1; v += FEM_WIN_THREADS)
        if (int_idx[v] < 0) coeffs[v] = rhs[v];                    // c_B = RHS_B (the identity rows, difFEM_2d.py:358-359)
    for (int i = 1, p = 0; i <= w; ++i)                            // fill_pairs' table, spread over this workgroup's lanes
        for (int j = 1; j <= i; ++j, ++p)
            if ((p % FEM_WIN_THREADS) == (int)threadIdx.x) pairs[p] = (i << 16) | j;
    double* Lg = work + ((int64_t)mt[GADAPT_FEM_M_BAND_OFF] + io);   // this mesh's part: n rows of w + 1, then y [n]
    double* yg = Lg + (int64_t)n * L.ld;
    win_factor_forward(n, w, io, L, A, bv, pairs, cells, int_idx, int_node, nt_ptr, nt_idx, x, rhs, Lg, yg);
    win_back_substitute(n, w, io, L, A, bv, int_node, Lg, yg, coeffs);
}

// ---------------------------------------------------------------------------------------------------- slabbed evaluation
// LDS: acc [ceil(Q / chunks)] running sums of this chunk's lattice points | mask [FEM_NB^2][tri_slab / 32]
__host__ __device__ inline int64_t win_eval_acc_floats(int nlat) {
    return ((int64_t)nlat * nlat + FEM_EVAL_CHUNKS - 1) / FEM_EVAL_CHUNKS;
}

// eval_point's walk over one slab of triangles (t0 = the slab's first triangle, W its words), continuing the sum `acc`
__device__ inline float win_eval_point_add(float acc, float px, float py, const uint32_t* mask, int W, int t0, const EvalFrame& f,
                                           const int32_t* __restrict__ cells, const int32_t* __restrict__ nt_ptr,
                                           const int32_t* __restrict__ nt_idx, const float* __restrict__ x,
                                           const float* __restrict__ coeffs) {
    const uint32_t* bm = mask + (bin_of(px, f.lox, f.scx) * FEM_NB + bin_of(py, f.loy, f.scy)) * W;
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

__global__ void __launch_bounds__(FEM_EVAL_THREADS) fem_eval_err_slab_kernel(const int32_t* __restrict__ meta, const int32_t* __restrict__ cells,
                                                                             const int32_t* __restrict__ nt_ptr,
                                                                             const int32_t* __restrict__ nt_idx,
                                                                             const int32_t* __restrict__ gptr, const float* __restrict__ gpar,
                                                                             const float* __restrict__ x, const float* __restrict__ coeffs,
                                                                             const float* __restrict__ lat_x, const float* __restrict__ lat_y,
                                                                             int nlat, int tri_slab, float* __restrict__ partials) {
    extern __shared__ float lds_eval[];
    const int b = blockIdx.x;
    const int32_t* mt = meta + b * GADAPT_FEM_META;
    const int t0 = mt[GADAPT_FEM_M_TRI_OFF], nt = mt[GADAPT_FEM_M_N_TRIS];
    const int g0 = gptr[b], g1 = gptr[b + 1];
    const EvalFrame f = eval_frame(lat_x, lat_y, nlat);
    const int Q = nlat * nlat;
    const int q0 = (int)((int64_t)Q * blockIdx.y / gridDim.y), q1 = (int)((int64_t)Q * (blockIdx.y + 1) / gridDim.y);
    float* acc = lds_eval;
    uint32_t* mask = reinterpret_cast<uint32_t*>(lds_eval + win_eval_acc_floats(nlat));
    for (int q = q0 + threadIdx.x; q < q1; q += FEM_EVAL_THREADS) acc[q - q0] = 0.0f;   // each point is its own lane's throughout
    for (int s0 = 0; s0 < nt; s0 += tri_slab) {
        const int ns = min(tri_slab, nt - s0), W = (int)eval_words(ns);
        __syncthreads();                                           // every lane is done with the previous slab's mask
        build_bin_mask(mask, W, t0 + s0, ns, f, cells, x);
        for (int q = q0 + threadIdx.x; q < q1; q += FEM_EVAL_THREADS)
            acc[q - q0] = win_eval_point_add(acc[q - q0], lat_x[q / nlat], lat_y[q % nlat], mask, W, t0 + s0, f, cells, nt_ptr, nt_idx, x,
                                             coeffs);
    }
    float s1 = 0.0f, s2 = 0.0f;
    for (int q = q0 + threadIdx.x; q < q1; q += FEM_EVAL_THREADS) {
        const int i = q / nlat, j = q % nlat;
        const float px = lat_x[i], py = lat_y[j];
        const float e = acc[q - q0] - fem::u_true(px, py, gpar, g0, g1);
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

// ---------------------------------------------------------------------------------------------------- launch plan
// The LDS of a windowed launch (the windowed half of make_plan in fem_kernels.hip), checked before anything is launched and
// shared by every windowed entry point: the ring of the solve (and of the adjoint solve on the kept workspace) with its
// slack rows, and the slab of the evaluation.

static int win_ring_plan(int max_lds_bytes, int64_t* solve_lds) {
    if (max_lds_bytes <= 0 || max_lds_bytes > GADAPT_FEM_LDS_BUDGET)
        return fem_fail(GADAPT_FEM_E_LDS, "windowed band: the ring's LDS bytes are outside (0, GADAPT_FEM_LDS_BUDGET]");
    // the widest band max_lds_bytes stands for, then room for FEM_WIN_MAX_S slack rows on it (what the budget leaves of them)
    int w_max = 0;
    while (gadapt_fem_window_lds_bytes(1, w_max + 1) <= max_lds_bytes) ++w_max;
    int64_t lds = win_bytes(w_max, w_max + FEM_WIN_MAX_S > 2 * FEM_WIN_MAX_S ? w_max + FEM_WIN_MAX_S : 2 * FEM_WIN_MAX_S);
    if (lds > GADAPT_FEM_LDS_BUDGET) lds = GADAPT_FEM_LDS_BUDGET;
    if (lds < max_lds_bytes) lds = max_lds_bytes;
    *solve_lds = lds;
    return GADAPT_FEM_OK;
}

static int win_plan(const char* who, int nlat, int max_lds_bytes, int max_tris, int tri_slab, FemPlan* P) {
    if (tri_slab < 0 || (tri_slab & 31)) return fem_fail_as(GADAPT_FEM_E_BADARG, who, "tri_slab must be 0 or a positive multiple of 32");
    int rc = win_ring_plan(max_lds_bytes, &P->solve_lds);
    if (rc) return rc;
    // the slab: acc and the mask share the budget
    const int64_t acc_bytes = win_eval_acc_floats(nlat) * 4;
    const int64_t per_word = (int64_t)FEM_NB * FEM_NB * 4;                       // mask bytes per 32 triangles
    const int64_t fit_words = (GADAPT_FEM_LDS_BUDGET - acc_bytes) / per_word;
    if (acc_bytes > GADAPT_FEM_LDS_BUDGET || fit_words < 1)
        return fem_fail(GADAPT_FEM_E_LDS, "windowed evaluation: the lattice's running sums leave no room for a triangle slab in the LDS budget");
    int64_t words = tri_slab ? tri_slab / 32 : fit_words;
    if (words > fit_words) return fem_fail(GADAPT_FEM_E_LDS, "windowed evaluation: tri_slab's bin mask exceeds the LDS budget");
    if (words > eval_words(max_tris)) words = eval_words(max_tris);
    P->eval_lds = acc_bytes + words * per_word;
    P->slab = (int)words * 32;
    return GADAPT_FEM_OK;
}
