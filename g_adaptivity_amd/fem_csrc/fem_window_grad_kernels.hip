// fem_window_grad_kernels.hip - the differentiable tail of the windowed FEM route (band='window': gadapt_fem_forward_window,
// gadapt_fem_modular_forward_window, gadapt_fem_backward_window in include/gadapt_fem.h) for meshes whose band does not stay
// resident in LDS.
//
// This file is compiled inside fem_kernels.hip's translation unit, after fem_window_kernels.hip: it calls that file's
// win_eval_point_add, win_prefetch and win_back_substitute.  The entry points and the launch sequences, which run these
// kernels between the load vector, solve, loss, chain-rule and gather kernels both routes share, are at the end of
// fem_kernels.hip.
//
// Forward.  The solve leaves the fp64 factor L (n rows of w + 1, entry d of row k = L[k][k-d]) and y in the workspace;
// fem_eval_slab_kernel is fem_eval_err_slab_kernel's slab walk with each lattice point's sum stored to sol: one chain of
// fp32 additions over the triangles in increasing id per point, so sol does not depend on tri_slab, bit for bit.
//
// Backward.  fem_window_adjoint_kernel solves P_II mu = gc_I on the kept factor, one 256-lane workgroup per mesh with the
// solve's ring layout (WinLayout): L z = gc_I forward, L^T mu = z backward (win_back_substitute), both in fp64, mu stored
// in fp32, mu = 0 on boundary nodes.  The forward substitution is column-oriented like the one that rides along the
// factorisation: rows of L enter a ring of R = max(w + S, 2 S) rows in increasing k, S rows per group after the first
// window of w + S rows; the next group's rows (and right-hand side entries) are loaded into registers before the current
// group's columns run and are placed into the ring slots of the rows that group finished.
// Order of a row's sum: entry r starts as (double) gc[int_node[io + r]]; column k = r - w, ..., r - 1 (those >= 0), in
// increasing k, subtracts L[r][k] * z_k, one lane per (column, row) pair and a barrier between columns; then z_r is the
// quotient by L[r][r].  That order is fixed by k and w alone: S, the launch's LDS and the rest of the batch only decide
// when a row enters the ring.  z overwrites the mesh's y slot in the workspace (the forward is done with it) and is
// rewritten from gc on every call; L is only read: a second backward on one forward gives the same bits.
//
// Every loop bound that encloses a __syncthreads() (n, w, S, R, the slab count) comes from the mesh's meta row and the
// launch arguments: uniform over the workgroup.  No hand-over between workgroups, no float atomics, no spin waits.

// ---------------------------------------------------------------------------------------------------- slabbed evaluation
// LDS as fem_eval_err_slab_kernel: acc [ceil(Q / chunks)] | mask [FEM_NB^2][tri_slab / 32]
__global__ void __launch_bounds__(FEM_EVAL_THREADS) fem_eval_slab_kernel(const int32_t* __restrict__ meta, const int32_t* __restrict__ cells,
                                                                         const int32_t* __restrict__ nt_ptr,
                                                                         const int32_t* __restrict__ nt_idx, const float* __restrict__ x,
                                                                         const float* __restrict__ coeffs, const float* __restrict__ lat_x,
                                                                         const float* __restrict__ lat_y, int nlat, int tri_slab,
                                                                         float* __restrict__ sol) {
    extern __shared__ float lds_eval[];
    const int b = blockIdx.x;
    const int32_t* mt = meta + b * GADAPT_FEM_META;
    const int t0 = mt[GADAPT_FEM_M_TRI_OFF], nt = mt[GADAPT_FEM_M_N_TRIS];
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
    for (int q = q0 + threadIdx.x; q < q1; q += FEM_EVAL_THREADS) sol[(int64_t)b * Q + q] = acc[q - q0];
}

// ---------------------------------------------------------------------------------------------------- the adjoint solve
// L z = gc_I on the stored factor, in increasing k: z goes to yg [n].  A [R][ldp] and bv [R] in LDS (the solve's ring).
// yg is written here and read back by win_back_substitute in the same workgroup: no __restrict__ on it or on Lg.
__device__ inline void win_forward_substitute(int n, int w, int io, const WinLayout& L, double* A, double* bv,
                                              const int32_t* __restrict__ int_node, const float* __restrict__ gc, const double* Lg,
                                              double* yg) {
    const int tid = threadIdx.x, ld = L.ld, ldp = L.ldp, R = L.R, S = L.S;
    double pre[FEM_WIN_PRE];
    double gpre = 0.0;
    int hi = min(min(S, n) + w, n);                               // rows [0, hi) have entered the ring; hi <= w + S <= R
    for (int idx = tid; idx < hi * ld; idx += FEM_WIN_THREADS) {
        const int rr = idx / ld, dd = idx - rr * ld;
        A[rr * ldp + dd] = Lg[idx];
    }
    for (int r = tid; r < hi; r += FEM_WIN_THREADS) bv[r] = (double)gc[int_node[io + r]];
    for (int k0 = 0; k0 < n; k0 += S) {
        const int kend = min(k0 + S, n);
        const int nhi = min(min(kend + S, n) + w, n);             // the next group's window: at most S rows more
        if (nhi > hi) {
            win_prefetch(pre, Lg, ld, hi, nhi);
            if (tid < nhi - hi) gpre = (double)gc[int_node[io + hi + tid]];
        }
        __syncthreads();
        int sk = k0 % R;
        for (int k = k0; k < kend; ++k) {
            const double z = bv[sk] / A[sk * ldp];
            const int m = min(w, n - 1 - k);                      // rows k + i < n
            for (int i = 1 + tid; i <= m; i += FEM_WIN_THREADS) {
                int s = sk + i;
                if (s >= R) s -= R;
                bv[s] -= A[s * ldp + i] * z;
            }
            __syncthreads();                                      // every lane has read bv[sk]
            if (tid == 0) bv[sk] = z;
            if (++sk == R) sk = 0;
        }
        __syncthreads();
        for (int k = k0 + tid; k < kend; k += FEM_WIN_THREADS) yg[k] = bv[k % R];
        __syncthreads();                                          // rows k0 .. kend-1 are done: the next rows take their slots
        const int cnt = (nhi - hi) * ld;                          // (row r's slot held row r - R < kend)
#pragma unroll
        for (int i = 0; i < FEM_WIN_PRE; ++i) {
            const int idx = tid + i * FEM_WIN_THREADS;
            if (idx < cnt) {
                const int rr = idx / ld, dd = idx - rr * ld;
                A[((hi + rr) % R) * ldp + dd] = pre[i];
            }
        }
        if (tid < nhi - hi) bv[(hi + tid) % R] = gpre;
        if (nhi > hi) hi = nhi;
    }
    __syncthreads();                                              // yg is complete and the ring is free
}

// adjoint: P_II mu = gc_I on the kept workspace (lambda_I = -mu); mu = 0 on the boundary
__global__ void __launch_bounds__(FEM_WIN_THREADS) fem_window_adjoint_kernel(const int32_t* __restrict__ meta, const int32_t* __restrict__ int_idx,
                                                                             const int32_t* __restrict__ int_node,
                                                                             const float* __restrict__ gc, float* __restrict__ mu,
                                                                             double* work, int lds_bytes) {
    extern __shared__ double lds_win[];
    const int32_t* mt = meta + blockIdx.x * GADAPT_FEM_META;
    const int n = mt[GADAPT_FEM_M_N_INT], w = mt[GADAPT_FEM_M_BAND], io = mt[GADAPT_FEM_M_INT_OFF];
    const int v0 = mt[GADAPT_FEM_M_NODE_OFF], v1 = v0 + mt[GADAPT_FEM_M_N_NODES];
    const WinLayout L = win_layout(w, lds_bytes);
    if (L.R == 0) {                                               // the host checks this before it launches: never write past the ring
        for (int v = v0 + threadIdx.x; v < v1; v += FEM_WIN_THREADS) mu[v] = NAN;
        return;
    }
    double* A = lds_win;
    double* bv = A + L.R * L.ldp;
    for (int v = v0 + threadIdx.x; v < v1; v += FEM_WIN_THREADS)
        if (int_idx[v] < 0) mu[v] = 0.0f;
    const double* Lg = work + ((int64_t)mt[GADAPT_FEM_M_BAND_OFF] + io);   // this mesh's part: n rows of w + 1, then y [n]
    double* yg = work + ((int64_t)mt[GADAPT_FEM_M_BAND_OFF] + io) + (int64_t)n * L.ld;
    win_forward_substitute(n, w, io, L, A, bv, int_node, gc, Lg, yg);
    win_back_substitute(n, w, io, L, A, bv, int_node, Lg, yg, mu);
}
