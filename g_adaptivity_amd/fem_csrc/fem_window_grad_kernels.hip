// fem_window_grad_kernels.hip - the differentiable tail of the windowed FEM route (band='window': gadapt_fem_forward_window,
// gadapt_fem_modular_forward_window, gadapt_fem_backward_window in include/gadapt_fem.h) for meshes whose band does not stay
// resident in LDS.
//
// This file is compiled as the tail of fem_kernels.hip's translation unit, after fem_window_kernels.hip: it launches that
// file's fem_window_rhs_kernel and fem_window_solve_kernel as they are, calls its win_eval_point_add, win_prefetch and
// win_back_substitute, shares its launch plan (win_plan, win_ring_plan), and launches fem_loss_kernel, fem_gc_kernel,
// fem_tri_bwd_kernel and fem_gather_kernel of fem_kernels.hip unchanged.
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

// ---------------------------------------------------------------------------------------------------- C-ABI
static int check_window_forward(const char* who, int B, int N, int T, const void* meta, const void* cells, const void* node_mesh,
                                const void* int_idx, const void* int_node, const void* nt_ptr, const void* nt_idx, const void* gptr,
                                const void* gpar, const void* x, const float* lat_x, const float* lat_y, int nlat, int max_lds_bytes,
                                int max_tris, const void* rhs, const void* coeffs, const void* work, int tri_slab, const void* sol, WinPlan* P) {
    char msg[96];
    if (B <= 0 || N <= 0 || T <= 0 || !meta || !cells || !node_mesh || !int_idx || !int_node || !nt_ptr || !nt_idx || !gptr || !gpar || !x ||
        !rhs || !coeffs || !work || ((uintptr_t)work & 7) || !sol || max_tris <= 0) {
        snprintf(msg, sizeof msg, "%s: null pointer or bad size", who);
        return fail(GADAPT_FEM_E_BADARG, msg);
    }
    int rc = check_lat(lat_x, lat_y, nlat);
    if (rc) return rc;
    if (nlat > 46340) {
        snprintf(msg, sizeof msg, "%s: nlat * nlat exceeds the int range", who);
        return fail(GADAPT_FEM_E_BADARG, msg);
    }
    return win_plan(who, nlat, max_lds_bytes, max_tris, tri_slab, P);
}

static int launch_window_forward(int B, int N, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh, const int32_t* int_idx,
                                 const int32_t* int_node, const int32_t* nt_ptr, const int32_t* nt_idx, const int32_t* gptr,
                                 const float* gpar, const float* x, const float* lat_x, const float* lat_y, int nlat, const WinPlan& P,
                                 float* rhs, float* coeffs, float* work, float* sol, hipStream_t s) {
    fem_window_rhs_kernel<<<(N + 255) / 256, 256, 0, s>>>(N, cells, node_mesh, int_idx, nt_ptr, nt_idx, gptr, gpar, x, rhs);
    int rc = launched("fem_window_rhs_kernel");
    if (rc) return rc;
    fem_window_solve_kernel<<<B, FEM_WIN_THREADS, (size_t)P.solve_lds, s>>>(meta, cells, int_idx, int_node, nt_ptr, nt_idx, x, rhs, coeffs,
                                                                            reinterpret_cast<double*>(work), (int)P.solve_lds);
    if ((rc = launched("fem_window_solve_kernel"))) return rc;
    fem_eval_slab_kernel<<<dim3(B, FEM_EVAL_CHUNKS), FEM_EVAL_THREADS, (size_t)P.eval_lds, s>>>(meta, cells, nt_ptr, nt_idx, x, coeffs, lat_x,
                                                                                                lat_y, nlat, P.slab, sol);
    return launched("fem_eval_slab_kernel");
}

extern "C" int gadapt_fem_forward_window(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                         const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr, const int32_t* nt_idx,
                                         const int32_t* gptr, const float* gpar, const float* x, const float* lat_x, const float* lat_y,
                                         int nlat, int max_lds_bytes, int max_tris, float* rhs, float* coeffs, float* work, int tri_slab,
                                         float* sol, void* stream) {
    WinPlan P;
    int rc = check_window_forward("gadapt_fem_forward_window", B, N, T, meta, cells, node_mesh, int_idx, int_node, nt_ptr, nt_idx, gptr, gpar,
                                  x, lat_x, lat_y, nlat, max_lds_bytes, max_tris, rhs, coeffs, work, tri_slab, sol, &P);
    if (rc) return rc;
    return launch_window_forward(B, N, meta, cells, node_mesh, int_idx, int_node, nt_ptr, nt_idx, gptr, gpar, x, lat_x, lat_y, nlat, P, rhs,
                                 coeffs, work, sol, (hipStream_t)stream);
}

extern "C" int gadapt_fem_modular_forward_window(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                                 const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                                                 const int32_t* nt_idx, const int32_t* gptr, const float* gpar, const float* x,
                                                 const float* lat_x, const float* lat_y, int nlat, int max_lds_bytes, int max_tris,
                                                 int reduction, float* rhs, float* coeffs, float* work, int tri_slab, float* sol, float* loss,
                                                 float* g_sol, void* stream) {
    if (B <= 0 || !loss || !g_sol || (reduction != GADAPT_FEM_LOSS_MSE && reduction != GADAPT_FEM_LOSS_SIMPSON))
        return fail(GADAPT_FEM_E_BADARG, "gadapt_fem_modular_forward_window: null output or unknown reduction");
    if (reduction == GADAPT_FEM_LOSS_SIMPSON && (nlat < 3 || !(nlat & 1)))
        return fail(GADAPT_FEM_E_BADARG, "gadapt_fem_modular_forward_window: the Simpson rule needs an odd nlat >= 3");
    if (nlat > 0 && (int64_t)nlat * 4 > GADAPT_FEM_LDS_BUDGET)
        return fail(GADAPT_FEM_E_LDS, "gadapt_fem_modular_forward_window: the lattice's row sums exceed the LDS budget");
    WinPlan P;
    int rc = check_window_forward("gadapt_fem_modular_forward_window", B, N, T, meta, cells, node_mesh, int_idx, int_node, nt_ptr, nt_idx,
                                  gptr, gpar, x, lat_x, lat_y, nlat, max_lds_bytes, max_tris, rhs, coeffs, work, tri_slab, sol, &P);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = launch_window_forward(B, N, meta, cells, node_mesh, int_idx, int_node, nt_ptr, nt_idx, gptr, gpar, x, lat_x, lat_y, nlat, P, rhs,
                                    coeffs, work, sol, s)))
        return rc;
    fem_loss_kernel<<<B, FEM_LOSS_THREADS, (size_t)nlat * 4, s>>>(gptr, gpar, lat_x, lat_y, nlat, reduction, sol, loss, g_sol);
    return launched("fem_loss_kernel");
}

extern "C" int gadapt_fem_backward_window(int B, int N, int T, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                          const int32_t* tri_mesh, const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                                          const int32_t* nt_idx, const int32_t* gptr, const float* gpar, const float* x, const float* lat_x,
                                          const float* lat_y, int nlat, int max_lds_bytes, const float* coeffs, float* work,
                                          const float* g_coeffs, const float* g_sol, float* gc, float* mu, float* tgrad, float* gx,
                                          void* stream) {
    if (B <= 0 || N <= 0 || T <= 0 || !meta || !cells || !node_mesh || !tri_mesh || !int_idx || !int_node || !nt_ptr || !nt_idx || !gptr ||
        !gpar || !x || !coeffs || !work || ((uintptr_t)work & 7) || !gc || !mu || !tgrad || !gx)
        return fail(GADAPT_FEM_E_BADARG, "gadapt_fem_backward_window: null pointer or bad size");
    int rc = check_lat(lat_x, lat_y, nlat);
    if (rc) return rc;
    int64_t solve_lds = 0;
    if ((rc = win_ring_plan(max_lds_bytes, &solve_lds))) return rc;
    hipStream_t s = (hipStream_t)stream;
    fem_gc_kernel<<<(N + 255) / 256, 256, 0, s>>>(N, cells, node_mesh, nt_ptr, nt_idx, x, lat_x, lat_y, nlat, g_coeffs, g_sol, gc);
    if ((rc = launched("fem_gc_kernel"))) return rc;
    fem_window_adjoint_kernel<<<B, FEM_WIN_THREADS, (size_t)solve_lds, s>>>(meta, int_idx, int_node, gc, mu, reinterpret_cast<double*>(work),
                                                                            (int)solve_lds);
    if ((rc = launched("fem_window_adjoint_kernel"))) return rc;
    fem_tri_bwd_kernel<<<(T + 255) / 256, 256, 0, s>>>(T, cells, tri_mesh, int_idx, nt_ptr, nt_idx, gptr, gpar, x, lat_x, lat_y, nlat, coeffs,
                                                       mu, g_sol, tgrad);
    if ((rc = launched("fem_tri_bwd_kernel"))) return rc;
    fem_gather_kernel<<<(N + 255) / 256, 256, 0, s>>>(N, nt_ptr, nt_idx, tgrad, gx);
    return launched("fem_gather_kernel");
}
