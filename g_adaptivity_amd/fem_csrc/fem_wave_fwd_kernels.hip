// fem_wave_fwd_kernels.hip - the wave-parallel form of the forward's load vector and lattice evaluation on the resident-band
// route (fem_forward='wave': gadapt_fem_forward_wave, gadapt_fem_modular_forward_wave in include/gadapt_fem.h), and at the
// file's end the error norms of the evaluation on them (gadapt_fem_eval_errors_wave).
//
// This file is compiled inside fem_kernels.hip's translation unit, after fem_wave_grad_kernels.hip: it calls
// fem_kernels.hip's simpson_box, eval_frame, build_bin_mask and bin_of and the fem:: helpers, and takes FEM_WAVE from the
// backward's file.  The entry points are at fem_kernels.hip's end; the factor launch between the two kernels is
// fem_factor_kernel as it is.
//
// fem_rhs_kernel gives a node to a lane, which computes the 81 points of its 9 x 9 Simpson rule one after the other, each a
// phim walk over the node's triangles; fem_eval_kernel gives five lattice points to a lane, and the 64 lanes of a wave meet
// their containing triangles at different turns of the candidate loop, so the wave runs the expensive branch at nearly
// every turn.  A result of either kernel is a chain of fp32 additions in a fixed order on addends that do not depend on
// each other.  Here the addends are computed side by side with the same helpers on the same arguments (no FMA contraction:
// the same bits) and each chain is then added in the lane kernel's order.  The results are the lane kernels', bit for bit.
//
// Load vector.  A node is a wave's: the 81 integrand values go over the lanes in two rounds (64 + 17) into an LDS slab in
// (i, j) order, nine lanes form the nine y-rule sums with fem_rhs_kernel's statement, one lane the x-rule sum.  A workgroup
// is ONE wave; the node's range exit and the boundary exit are taken by the whole workgroup or not at all (every lane reads
// int_idx[m] from the same address), both stand in front of the barriers, and the loop counts are compile-time constants:
// every barrier is reached by every lane.  372 B of static LDS.
//
// Evaluation.  A lane keeps fem_eval_kernel's chain of one lattice point, but walks the bin's candidates in two phases.
// Phase 1 runs fem::inside alone and notes the containing triangles, in increasing id, in FEM_EVALW_CAP registers of the
// lane (named ones, chosen by compares: no array indexed at run time, so no scratch, and no LDS beyond the mask, so the
// route's LDS account and its refusals are fem_eval_kernel's).  Phase 2 runs the three rotations, aux_value and phim_parts
// of the noted triangles in that order and adds coeffs[vc] * (inc / div) to the chain, as eval_point does.  So the lanes of
// a wave run the expensive part together, once or twice per point, not once per candidate.  The note has no silent cap: a
// lane whose registers are full runs phase 2 on them and goes on scanning, which keeps the order; a point in any number of
// overlapping triangles gets eval_point's sum.  A workgroup is one wave and its chunk count is the host's choice: sol[q] does
// not depend on how the lattice is cut, so a batch of one mesh is cut down to one point per lane and spreads over the
// device, at the price of one build_bin_mask per workgroup.  Every lane of the workgroup reaches build_bin_mask's barriers:
// nothing returns before them, and there is none after.  No atomics on floats (the mask's atomicOr is on LDS words).
#define FEM_EVALW_CAP 4

__global__ void __launch_bounds__(FEM_WAVE) fem_rhs_wave_kernel(int n_nodes, const int32_t* __restrict__ cells, const int32_t* __restrict__ node_mesh,
                                                                const int32_t* __restrict__ int_idx, const int32_t* __restrict__ nt_ptr,
                                                                const int32_t* __restrict__ nt_idx, const int32_t* __restrict__ gptr,
                                                                const float* __restrict__ gpar, const float* __restrict__ x, float* __restrict__ rhs) {
    constexpr int n = FEM_SIMPSON_N;
    __shared__ float f[n * n];                                     // the integrand, point (i, j) at i * n + j
    __shared__ float row[n];
    const int m = blockIdx.x, lane = threadIdx.x;
    if (m >= n_nodes) return;                                      // the whole workgroup
    const int b = node_mesh[m];
    const int g0 = gptr[b], g1 = gptr[b + 1];
    if (int_idx[m] < 0) {                                          // the whole workgroup
        const V2 xm = ld2(x, m);
        if (lane == 0) rhs[m] = fem::u_true(xm.x, xm.y, gpar, g0, g1);
        return;
    }
    float bx0, bx1, by0, by1;
    simpson_box(m, nt_ptr, nt_idx, cells, x, bx0, bx1, by0, by1);
    const float hx3 = (bx1 - bx0) / (float)(n - 1) / 3.0f, hy3 = (by1 - by0) / (float)(n - 1) / 3.0f;
    for (int k0 = 0; k0 < n * n; k0 += FEM_WAVE) {
        const int q = k0 + lane;
        if (q < n * n) {
            const float px = fem::linspace_at(bx0, bx1, n, q / n), py = fem::linspace_at(by0, by1, n, q % n);
            float out;
            const float div = fem::phim_parts(px, py, m, nt_ptr, nt_idx, cells, x, &out);
            f[q] = out / div * fem::forcing(px, py, gpar, g0, g1);
        }
    }
    __syncthreads();
    if (lane < n) {
        const float* fi = f + lane * n;
        float s = 0.0f;
        for (int k = 0; k + 2 < n; k += 2) s = s + hy3 * (fi[k] + 4.0f * fi[k + 1] + fi[k + 2]);
        row[lane] = s;
    }
    __syncthreads();
    if (lane == 0) {
        float s = 0.0f;
        for (int k = 0; k + 2 < n; k += 2) s = s + hx3 * (row[k] + 4.0f * row[k + 1] + row[k + 2]);
        rhs[m] = s;
    }
}

// eval_point's terms of the `cnt` noted triangles (4 * id + indicator, the indicator being 1 or 2), added to acc in order
__device__ inline float eval_noted(float acc, int cnt, int c0, int c1, int c2, int c3, float px, float py, const int32_t* __restrict__ cells,
                                   const int32_t* __restrict__ nt_ptr, const int32_t* __restrict__ nt_idx, const float* __restrict__ x,
                                   const float* __restrict__ coeffs) {
    for (int k = 0; k < cnt; ++k) {
        const int code = k == 0 ? c0 : (k == 1 ? c1 : (k == 2 ? c2 : c3));
        const int t = code >> 2;
        const float ind = (float)(code & 3);
        for (int l = 0; l < 3; ++l) {
            int va, vb, vc;
            fem::rotation(cells, t, l, va, vb, vc);
            const float inc = fem::aux_value(px, py, ld2(x, va), ld2(x, vb), ld2(x, vc), ind);
            if (inc == 0.0f) continue;
            const float div = fem::phim_parts(px, py, vc, nt_ptr, nt_idx, cells, x, nullptr);
            acc += coeffs[vc] * (inc / div);
        }
    }
    return acc;
}

// eval_point, the candidates of the bin scanned first and the containing ones evaluated after (the file's head)
__device__ inline float eval_point_wave(float px, float py, const uint32_t* mask, int W, int t0, const EvalFrame& f,
                                        const int32_t* __restrict__ cells, const int32_t* __restrict__ nt_ptr,
                                        const int32_t* __restrict__ nt_idx, const float* __restrict__ x, const float* __restrict__ coeffs) {
    const uint32_t* bm = mask + (bin_of(px, f.lox, f.scx) * FEM_NB + bin_of(py, f.loy, f.scy)) * W;
    float acc = 0.0f;
    int cnt = 0, c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    static_assert(FEM_EVALW_CAP == 4, "c0..c3");
    for (int wd = 0; wd < W; ++wd) {
        uint32_t bits = bm[wd];
        while (bits) {
            const int t = t0 + wd * 32 + __builtin_ctz(bits);
            bits &= bits - 1;
            const float ind = fem::inside(px, py, ld2(x, cells[3 * t + 2]), ld2(x, cells[3 * t + 1]), ld2(x, cells[3 * t]));
            if (ind == 0.0f) continue;
            if (cnt == FEM_EVALW_CAP) {                            // full: evaluate what is noted, in order, and go on
                acc = eval_noted(acc, cnt, c0, c1, c2, c3, px, py, cells, nt_ptr, nt_idx, x, coeffs);
                cnt = 0;
            }
            const int code = 4 * t + (int)ind;                     // ind is 1, or 2 on a degenerate triangle: a sum of two 0/1 products
            if (cnt == 0) c0 = code;
            else if (cnt == 1) c1 = code;
            else if (cnt == 2) c2 = code;
            else c3 = code;
            ++cnt;
        }
    }
    return eval_noted(acc, cnt, c0, c1, c2, c3, px, py, cells, nt_ptr, nt_idx, x, coeffs);
}

// grid (n_meshes, chunks), chunks chosen by eval_wave_chunks
__global__ void __launch_bounds__(FEM_WAVE) fem_eval_wave_kernel(const int32_t* __restrict__ meta, const int32_t* __restrict__ cells,
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
    for (int q = q0 + threadIdx.x; q < q1; q += FEM_WAVE)
        sol[(int64_t)blockIdx.x * Q + q] = eval_point_wave(lat_x[q / nlat], lat_y[q % nlat], mask, W, t0, f, cells, nt_ptr, nt_idx, x, coeffs);
}

// Chunks per mesh of fem_eval_wave_kernel: one point per lane (ceil(Q / 64) workgroups) while the batch leaves the device
// room for that, else as many as keep the launch near FEM_EVALW_GROUPS workgroups, each of which builds its mesh's bin mask.
#define FEM_EVALW_GROUPS 2048

static int eval_wave_chunks(int n_meshes, int nlat) {
    const int64_t per_lane = ((int64_t)nlat * nlat + FEM_WAVE - 1) / FEM_WAVE;
    const int64_t room = FEM_EVALW_GROUPS / n_meshes > 1 ? FEM_EVALW_GROUPS / n_meshes : 1;
    return (int)(per_lane < room ? per_lane : room);
}

// ---------------------------------------------------------------------------------------------------- error norms
// gadapt_fem_eval_errors_wave: the evaluation's norms on the wave-parallel walk.  fem_eval_err_kernel fuses eval_point with the
// sums of the two norms, and the order of those sums is tied to its cut of the lattice (FEM_EVAL_CHUNKS chunks of
// FEM_EVAL_THREADS lanes), which fem_eval_wave_kernel's cut is not.  So the wave route takes two launches: fem_eval_wave_kernel
// writes sol to a workspace (sol_work: 4 * nlat * nlat bytes a mesh, 40 KB at 101 points - on this route sol DOES reach
// memory; the lane route's "sol never written" stays true of the lane route), and the kernel below is fem_eval_err_kernel's
// loop, statement for statement, with eval_point's value read from there.  sol_work carries eval_point's bits, so the
// partials and err are the lane route's, bit for bit, in any batch.  grid (n_meshes, FEM_EVAL_CHUNKS), FEM_EVAL_THREADS
// lanes; 2 * waves floats of static LDS for the wave sums and no dynamic LDS.  Nothing returns before the two barriers:
// every lane reaches both.  No float atomics.
__global__ void __launch_bounds__(FEM_EVAL_THREADS) fem_err_lattice_kernel(const int32_t* __restrict__ gptr, const float* __restrict__ gpar,
                                                                           const float* __restrict__ lat_x, const float* __restrict__ lat_y,
                                                                           int nlat, const float* __restrict__ sol_work,
                                                                           float* __restrict__ partials) {
    constexpr int waves = FEM_EVAL_THREADS / 64;
    __shared__ float red[2 * waves];
    const int b = blockIdx.x;
    const int g0 = gptr[b], g1 = gptr[b + 1];
    const int Q = nlat * nlat;
    const int q0 = (int)((int64_t)Q * blockIdx.y / gridDim.y), q1 = (int)((int64_t)Q * (blockIdx.y + 1) / gridDim.y);
    float s1 = 0.0f, s2 = 0.0f;
    for (int q = q0 + threadIdx.x; q < q1; q += FEM_EVAL_THREADS) {
        const int i = q / nlat, j = q % nlat;
        const float px = lat_x[i], py = lat_y[j];
        const float e = sol_work[(int64_t)b * Q + q] - fem::u_true(px, py, gpar, g0, g1);
        const float w = ((i == 0 || i == nlat - 1) ? 0.5f : 1.0f) * ((j == 0 || j == nlat - 1) ? 0.5f : 1.0f);
        s1 = s1 + w * fabsf(e);
        s2 = s2 + w * (e * e);
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    __syncthreads();                                               // fem_eval_err_kernel's barrier, kept: the same two on every lane
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
