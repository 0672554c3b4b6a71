// fem_wave_grad_kernels.hip - the wave-parallel form of the two lattice walks of the backward (fem_adjoint='wave':
// gadapt_fem_backward_wave, gadapt_fem_backward_window_wave in include/gadapt_fem.h).
//
// This file is compiled inside fem_kernels.hip's translation unit, after fem_window_grad_kernels.hip: it calls
// fem_kernels.hip's lattice_range, simpson_box and tri_geometry and the fem:: helpers.  The entry points are at that file's end.
//
// fem_gc_kernel gives a node to a lane and fem_tri_bwd_kernel a triangle to a lane; each lane then walks every lattice
// point of its triangles' bounding boxes alone, so a 11 x 11 mesh keeps 121 and 200 lanes busy.  Here a node, or a triangle,
// is a wave's.  A result of the lane kernels is a chain of fp32 additions in a fixed order; the wave computes the ADDENDS
// 64 at a time, with the same helpers on the same arguments (no FMA contraction: the same bits), leaves them in an LDS slab
// in point order, and the lane that owns a chain adds them in the lane kernel's order.  An addend the lane kernel skips
// (ind == 0, inc == 0) is skipped here too: the round's ballot says which points were added.  The results are the lane
// kernels', bit for bit.
//
// Launch shape.  A workgroup is ONE wave: the loop counts depend on the node's or the triangle's boxes, which every lane of
// a wave reads from the same addresses, so every barrier is reached by the whole workgroup; the grid is n_nodes or n_tris
// workgroups, and the range exit in front of the barriers is taken by a whole workgroup or not at all.  A box of any size
// is walked in rounds of 64 points with the chains carried in registers: the slab is 64 points whatever nlat is (256 B and
// 4 680 B of static LDS).  No scratch, no atomics.
#define FEM_WAVE 64
#define FEM_WAVE_LD (FEM_WAVE + 1)                                 // slab row stride: the six chain lanes read six banks

// gc[v] = g_coeffs[v] + sum_p g_sol[p] phim(p, v), fem_gc_kernel's sum: v's incidences in CSR order, each box i outer, j inner
__global__ void __launch_bounds__(FEM_WAVE) fem_gc_wave_kernel(int n_nodes, const int32_t* __restrict__ cells, const int32_t* __restrict__ node_mesh,
                                                               const int32_t* __restrict__ nt_ptr, const int32_t* __restrict__ nt_idx,
                                                               const float* __restrict__ x, const float* __restrict__ lat_x,
                                                               const float* __restrict__ lat_y, int nlat, const float* __restrict__ g_coeffs,
                                                               const float* __restrict__ g_sol, float* __restrict__ gc) {
    __shared__ float slab[FEM_WAVE];
    const int v = blockIdx.x, lane = threadIdx.x;
    if (v >= n_nodes) return;                                      // the whole workgroup
    float acc = g_coeffs ? g_coeffs[v] : 0.0f;                     // lane 0's is the chain
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
            const int nj = j1 - j0 + 1, npts = (i1 - i0 + 1) * nj;
            for (int k0 = 0; k0 < npts; k0 += FEM_WAVE) {
                const int k = k0 + lane;
                bool added = false;
                if (k < npts) {
                    const int i = i0 + k / nj, j = j0 + k % nj;
                    const float px = lat_x[i], py = lat_y[j];
                    const float ind = fem::inside(px, py, a, b, c);
                    if (ind != 0.0f) {
                        const float inc = fem::aux_value(px, py, a, b, c, ind);
                        if (inc != 0.0f) {
                            const float div = fem::phim_parts(px, py, v, nt_ptr, nt_idx, cells, x, nullptr);
                            slab[lane] = gs[i * nlat + j] * (inc / div);
                            added = true;
                        }
                    }
                }
                const unsigned long long bits = __ballot(added);
                __syncthreads();
                if (lane == 0)
                    for (unsigned long long m = bits; m; m &= m - 1) acc = acc + slab[__builtin_ctzll(m)];   // the added points, in order
                __syncthreads();                                   // the slab is free for the next round
            }
        }
    }
    if (lane == 0) gc[v] = acc;
}

// fem_tri_bwd_kernel's stiffness part as written there: E = sum_ab Abar_ab r_a.r_b / (2|D|), Abar_ab = -mu_a c_b
__device__ inline void wave_stiffness(const int vtx[3], const V2 p[3], const float* __restrict__ coeffs, const float* __restrict__ mu, V2 g[3]) {
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
    const float coef = -R * sgn * inv * inv * 2.0f;              // -R sign(D) / (2 D^2)
    for (int k = 0; k < 3; ++k) { g[k].x += coef * r[k].x; g[k].y += coef * r[k].y; }
}

// which of (ga, gb, gcv) of rotation l add_rot adds to g[k]: 0, 1 or 2
__device__ inline int rot_slot(int k, int l) { return k == l ? 2 : (k == (l + 2) % 3 ? 0 : 1); }

// d L / d (vertices of t), fem_tri_bwd_kernel's sums.  tgrad[t] is six chains, g[k].x and g[k].y: lane 2 k + comp owns one.
// Its order there: the stiffness terms; per interior vertex l = 0, 1, 2 one addend, the sum from zero of the Simpson
// points' terms in (i, j) order; then per lattice point in (i, j) order the terms of l = 0, 1, 2.
__global__ void __launch_bounds__(FEM_WAVE) fem_tri_bwd_wave_kernel(int n_tris, const int32_t* __restrict__ cells, const int32_t* __restrict__ tri_mesh,
                                                                    const int32_t* __restrict__ int_idx, const int32_t* __restrict__ nt_ptr,
                                                                    const int32_t* __restrict__ nt_idx, const int32_t* __restrict__ gptr,
                                                                    const float* __restrict__ gpar, const float* __restrict__ x,
                                                                    const float* __restrict__ lat_x, const float* __restrict__ lat_y, int nlat,
                                                                    const float* __restrict__ coeffs, const float* __restrict__ mu,
                                                                    const float* __restrict__ g_sol, float* __restrict__ tgrad) {
    __shared__ float slab[18 * FEM_WAVE_LD];                       // row 6 l + 2 s + comp: (ga, gb, gcv)[s] of rotation l; column: point
    const int t = blockIdx.x, lane = threadIdx.x;
    if (t >= n_tris) return;                                       // the whole workgroup
    const int b = tri_mesh[t];
    const int vtx[3] = {cells[3 * t], cells[3 * t + 1], cells[3 * t + 2]};
    const V2 p[3] = {ld2(x, vtx[0]), ld2(x, vtx[1]), ld2(x, vtx[2])};
    const bool owner = lane < 6;
    const int k = owner ? lane >> 1 : 0, comp = lane & 1;
    const int row0 = 2 * rot_slot(k, 0) + comp, row1 = 6 + 2 * rot_slot(k, 1) + comp, row2 = 12 + 2 * rot_slot(k, 2) + comp;

    // stiffness: on lane 0 as fem_tri_bwd_kernel writes it; each chain's start goes to its owner through the slab
    if (lane == 0) {
        V2 g[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
        wave_stiffness(vtx, p, coeffs, mu, g);
        slab[0] = g[0].x; slab[1] = g[0].y; slab[2] = g[1].x; slab[3] = g[1].y; slab[4] = g[2].x; slab[5] = g[2].y;
    }
    __syncthreads();
    float gk = owner ? slab[lane] : 0.0f;                          // this lane's chain
    __syncthreads();

    // load vector: the 81 Simpson points of vertex l's box over the lanes
    const int g0 = gptr[b], g1 = gptr[b + 1];
    constexpr int n = FEM_SIMPSON_N;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const int m = cells[3 * t + l];                            // vtx[l], without indexing the array by a loop count
        if (int_idx[m] < 0) continue;
        const float lam = -mu[m];
        int va, vb, vc;
        fem::rotation(cells, t, l, va, vb, vc);
        const V2 a = ld2(x, va), bb = ld2(x, vb), c = ld2(x, vc);
        float bx0, bx1, by0, by1;
        simpson_box(m, nt_ptr, nt_idx, cells, x, bx0, bx1, by0, by1);
        const float hx3 = (bx1 - bx0) / (float)(n - 1) / 3.0f, hy3 = (by1 - by0) / (float)(n - 1) / 3.0f;
        const int row = l == 0 ? row0 : (l == 1 ? row1 : row2);
        float s = 0.0f;                                            // ga, gb or gcv (.x or .y) of this l, from zero
        for (int k0 = 0; k0 < n * n; k0 += FEM_WAVE) {
            const int q = k0 + lane;
            bool added = false;
            if (q < n * n) {
                const int i = q / n, j = q % n;
                const float px = fem::linspace_at(bx0, bx1, n, i), py = fem::linspace_at(by0, by1, n, j);
                const float ind = fem::inside(px, py, a, bb, c);
                if (ind != 0.0f) {
                    const float div = fem::phim_parts(px, py, m, nt_ptr, nt_idx, cells, x, nullptr);
                    const float w = lam * (hx3 * fem::simpson_coef(i, n)) * (hy3 * fem::simpson_coef(j, n)) * fem::forcing(px, py, gpar, g0, g1) / div;
                    V2 ga = {0.f, 0.f}, gb = {0.f, 0.f}, gcv = {0.f, 0.f};
                    fem::aux_grad(px, py, a, bb, c, ind * w, ga, gb, gcv);
                    float* o = slab + 6 * l * FEM_WAVE_LD + lane;
                    o[0] = ga.x; o[FEM_WAVE_LD] = ga.y; o[2 * FEM_WAVE_LD] = gb.x; o[3 * FEM_WAVE_LD] = gb.y;
                    o[4 * FEM_WAVE_LD] = gcv.x; o[5 * FEM_WAVE_LD] = gcv.y;
                    added = true;
                }
            }
            const unsigned long long bits = __ballot(added);
            __syncthreads();
            if (owner)
                for (unsigned long long mm = bits; mm; mm &= mm - 1) s = s + slab[row * FEM_WAVE_LD + __builtin_ctzll(mm)];
            __syncthreads();
        }
        gk = gk + s;                                               // add_rot
    }

    // evaluation: the lattice points of t's bounding box over the lanes
    if (g_sol) {
        const float* gs = g_sol + (int64_t)b * nlat * nlat;
        int i0, i1, j0, j1;
        lattice_range(fminf(fminf(p[0].x, p[1].x), p[2].x), fmaxf(fmaxf(p[0].x, p[1].x), p[2].x), lat_x[0], lat_x[nlat - 1], nlat, i0, i1);
        lattice_range(fminf(fminf(p[0].y, p[1].y), p[2].y), fmaxf(fmaxf(p[0].y, p[1].y), p[2].y), lat_y[0], lat_y[nlat - 1], nlat, j0, j1);
        const int nj = j1 - j0 + 1, npts = (i1 - i0 + 1) * nj;
        for (int k0 = 0; k0 < npts; k0 += FEM_WAVE) {
            const int q = k0 + lane;
            bool added = false;
            if (q < npts) {
                const int i = i0 + q / nj, j = j0 + q % nj;
                const float px = lat_x[i], py = lat_y[j];
                const float ind = fem::inside(px, py, p[2], p[1], p[0]);
                if (ind != 0.0f) {
                    const float gp = gs[i * nlat + j];
#pragma unroll
                    for (int l = 0; l < 3; ++l) {
                        int va, vb, vc;
                        fem::rotation(cells, t, l, va, vb, vc);
                        const float div = fem::phim_parts(px, py, vc, nt_ptr, nt_idx, cells, x, nullptr);
                        V2 ga = {0.f, 0.f}, gb = {0.f, 0.f}, gcv = {0.f, 0.f};
                        fem::aux_grad(px, py, ld2(x, va), ld2(x, vb), ld2(x, vc), ind * (gp * coeffs[vc] / div), ga, gb, gcv);
                        float* o = slab + 6 * l * FEM_WAVE_LD + lane;
                        o[0] = ga.x; o[FEM_WAVE_LD] = ga.y; o[2 * FEM_WAVE_LD] = gb.x; o[3 * FEM_WAVE_LD] = gb.y;
                        o[4 * FEM_WAVE_LD] = gcv.x; o[5 * FEM_WAVE_LD] = gcv.y;
                    }
                    added = true;
                }
            }
            const unsigned long long bits = __ballot(added);
            __syncthreads();
            if (owner)
                for (unsigned long long mm = bits; mm; mm &= mm - 1) {
                    const int qq = __builtin_ctzll(mm);
                    gk = gk + slab[row0 * FEM_WAVE_LD + qq];
                    gk = gk + slab[row1 * FEM_WAVE_LD + qq];
                    gk = gk + slab[row2 * FEM_WAVE_LD + qq];
                }
            __syncthreads();
        }
    }
    if (owner) tgrad[6 * t + lane] = gk;
}
