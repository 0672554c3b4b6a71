/*
 * gadapt_mesh.h - C-ABI of the classical target-mesh generators: batched MMPDE5 and, further down, batched Monge-Ampere
 * (libgadapt_mesh.so; one node per lane up to 32 x 32, and a strided route with an fp64 potential up to 81 x 81).
 * The Monge-Ampere iteration that the entry points below share is stated once in g_adaptivity_amd/mesh_csrc/ma_iteration.h
 * (device side) and ma_host.h (the batch check and the launch geometry); a kernel file holds what is its monitor's own.
 *
 * The reference builds the target mesh `x_phys` of loss_type='mesh_loss' with the moving-mesh PDE "MMPDE5"
 * (classical_meshing/ma_mesh_1d.py:7-134, ma_mesh_2d.py:11-103, called from src/data.py:394-416): classical RK4 in
 * pseudo-time on
 *
 *   dX/dt = div(m grad X) / (tau m)          on the fixed computational grid xi, boundary nodes held,
 *
 * until the l1 size of one step's update falls to a tolerance.  The monitor m is evaluated on the computational grid,
 * never on the moving coordinates, so it is a constant of the iteration: the caller passes it as two arrays and the
 * kernel keeps coordinates, stage values and coefficients in registers and LDS for the whole loop.  One launch advances
 * a batch of meshes of mixed sizes and dimensions, each to its own stopping step.
 *
 * Per mesh b (`desc` is int32 [B, GADAPT_MMPDE5_DESC], fields GADAPT_MMPDE5_D_*):
 *   dim 1: N nodes; coordinates x [N]; ms [N-1] = m at the cell centres; m2 [N] = m at the nodes
 *   dim 2: N x N nodes, node = i * N + j (meshgrid(..., indexing='ij')); x, y [N*N]; ms [(N-1)*(N-1)], cell = i * (N-1) + j; m2 [N*N]
 *   right-hand side at an interior node, per index direction and per coordinate U:
 *       ms[here] * (U[next] - U[here]) - ms[previous cell] * (U[here] - U[previous])
 *   summed over the directions and multiplied by 1 / (dxi^2 tau m2[here]), dxi = 1 / (N - 1) (hoisted out of the loop;
 *   the reference divides three times at every evaluation).  fp32, no FMA contraction.
 *   loop:  while (steps < max_steps && measure > tol) { ++steps; RK4 step of size step[b];
 *                                                        measure = sum |new - old| of the stored fp32 coordinates;
 *                                                        if (measure > 1 / tol) break; }
 *   tol == 0 switches the stopping test off: exactly max_steps steps.  A NaN measure ends the loop.
 * All meshes are concatenated: nodes of mesh b start at desc[b].NODE_OFF in x0, y0, m2, x, y (y0 / y are not touched for
 * dim 1), cells at desc[b].CELL_OFF in ms.  The arithmetic of a mesh, the order of its reduction included, depends on its
 * own size only: a mesh gives the same bits alone and in any batch.
 *
 * Two routes run this arithmetic.  gadapt_mmpde5_batch holds one node per lane of one workgroup: 1-D N <= 1024, 2-D N <= 32.
 * gadapt_mmpde5_batch_strided holds K = ceil(nodes / T) nodes per lane, T = min(nodes rounded up to whole waves, 1024):
 * lane t owns nodes t + k * T, and 2-D meshes go up to 81 a side (K <= 7; 105 104 bytes of LDS at 81 x 81).  There the measure
 * is summed in a fixed order: a lane adds |dx| + |dy| of its nodes in increasing k, the 64 lanes of a wave are summed as on the
 * other route, then the waves in increasing order.  For K = 1 the two orders are the same, so a mesh of at most 1024 nodes
 * gives the same bits on both routes.
 *
 * Conventions as in gadapt_hip.h: plain pointers, `stream` is a hipStream_t passed as void*.  Entry points return 0 or a
 * negative GADAPT_MESH_E_* code and never abort; gadapt_mesh_last_error() gives the message.  The launch function neither
 * allocates nor synchronises, and checks every size on the host copy of `desc` before anything is launched.
 */
#ifndef GADAPT_MESH_H
#define GADAPT_MESH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GADAPT_MESH_ABI 2

#define GADAPT_MESH_OK         0
#define GADAPT_MESH_E_BADARG  -1   /* null pointer, bad dimension, offset or parameter */
#define GADAPT_MESH_E_LAUNCH  -2   /* hipGetLastError() after the launch, or the strided route's LDS was refused */
#define GADAPT_MESH_E_SIZE    -3   /* a mesh has more nodes than one workgroup holds, or max_steps is beyond the cap */

/* Nodes per mesh on the one-node-per-lane route: 1-D N <= 1024, 2-D N <= 32 a side (the strided route: 2-D N <= 81). */
#define GADAPT_MMPDE5_MAX_NODES 1024
/* The loop always ends: max_steps is bounded on the host. */
#define GADAPT_MMPDE5_MAX_STEPS 10000000

/* desc fields, per mesh */
#define GADAPT_MMPDE5_D_DIM      0
#define GADAPT_MMPDE5_D_N        1
#define GADAPT_MMPDE5_D_NODE_OFF 2
#define GADAPT_MMPDE5_D_CELL_OFF 3
#define GADAPT_MMPDE5_DESC       4

/* status, per mesh */
#define GADAPT_MMPDE5_CONVERGED 0   /* measure <= tol */
#define GADAPT_MMPDE5_CAP       1   /* max_steps reached with measure > tol (always, when tol == 0) */
#define GADAPT_MMPDE5_STIFF     2   /* measure > 1 / tol, or not finite: the step is too large for this monitor */

int gadapt_mesh_abi_version(void);
const char* gadapt_mesh_last_error(void);
int gadapt_mmpde5_max_nodes(void);
int gadapt_mmpde5_max_steps(void);

/* Threads one mesh of `nodes` nodes works with (a multiple of 64; a launch uses the largest of its batch), or a negative code. */
int gadapt_mmpde5_threads(int nodes);
/* Dynamic LDS of a launch whose largest mesh has `nodes` nodes. */
int64_t gadapt_mmpde5_lds_bytes(int nodes);

/* One launch, one workgroup per mesh.
 *   in   desc_host / desc [B, 4] (the same values on the host and on the device), x0, y0, ms, m2 (device, fp32),
 *        step [B] (device, fp64: the RK4 step of each mesh, the reference's CFL / N^3), tau, tol, max_steps
 *   out  x, y (device, fp32; buffers of their own), steps [B] int32, measure [B] fp32, status [B] int32 */
int gadapt_mmpde5_batch(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* x0, const float* y0,
                        const float* ms, const float* m2, const double* step, double tau, double tol, int max_steps,
                        float* x, float* y, int32_t* steps, float* measure, int32_t* status, void* stream);

/* The strided route: 1-D meshes up to 1024 nodes and 2-D meshes up to gadapt_mmpde5_strided_max_side() (81) a side in one
 * launch; arguments, outputs and status words as gadapt_mmpde5_batch.  GADAPT_MESH_E_SIZE for a larger mesh,
 * GADAPT_MESH_E_LAUNCH if the device refuses the launch or its LDS. */
int gadapt_mmpde5_strided_max_side(void);
/* Dynamic LDS of a strided launch whose largest mesh has `nodes` nodes (3..6561). */
int64_t gadapt_mmpde5_strided_lds_bytes(int nodes);
int gadapt_mmpde5_batch_strided(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* x0, const float* y0,
                                const float* ms, const float* m2, const double* step, double tau, double tol, int max_steps,
                                float* x, float* y, int32_t* steps, float* measure, int32_t* status, void* stream);

/*
 * Monge-Ampere target meshes (2-D, up to 32 x 32): the reference's default 2-D target (classical_meshing/ma_mesh_2d.py:163-295,
 * src/data.py:208-210) solves, with Firedrake and `movement`, for a convex potential phi on the computational square with
 *   x = xi + grad phi,   m(x) det(I + H phi) = theta,   grad phi . n = 0.
 * Here the same equation is relaxed by finite differences in pseudo-time; parity with `movement` is not pinned.
 *
 * Per mesh b (`desc` is int32 [B, GADAPT_MA_DESC], fields GADAPT_MA_D_*): N x N nodes, node = i * N + j, xi_i = (float)i / (float)(N - 1).
 * phi [N, N] is fp32, starts at 0 and is continued by even reflection at every edge (phi[-1, j] = phi[1, j], phi[N, j] = phi[N-2, j],
 * likewise in j, a corner's diagonal neighbour in both).  With n1 = N - 1 (h = 1 / n1), per node, fp32 without FMA contraction:
 *   px  = (phi[i+1,j] - phi[i-1,j]) * (n1 / 2)                        py likewise in j
 *   a   = 1 + (phi[i+1,j] - 2 phi[i,j] + phi[i-1,j]) * n1^2           b likewise in j
 *   c   = (phi[i+1,j+1] - phi[i+1,j-1] - phi[i-1,j+1] + phi[i-1,j-1]) * (n1^2 / 4)
 *   x   = xi_i + px,  y = xi_j + py          (the reflection makes px exactly 0 at i = 0 and i = N - 1: boundary nodes keep
 *                                             their normal coordinate bit for bit, corners do not move)
 *   det = a b - c^2,  lambda = ((a + b) - sqrt((a - b)^2 + 4 c^2)) / 2
 *   per Gaussian k (gauss[k] = c0, c1, s0, s1;  q0 = s0^2, q1 = s1^2;  A0 = 4 / q0^2, B0 = 2 / q0, A1, B1 likewise, once per mesh):
 *       dx2 = (x - c0)^2,  dy2 = (y - c1)^2,  g = expf(-(dx2 / q0) - dy2 / q1)   with the quotients as products by 1 / q0, 1 / q1
 *       u_xx += (A0 dx2 - B0) g,   u_yy += (A1 dy2 - B1) g
 *   m   = powf(mon[b][0] + sqrtf(u_xx^2 + u_yy^2), mon[b][1])         ((mon_reg, mon_power); (1, 0.2) is the default monitor)
 *   r   = logf(m det)
 * Per step: rbar = (sum of w r) / n1^2 with w = 1 inside, 1/2 on an edge, 1/4 at a corner (the 64 lanes of a wave as in the
 * MMPDE5 sum, then the waves in increasing order); res = max(max r - rbar, rbar - min r); lmin = min lambda;
 *   if (!(lmin > 0) || res is not finite) stop, NONCONVEX;  else if (tol > 0 && res <= tol) stop, CONVERGED;
 *   else if (steps == max_steps) stop, CAP;  else phi += (float)(cfl / n1^2) * min(1, lmin) * (r - rbar), ++steps.
 * Outputs: x, y of the last evaluated phi, the number of updates, res, status.  A mesh without Gaussians has a constant
 * monitor: 0 steps and the grid itself.  tol == 0 runs exactly max_steps updates; max_steps <= GADAPT_MMPDE5_MAX_STEPS.
 * One workgroup per mesh, one lane per node; the arithmetic of a mesh depends on its own size only.
 */
#define GADAPT_MA_D_N         0
#define GADAPT_MA_D_NODE_OFF  1
#define GADAPT_MA_D_GAUSS_OFF 2
#define GADAPT_MA_D_GAUSS_N   3
#define GADAPT_MA_DESC        4

#define GADAPT_MA_CONVERGED 0   /* res <= tol */
#define GADAPT_MA_CAP       1   /* max_steps updates done with res > tol (always, when tol == 0) */
#define GADAPT_MA_NONCONVEX 2   /* min lambda <= 0 or res not finite: the map stopped being a convex potential's gradient */

int gadapt_ma_max_side(void);    /* 32 */
int gadapt_ma_max_gauss(void);   /* 8 */
/* Dynamic LDS of a launch whose largest mesh has `nodes` nodes (9..1024). */
int64_t gadapt_ma_lds_bytes(int nodes);

/* One launch, one workgroup per mesh.
 *   in   desc_host / desc [B, 4] (the same values on the host and on the device), gauss [G_total, 4] and mon [B, 2]
 *        (device, fp32), cfl > 0, tol >= 0, max_steps
 *   out  x, y (device, fp32, [total nodes]), steps [B] int32, residual [B] fp32, status [B] int32
 * GADAPT_MESH_E_SIZE for N > 32, more than 8 Gaussians or max_steps beyond the cap; neither allocates nor synchronises. */
int gadapt_ma_batch(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* gauss, const float* mon, double cfl,
                    double tol, int max_steps, float* x, float* y, int32_t* steps, float* residual, int32_t* status, void* stream);

/*
 * The strided route: Monge-Ampere meshes up to gadapt_ma_strided_max_side() (81) a side, with an fp64 potential.  The fp32
 * iteration above stalls against its rounding floor as the mesh grows (its residual floor reaches tol near 64 x 64), so this
 * route is not the same arithmetic on more nodes: it is the iteration above with these changes and no others.
 *   phi [N, N] is fp64 (it starts at 0 and is reflected as above).
 *   The five stencil expressions are formed in fp64 from the fp64 phi, with the association and the exact constants above,
 *   and each is rounded once to fp32:
 *       px = (float)((phi[i+1,j] - phi[i-1,j]) * (n1 / 2))                                      py likewise in j
 *       a  = (float)(1 + ((phi[i+1,j] - 2 phi[i,j]) + phi[i-1,j]) * n1^2)                       b likewise in j
 *       c  = (float)((((phi[i+1,j+1] - phi[i+1,j-1]) - phi[i-1,j+1]) + phi[i-1,j-1]) * (n1^2 / 4))
 *   Everything after that is the fp32 above, operation for operation: x = xi_i + px, det, lambda, the Gaussians, m,
 *   r = logf(m det).
 *   One workgroup per mesh, T = min(nodes rounded up to whole waves, 1024) lanes, K = ceil(nodes / T) <= 7 nodes per lane, lane t
 *   owning nodes t + k T (the ownership of gadapt_mmpde5_batch_strided).  Reductions: a lane starts from 0, -inf, +inf, +inf and,
 *   over its own slots in increasing k, adds w r, takes the max and the min of r and the min of lambda; then the 64 lanes of a
 *   wave as above; then the waves in increasing order, read back from LDS by every lane alike, so that no lane decides an
 *   exit from a value it computed alone.  Lanes and slots without a node contribute 0, -inf, +inf, +inf.
 *   The exit tests are those above, in that order: NONCONVEX, then CONVERGED, then CAP.
 *   Update: phi += (double)(((float)(cfl / n1^2) * fminf(1, lmin)) * (r - rbar)): the increment is formed in fp32 and added in fp64.
 * T, K and the order of the reductions follow from the mesh's own node count only: a mesh gives the same bits alone and in any
 * batch.  The two routes do NOT give the same bits at N <= 32: phi is fp64 here and fp32 there.
 * With the default cfl = 0.2 and tol = 1e-4, 64 x 64 wanted 17 500 to 25 500 updates in the cases tried and 81 x 81
 * 28 000 to 32 000: the default max_steps of the Python callers (20 000) can return CAP there.
 * Arguments, descriptor, outputs, status words and error codes are those of gadapt_ma_batch; GADAPT_MESH_E_SIZE for N > 81, more
 * than 8 Gaussians or max_steps beyond the cap; neither allocates nor synchronises.  The launch's dynamic LDS (one fp64 image of
 * phi, the wave partials and the Gaussians' constants: 53 000 bytes at 81 x 81) stays below the 64 KB that need no raised limit.
 */
int gadapt_ma_strided_max_side(void);   /* 81 */
/* Dynamic LDS of a strided launch whose largest mesh has `nodes` nodes (9..6561). */
int64_t gadapt_ma_strided_lds_bytes(int nodes);
int gadapt_ma_batch_strided(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* gauss, const float* mon,
                            double cfl, double tol, int max_steps, float* x, float* y, int32_t* steps, float* residual,
                            int32_t* status, void* stream);

/*
 * The M2N 'fast' monitor: the reference's MA2d with mesh_type = 'M2N' and fast_M2N_monitor = 'fast'
 * (classical_meshing/ma_mesh_2d.py:263-272), the value its run parameters select for M2N.  The monitor of a node is scaled by a
 * maximum over the mesh's current nodes, so it moves with the mesh:
 *   m(x, y) = mon_reg + beta F(x, y) / max over the nodes of F,   F = sqrt(u_xx^2 + 2 u_xy^2 + u_yy^2).
 * The 'slow' and 'superslow' monitors add a Poisson solve on the moving mesh per evaluation: 'slow' is gadapt_ma_m2n_slow_batch
 * further down, 'superslow' is not built.  gadapt_ma_m2n_batch
 * is the iteration of gadapt_ma_batch above with these changes and no others:
 *   Per mesh, once: the Gaussians' constants above, and Cxy = (16 * (1 / q0)) * (1 / q1) of the LAST Gaussian of the mesh.  The
 *   reference assigns u_xy with `=` inside its loop over the Gaussians (ma_mesh_2d.py:133,151), so only the last Gaussian's u_xy
 *   survives; that is kept.
 *   Per node, fp32 without FMA contraction, after u_xx and u_yy (the signed sums above):
 *       u_xy = (Cxy * (dx * dy)) * g        with dx = x - c0, dy = y - c1 and g of the last Gaussian (0 without Gaussians)
 *       F    = sqrtf((u_xx*u_xx + 2.0f*(u_xy*u_xy)) + u_yy*u_yy)
 *   Per step: Fmax = max of F over the mesh's nodes, reduced like the other extremes: lanes without a node give -inf, then the
 *   64 lanes of a wave, then the waves in increasing order, read back from LDS by every lane alike.  Then per node
 *       m = mon[b][0] + (Fmax > 0 ? mon[b][1] * (F / Fmax) : 0)            (mon[b] = (mon_reg, beta); there is no powf)
 *       r = logf(m det)
 *   A mesh without Gaussians, or whose F underflows to 0 at every node, has the constant monitor mon_reg: 0 updates and the grid
 *   itself.  That choice is made on Fmax as read from LDS, never by a lane from its own F.
 *   rbar, res, lmin, the three exit tests and their order, the update, the status words, the descriptor, cfl, tol and
 *   max_steps are unchanged.  Three barriers a step instead of two (F, then Fmax and r, then the combine), and a fifth row of
 *   wave partials for Fmax.
 * gadapt_ma_m2n_batch_strided is gadapt_ma_batch_strided with the same changes: fp64 phi, the five stencil expressions rounded
 * once, the rest in fp32.  A lane folds F over its own slots in increasing k, starting from -inf, before the wave step; F and
 * det of a slot (det itself, not its logarithm) are what a lane keeps until Fmax is known.
 * Arguments, outputs, limits (32 and 81 a side, 8 Gaussians) and error codes are those of the two entry points above.
 * Dynamic LDS: 4 * (5*16 + 8*8 + 4 + 2 * nodes) bytes on the lane route (the 4 floats hold Cxy), 592 + 8 * nodes on the strided
 * route (53 080 bytes at 81 x 81).
 */
int64_t gadapt_ma_m2n_lds_bytes(int nodes);           /* 9..1024 nodes */
int64_t gadapt_ma_m2n_strided_lds_bytes(int nodes);   /* 9..6561 nodes */
int gadapt_ma_m2n_batch(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* gauss, const float* mon, double cfl,
                        double tol, int max_steps, float* x, float* y, int32_t* steps, float* residual, int32_t* status,
                        void* stream);
int gadapt_ma_m2n_batch_strided(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* gauss, const float* mon,
                                double cfl, double tol, int max_steps, float* x, float* y, int32_t* steps, float* residual,
                                int32_t* status, void* stream);

/*
 * The M2N 'slow' monitor (classical_meshing/ma_mesh_2d.py:227-261; the reference's argparse default for fast_M2N_monitor):
 *   m = mon_reg + alpha (u_h - u)^2 / max + beta F / max,
 * u = the sum of the Gaussians, u_h the P1 finite-element solution of -Laplace(u_h) = f = -(u_xx + u_yy), u_h = u on the boundary,
 * ON THE MOVING MESH, solved again at every monitor evaluation; both maxima over the mesh's current nodes.  'superslow'
 * (it differentiates a high-order solution) is not built.  Stated deviations, parity being unpinned as above: the reference
 * L2-projects f and u into P1 and solves with Firedrake, here both are nodal values; u_xy is still the last Gaussian's only.
 * gadapt_ma_m2n_slow_batch is the iteration of gadapt_ma_m2n_batch on the lane route (one workgroup per mesh, one lane per node,
 * fp32, no FMA contraction) with these changes and no others:
 *   In the loop over the Gaussians each node also forms u = u + g (from 0); after the loop f = -(u_xx + u_yy).
 *   The mesh is square_mesh(N)'s: node (i, j) = i N + j; quad (ix, iy) has v0 = (ix, iy), v1 = (ix, iy+1), v2 = (ix+1, iy+1),
 *   v3 = (ix+1, iy) and is cut into the triangles (v0, v1, v3) ("lower") and (v1, v2, v3) ("upper").
 *   The solve: x, y, u, f of all nodes go to LDS.  Interior node (i, j), 1 <= i, j <= N - 2, is row r = (i-1)(N-2) + (j-1);
 *   w = N - 2 is the half-bandwidth, n_int = w^2.   K_II c = b_I - K_IB u_B,  with per triangle (p0, p1, p2), as in fem_factor_kernel:
 *       r0 = (p1.y - p2.y, p2.x - p1.x), r1 = (p2.y - p0.y, p0.x - p2.x), r2 = (p0.y - p1.y, p1.x - p0.x)
 *       D  = p0.x (p1.y - p2.y) + p1.x (p2.y - p0.y) + p2.x (p0.y - p1.y),   inv = 1 / (2 |D|),   p_lk = (r_l . r_k) * inv
 *   and the consistent P1 mass matrix applied to the nodal f as the load: (|D| / 24) * (f_l + ((f_0 + f_1) + f_2)).
 *   The lane of node (i, j) owns band row r (K[r][r-d] at r (w+1) + d) and b[r].  From zeros it gathers its six triangles in the
 *   order of their cell numbers: lower of quad (i-1, j) (the node is vertex l = 2), lower of (i, j-1) (l = 1), lower of (i, j)
 *   (l = 0), upper of (i-1, j-1) (l = 1), upper of (i-1, j) (l = 2), upper of (i, j-1) (l = 0).  Per triangle: b += load; then for
 *   k = 0, 1, 2: a boundary vertex gives b -= p_lk u_k, an interior vertex of row r' <= r gives K[r][r'] += p_lk.
 *   Banded Cholesky in fp32, in LDS, right-looking: per column k, d = sqrtf(K[k][k]) if K[k][k] > 0 else NaN;
 *   L[k+i][k] = K[k+i][k] / d and b[k] = b[k] / d; then K[k+i][k+j] -= L[k+i][k] L[k+j][k] for 1 <= j <= i <= w (rows below
 *   n_int skipped) and b[k+i] -= L[k+i][k] b[k].  Backwards, k = n_int - 1 .. 0: y = b[k] / d_k, b[k-j] -= L[k][k-j] y; c_r = b[r] / d_r.
 *   e = c - u at interior nodes and exactly 0 on the boundary.
 *   The monitor: E = e*e; Emax is reduced exactly like Fmax (lanes without a node give -inf, then the 64 lanes of a wave, then the
 *   waves in increasing order, read back from LDS by every lane alike), in a partial row of its own.  Then per node
 *       m = (mon[b][0] + (Emax > 0 ? mon[b][1] * (E / Emax) : 0)) + (Fmax > 0 ? mon[b][2] * (F / Fmax) : 0)
 *   with mon[b] = (mon_reg, alpha, beta), so mon is [B, 3]; both choices are made on the LDS values.  A pivot that is not
 *   positive makes m NaN at every node (every lane reads every pivot from LDS), so it arrives as NaN in res and ends the loop
 *   as NONCONVEX.  alpha = 0 gives the bits of gadapt_ma_m2n_batch with the same mon_reg and beta: reg + 0 is exact.
 *   rbar, res, lmin, the three exit tests and their order, the update, the status words, the descriptor, cfl, tol and max_steps
 *   are unchanged.  3 n_int + 5 barriers an update, each reached by every lane of the workgroup: all trip counts follow from N.
 * Limits: N <= gadapt_ma_m2n_slow_max_side() (24; the band has to stay in LDS), 8 Gaussians.  Dynamic LDS of a launch whose largest
 * mesh has N x N nodes: 4 * (6*16 + 8*8 + 4 + 6 N^2 + (N-2)^2 (N-1) + (N-2)^2) bytes, 60 944 at 24 x 24, below the 64 KB that need no
 * raised limit.  Arguments, checks and error codes are those of gadapt_ma_m2n_batch, with mon3 [B, 3] and one more output:
 * monitor_out [total nodes] (device, fp32; may be null) receives m of the last evaluation, so max_steps = 0 with tol = 0 gives the
 * monitor of the uniform grid: the solve alone.
 */
int gadapt_ma_m2n_slow_max_side(void);                /* 24 */
int64_t gadapt_ma_m2n_slow_lds_bytes(int nodes);      /* N x N nodes, 3 <= N <= 24 */
int gadapt_ma_m2n_slow_batch(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* gauss, const float* mon3,
                             double cfl, double tol, int max_steps, float* x, float* y, int32_t* steps, float* residual,
                             int32_t* status, float* monitor_out, void* stream);

/*
 * Monge-Ampere meshes from a TABULATED monitor: the monitor is not a closed form of the sample's Gaussians but a table on a
 * lattice of the physical unit square, so a mesh can be adapted to any nodal field (a computed coarse solution, say).
 * gadapt_ma_table_batch is the iteration of gadapt_ma_batch and gadapt_ma_table_batch_strided that of gadapt_ma_batch_strided,
 * each with this change and no other: the lines "per Gaussian k" and "m = powf(...)" are replaced by a bilinear read of the
 * mesh's own table M [T, T] (fp32, row-major), M[i, j] being the monitor at the physical point (i / (T-1), j / (T-1)), the
 * 'ij' convention of the coordinates.  Per node, fp32 without FMA contraction:
 *   xc = x > 0 ? (x < 1 ? x : 1) : 0            (a NaN maps to 0: no index is ever formed from a NaN)     yc likewise
 *   fx = xc * (float)(T-1),  i0 = min((int)fx, T-2),  ax = fx - (float)i0                                 fy, j0, ay likewise
 *   m0 = M[i0,j0]   + ax * (M[i0+1,j0]   - M[i0,j0])
 *   m1 = M[i0,j0+1] + ax * (M[i0+1,j0+1] - M[i0,j0+1])
 *   m  = m0 + ay * (m1 - m0)
 *   r  = logf(m det)
 * The form is continuous across table cells (a node whose i0 differs between two arithmetics costs rounding only) and exact for
 * tables linear in x and y.  Nodes with x == 1 exactly (every mesh has them: boundary nodes keep their normal coordinate) give
 * i0 = T-2, ax = 1: the last row and column are read, in bounds.  A table entry that is <= 0 or not finite has no check of its
 * own: it makes r not finite, which is the NONCONVEX exit.  A constant table gives 0 updates and the grid itself.
 * px, py, a, b, c, x, y, det, lambda, rbar, res, lmin, the reductions and their order, the three exit tests and their order, the
 * update, the status words, cfl, tol and max_steps are unchanged; on the strided route so are the fp64 phi, the five stencil
 * expressions rounded once to fp32, the ownership t + k T and the fp32 increment added in fp64.  The two routes do not give the
 * same bits at N <= 32, as above.
 * `desc` is int32 [B, GADAPT_MA_DESC] with GADAPT_MA_D_N and GADAPT_MA_D_NODE_OFF as above, GADAPT_MA_D_TABLE_OFF the offset of
 * the mesh's table in `tables`, in floats, and GADAPT_MA_D_TABLE_T its side.  `tables` is one device buffer [sum of T_b^2], fp32;
 * every mesh has its own T, 2 <= T <= gadapt_ma_table_max_side() (1024).  The table is read from global memory on both routes;
 * the launch's dynamic LDS is 256 + 8 N^2 bytes (two fp32 images on the lane route, one fp64 image on the strided one), 52 744
 * at 81 x 81.
 * Arguments are those of gadapt_ma_batch with `tables` in the place of `gauss` and without `mon`; outputs and error codes are
 * the same: GADAPT_MESH_E_SIZE for N above the route's side (32, 81), T outside 2..1024 or max_steps beyond the cap; neither
 * allocates nor synchronises.
 */
#define GADAPT_MA_D_TABLE_OFF 2   /* the word of GADAPT_MA_D_GAUSS_OFF */
#define GADAPT_MA_D_TABLE_T   3   /* the word of GADAPT_MA_D_GAUSS_N */

int gadapt_ma_table_max_side(void);                   /* 1024 */
int gadapt_ma_table_batch(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* tables, double cfl, double tol,
                          int max_steps, float* x, float* y, int32_t* steps, float* residual, int32_t* status, void* stream);
int gadapt_ma_table_batch_strided(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* tables, double cfl,
                                  double tol, int max_steps, float* x, float* y, int32_t* steps, float* residual, int32_t* status,
                                  void* stream);

#ifdef __cplusplus
}
#endif

#endif
