/*
 * gadapt_fem.h - C-ABI of the differentiable P1 finite-element tail of loss_type='pde_loss' (2-D Poisson).
 *
 * The reference solves -Laplace(u) = f on the moved mesh with a differentiable P1 FEM
 * (firedrake_difFEM/difFEM_2d.py:63-372, called from src/GNN.py:307-342) and trains the mesh
 * on the error of that solve.  This library does the same arithmetic for a whole batch of
 * meshes, forward and backward with respect to the node coordinates:
 *
 *   stiffness   P_T[a][b] = area_T grad(phi_a).grad(phi_b)       (A = -sum_T P_T, difFEM_2d.py:63-117)
 *   load        RHS_m = u_true(x_m) on the boundary (detached), else a 9 x 9 Simpson rule of
 *               phim(., m) f over the bounding box of m's incident triangles (:159-203, :298-309)
 *   solve       c_B = RHS_B;  P_II c_I = -RHS_I - P_IB c_B  by a banded Cholesky, band in LDS (:355-367)
 *   evaluation  sol(p) = sum_m c_m phim(p, m) on a tensor-product lattice (:312-318)
 *
 * phim follows the reference's hat-function rules literally (:16-61): an inclusive edge test,
 * evaluated in fp32 without FMA contraction, the sum over incident triangles divided by the number
 * of positive contributions.  Backward accumulates per node by gather over a node -> incident
 * triangle CSR: no float atomics, bit-reproducible.
 *
 * Conventions as in gadapt_hip.h: plain pointers, int32 indices, fp32 values, `stream` is a
 * hipStream_t passed as void*.  Entry points return 0 or a negative GADAPT_FEM_E_* code and never
 * abort; gadapt_fem_last_error() gives the message.  Launch functions neither allocate nor
 * synchronise; the *_host helpers run on the CPU.
 *
 * Batch layout.  Meshes b = 0..B-1 are concatenated: nodes [node_off[b], node_off[b+1]), triangles
 * [tri_off[b], tri_off[b+1]) with GLOBAL node ids in `cells` [T,3].  `meta` is int32 [B, GADAPT_FEM_META]
 * (fields GADAPT_FEM_M_*), built on the host by gadapt_fem_topology_host and copied to the device.
 *
 * The 1-D tails (gadapt_fem1d_*, fem_csrc/fem1d_kernels.hip) are declared at the end of this file.
 */
#ifndef GADAPT_FEM_H
#define GADAPT_FEM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4: also with gadapt_fem1d_spline, an addition that changes no existing signature (a library without it fails when the
 * caller resolves its table of prototypes). */
#define GADAPT_FEM_ABI 4

#define GADAPT_FEM_OK          0
#define GADAPT_FEM_E_BADARG   -1   /* null pointer, bad size, bad lattice */
#define GADAPT_FEM_E_LAUNCH   -2   /* hipGetLastError() after a launch */
#define GADAPT_FEM_E_RANGE    -3   /* node id outside its mesh */
#define GADAPT_FEM_E_LDS      -5   /* a mesh's band (or triangle bin mask) does not fit the LDS budget */

/* Simpson points per dimension of the load-vector rule (see fem_csrc/fem_common.h). */
#define GADAPT_FEM_SIMPSON_N 9
/* Bytes of LDS one mesh's factor kernel may use (gadapt_fem_factor_lds_bytes) and one mesh's bin mask (gadapt_fem_eval_lds_bytes). */
#define GADAPT_FEM_LDS_BUDGET 65536

/* meta fields, per mesh */
#define GADAPT_FEM_M_NODE_OFF 0
#define GADAPT_FEM_M_N_NODES  1
#define GADAPT_FEM_M_TRI_OFF  2
#define GADAPT_FEM_M_N_TRIS   3
#define GADAPT_FEM_M_INT_OFF  4   /* first interior slot of this mesh in int_node */
#define GADAPT_FEM_M_N_INT    5
#define GADAPT_FEM_M_BAND     6   /* half-bandwidth of P_II in the interior numbering */
#define GADAPT_FEM_M_BAND_OFF 7   /* first float of this mesh's band factor: sum over earlier meshes of n_int * (band + 1) */
#define GADAPT_FEM_META       8

int gadapt_fem_abi_version(void);
const char* gadapt_fem_last_error(void);
int gadapt_fem_simpson_points(void);
int gadapt_fem_lds_budget(void);

/* Host: per-batch topology, once per topology (cached by the caller).
 *   in   node_off [B+1], tri_off [B+1], cells [T,3] (global ids), boundary [N] (0/1)
 *   out  meta [B, GADAPT_FEM_META]; node_mesh [N]; tri_mesh [T]
 *        int_idx [N]  (interior index within the mesh, -1 on the boundary; interior numbering follows node numbering)
 *        int_node [N] (global node of interior slot; the first meta[.., N_INT] summed entries are used)
 *        nt_ptr [N+1], nt_idx [3T]  (node -> incident triangles, increasing triangle id; entry = 4 * tri + local vertex)
 * The band is max |int_idx[a] - int_idx[b]| over interior pairs sharing a triangle.  Returns the total band-factor
 * floats (>= 0) or a negative code. */
int64_t gadapt_fem_topology_host(int n_meshes, const int32_t* node_off, const int32_t* tri_off, const int32_t* cells,
                                 const uint8_t* boundary, int32_t* meta, int32_t* node_mesh, int32_t* tri_mesh,
                                 int32_t* int_idx, int32_t* int_node, int32_t* nt_ptr, int32_t* nt_idx);

/* LDS bytes the factor kernel needs for one mesh (band, right-hand side, update pair table). */
int64_t gadapt_fem_factor_lds_bytes(int n_int, int band);
/* LDS bytes the evaluation kernel needs for a mesh of n_tris triangles (its triangle bin mask). */
int64_t gadapt_fem_eval_lds_bytes(int n_tris);

/* Forward, three launches.
 *   x [N,2] node coordinates; meta/cells/... from gadapt_fem_topology_host (device copies)
 *   gptr [B+1], gpar [G,4] = (c0, c1, s0, s1) of each mesh's Gaussians (u_true = sum exp(-sum_d (x_d-c_d)^2/s_d^2))
 *   lat_x [nlat], lat_y [nlat]: the evaluation lattice, uniform and increasing; point (i,j) = (lat_x[i], lat_y[j]) -> i*nlat+j
 *   max_tris: largest triangle count of a mesh in the batch (sizes the evaluation kernel's LDS)
 * out rhs [N], coeffs [N], lfac [band floats] (the Cholesky factor, kept for the backward), sol [B*nlat*nlat] */
int gadapt_fem_forward(int n_meshes, int n_nodes, int n_tris, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                       const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr, const int32_t* nt_idx,
                       const int32_t* gptr, const float* gpar, const float* x, const float* lat_x, const float* lat_y, int nlat,
                       int max_lds_bytes, int max_tris, float* rhs, float* coeffs, float* lfac, float* sol, void* stream);

/* Error norms of an evaluation (the reference's evaluate_model_fine, src/utils_eval.py:46-65), forward only, four launches:
 * the load vector and banded Cholesky solve of gadapt_fem_forward, then the lattice evaluation fused with the trapezium
 * norms of e = sol - u_true (u_true from each mesh's own Gaussians), then the sum of each mesh's chunk partials:
 *   err [B,2] = (L1, L2):  L1 = sum_p w_p |e_p|,  L2 = sqrt(sum_p w_p e_p^2),
 *   w_p = h_x h_y times 1, 1/2 or 1/4 for interior, edge and corner points (every lattice cell gives dx dy / 4 to each corner).
 * sol is never written.  Arguments as gadapt_fem_forward without sol; lfac may be NULL (the factor is not kept).
 * partials: caller-owned work buffer of gadapt_fem_eval_partials_floats floats, no initialisation needed.  Every sum runs in a
 * fixed order without atomics: a mesh's pair does not depend on the rest of the batch.  Everything is checked before the first
 * launch. */
int gadapt_fem_eval_partials_floats(int n_meshes);
int gadapt_fem_eval_errors(int n_meshes, int n_nodes, int n_tris, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                           const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr, const int32_t* nt_idx,
                           const int32_t* gptr, const float* gpar, const float* x, const float* lat_x, const float* lat_y, int nlat,
                           int max_lds_bytes, int max_tris, float* rhs, float* coeffs, float* lfac, float* partials, float* err,
                           void* stream);

/* The same error norms for meshes whose band does not stay resident (fem_csrc/fem_window_kernels.hip), forward only, four
 * launches; these entry points were added without changing GADAPT_FEM_ABI (no existing signature changed).
 *   load        gadapt_fem_forward's load vector with the forcing and the two Simpson sums in fp64 (points, hat function and
 *               boundary values as there, stored in fp32): the fp32 forcing cancels and alone costs 1.2e-3 of the 64 x 64
 *               error norm (L1), beyond the evaluation's rule
 *   solve       one 256-lane workgroup per mesh; a ring of band rows in LDS (the w + 1 rows a column touches, plus as many
 *               slack rows, at most 64, as the launch's LDS leaves: rows enter the window in groups, one lane assembling each);
 *               row k of L goes to `work` once column k is eliminated, the forward substitution rides along, the back
 *               substitution reads the factor back in reverse.  The element terms are the fp32 expressions of
 *               gadapt_fem_forward's assembly; they are summed into an fp64 ring, and the factor, the stored rows and both
 *               substitutions are fp64 (an fp32 ring, bit-identical to gadapt_fem_forward's solve, was 2.6e-4 from the fp64
 *               yardstick in L1 at 27 x 27, beyond the evaluation's 2e-4 rule): coeffs differ from gadapt_fem_forward's in
 *               the last digits.
 *   evaluation  the triangles of a mesh in slabs of tri_slab ids (a multiple of 32; 0: the largest slab the budget leaves
 *               beside the chunk's running sums, 1888 triangles at nlat = 101); the bin mask is rebuilt per slab and a
 *               lattice point's sum runs on over the slabs, so in increasing triangle id as in gadapt_fem_eval_errors: err
 *               does not depend on tri_slab, bit for bit.  partials and the last launch are those of gadapt_fem_eval_errors.
 *   gadapt_fem_window_lds_bytes(n_int, band)   the ring's least LDS: pair table, max(band + 1, 2) fp64 rows (padded to an
 *               even length) and their right-hand side.  Within GADAPT_FEM_LDS_BUDGET up to band 79: square meshes up to
 *               81 x 81 nodes (64 x 64, band 62: 40 572 B).  128 x 128 (band 126, 159 KB) is refused: GADAPT_FEM_E_LDS.
 *   gadapt_fem_window_workspace_floats(B, meta)   host, from the HOST copy of meta: the floats of `work` (caller-owned, 8-byte
 *               aligned, no initialisation needed): 2 sum_b n_int[b] * (band[b] + 2), i.e. per mesh n_int fp64 rows of
 *               band + 1 and the fp64 intermediate y [n_int]; mesh b's part starts at double meta[b, BAND_OFF] + meta[b, INT_OFF].
 *               1.97 MB per 64 x 64 mesh.
 *   max_lds_bytes  the largest gadapt_fem_window_lds_bytes of the batch; the launch asks for up to the budget on top of it
 *   tri_slab < 0 or not a multiple of 32: GADAPT_FEM_E_BADARG; a slab whose mask exceeds the budget: GADAPT_FEM_E_LDS.
 * The other arguments as gadapt_fem_eval_errors.  Everything is checked before the first launch. */
int64_t gadapt_fem_window_lds_bytes(int n_int, int band);
int64_t gadapt_fem_window_workspace_floats(int n_meshes, const int32_t* meta);
int gadapt_fem_eval_errors_window(int n_meshes, int n_nodes, int n_tris, const int32_t* meta, const int32_t* cells,
                                  const int32_t* node_mesh, const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                                  const int32_t* nt_idx, const int32_t* gptr, const float* gpar, const float* x, const float* lat_x,
                                  const float* lat_y, int nlat, int max_lds_bytes, int max_tris, float* rhs, float* coeffs,
                                  float* work, int tri_slab, float* partials, float* err, void* stream);

/* Lattice-loss reductions of gadapt_fem_modular_forward. */
#define GADAPT_FEM_LOSS_MSE     0   /* mean over the nlat x nlat lattice of e^2 (F.mse_loss) */
#define GADAPT_FEM_LOSS_SIMPSON 1   /* torchquad's composite Simpson rule of e^2, y rule per x row, then x (nlat odd, >= 3) */

/* The 2-D modular loss (gradient_meshpoints_2D, difFEM_2d.py:374-535), forward, four launches: the three of
 * gadapt_fem_forward, then per mesh b the loss of e = sol - u_true on its lattice (u_true from b's own Gaussians):
 * loss [B] and g_sol [B*nlat*nlat] = d loss[b] / d sol.  One workgroup per mesh, sums in a fixed order.  The gradient
 * d loss[b] / d x is gadapt_fem_backward with g_coeffs = NULL and this g_sol.  Arguments otherwise as gadapt_fem_forward;
 * everything is checked before the first launch. */
int gadapt_fem_modular_forward(int n_meshes, int n_nodes, int n_tris, const int32_t* meta, const int32_t* cells,
                               const int32_t* node_mesh, const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                               const int32_t* nt_idx, const int32_t* gptr, const float* gpar, const float* x, const float* lat_x,
                               const float* lat_y, int nlat, int max_lds_bytes, int max_tris, int reduction, float* rhs,
                               float* coeffs, float* lfac, float* sol, float* loss, float* g_sol, void* stream);

/* Backward, four launches: d L / d x [N,2] from g_coeffs [N] and g_sol [B*nlat*nlat] (either may be NULL: zero).
 * Work buffers (caller-owned, no initialisation needed): gc [N], mu [N], tgrad [T,3,2]. */
int gadapt_fem_backward(int n_meshes, int n_nodes, int n_tris, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                        const int32_t* tri_mesh, const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                        const int32_t* nt_idx, const int32_t* gptr, const float* gpar, const float* x, const float* lat_x,
                        const float* lat_y, int nlat, int max_lds_bytes, const float* coeffs, const float* lfac,
                        const float* g_coeffs, const float* g_sol, float* gc, float* mu, float* tgrad, float* gx, void* stream);

/* The differentiable tail on the windowed route (fem_csrc/fem_window_grad_kernels.hip): forward, modular forward and backward
 * for meshes whose band does not stay resident, square meshes up to 81 x 81 nodes; these entry points were added without
 * changing GADAPT_FEM_ABI (no existing signature changed).
 *   gadapt_fem_forward_window          gadapt_fem_forward's arguments with the fp64 workspace `work` (sized by
 *               gadapt_fem_window_workspace_floats, 8-byte aligned, no initialisation needed) in lfac's place and tri_slab
 *               after it.  Three launches: the load vector and the windowed solve of gadapt_fem_eval_errors_window, then
 *               its slab walk with each lattice point's sum stored to sol (one chain of fp32 additions over the triangles
 *               in increasing id: sol does not depend on tri_slab, bit for bit).  The workspace keeps the factor for the
 *               backward.
 *   gadapt_fem_modular_forward_window  the same, then gadapt_fem_modular_forward's loss launch as it is (loss, g_sol).
 *   gadapt_fem_backward_window         gadapt_fem_backward's arguments with the workspace in lfac's place.  Four launches:
 *               gadapt_fem_backward's first, third and fourth as they are; the second solves P_II mu = gc_I on the kept
 *               workspace, one 256-lane workgroup per mesh with the solve's ring: both substitutions in fp64, mu stored in
 *               fp32, 0 on boundary nodes.  The forward substitution's intermediate overwrites the mesh's y slot in the
 *               workspace and is rewritten on every call; the factor is only read, so a second backward on one forward gives
 *               the same bits.  Each row's sum runs over its columns in increasing index whatever the ring's slack or the
 *               batch.
 *   max_lds_bytes, tri_slab as gadapt_fem_eval_errors_window; the ring's and the slab's LDS are sized by the same code.
 * Everything is checked before the first launch: null pointers, the workspace's alignment, tri_slab < 0 or not a multiple
 * of 32 (GADAPT_FEM_E_BADARG), LDS beyond the budget (GADAPT_FEM_E_LDS). */
int gadapt_fem_forward_window(int n_meshes, int n_nodes, int n_tris, const int32_t* meta, const int32_t* cells,
                              const int32_t* node_mesh, const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                              const int32_t* nt_idx, const int32_t* gptr, const float* gpar, const float* x, const float* lat_x,
                              const float* lat_y, int nlat, int max_lds_bytes, int max_tris, float* rhs, float* coeffs, float* work,
                              int tri_slab, float* sol, void* stream);
int gadapt_fem_modular_forward_window(int n_meshes, int n_nodes, int n_tris, const int32_t* meta, const int32_t* cells,
                                      const int32_t* node_mesh, const int32_t* int_idx, const int32_t* int_node,
                                      const int32_t* nt_ptr, const int32_t* nt_idx, const int32_t* gptr, const float* gpar,
                                      const float* x, const float* lat_x, const float* lat_y, int nlat, int max_lds_bytes,
                                      int max_tris, int reduction, float* rhs, float* coeffs, float* work, int tri_slab, float* sol,
                                      float* loss, float* g_sol, void* stream);
int gadapt_fem_backward_window(int n_meshes, int n_nodes, int n_tris, const int32_t* meta, const int32_t* cells,
                               const int32_t* node_mesh, const int32_t* tri_mesh, const int32_t* int_idx, const int32_t* int_node,
                               const int32_t* nt_ptr, const int32_t* nt_idx, const int32_t* gptr, const float* gpar, const float* x,
                               const float* lat_x, const float* lat_y, int nlat, int max_lds_bytes, const float* coeffs, float* work,
                               const float* g_coeffs, const float* g_sol, float* gc, float* mu, float* tgrad, float* gx, void* stream);

/* The wave-parallel adjoint (fem_csrc/fem_wave_grad_kernels.hip; fem_adjoint='wave' in Python): gadapt_fem_backward and
 * gadapt_fem_backward_window with their first and third launches - one lane per node, one lane per triangle, each walking
 * every lattice point of its bounding boxes alone - replaced by a wave per node and a wave per triangle.  Arguments, checks
 * and refusals are those of the entry point without the suffix (under this one's name); the adjoint solve and the gather
 * are the same launches.  These entry points were added without changing GADAPT_FEM_ABI (no existing signature changed).
 *
 * Ordering contract: gc, tgrad and gx are those of gadapt_fem_backward[_window], bit for bit.  The library is built without
 * FMA contraction, and each result is a chain of fp32 additions:
 *   gc[v]      starts at g_coeffs[v] (0 without); v's incident (triangle, corner) pairs in CSR order; within one, the lattice
 *              points of the triangle's bounding box, i outer, j inner; a point adds g_sol[p] * (inc / div), and a point
 *              with ind == 0 or inc == 0 adds nothing (it is skipped, not added as zero).
 *   tgrad[t]   six chains, (x, y) of the three vertices.  Each: the stiffness terms as one lane computes them; then per
 *              interior corner l = 0, 1, 2 ONE addend, the sum from zero over the 9 x 9 Simpson points in (i, j) order
 *              (ind == 0 skipped) of the aux_grad term that corner's rotation gives this vertex; then per lattice point of
 *              the bounding box in (i, j) order (ind == 0 skipped) the terms of l = 0, 1, 2.
 * The wave computes 64 addends at a time with the lane kernels' expressions, leaves them in LDS in point order, and one
 * lane per chain adds the points the round's ballot marks, in increasing order.  A workgroup is one wave (static LDS 256 B
 * and 4 680 B), so a box of any size is walked in rounds with the chains carried in registers.  No atomics, no scratch. */
int gadapt_fem_backward_wave(int n_meshes, int n_nodes, int n_tris, const int32_t* meta, const int32_t* cells,
                             const int32_t* node_mesh, const int32_t* tri_mesh, const int32_t* int_idx, const int32_t* int_node,
                             const int32_t* nt_ptr, const int32_t* nt_idx, const int32_t* gptr, const float* gpar, const float* x,
                             const float* lat_x, const float* lat_y, int nlat, int max_lds_bytes, const float* coeffs,
                             const float* lfac, const float* g_coeffs, const float* g_sol, float* gc, float* mu, float* tgrad,
                             float* gx, void* stream);
int gadapt_fem_backward_window_wave(int n_meshes, int n_nodes, int n_tris, const int32_t* meta, const int32_t* cells,
                                    const int32_t* node_mesh, const int32_t* tri_mesh, const int32_t* int_idx,
                                    const int32_t* int_node, const int32_t* nt_ptr, const int32_t* nt_idx, const int32_t* gptr,
                                    const float* gpar, const float* x, const float* lat_x, const float* lat_y, int nlat,
                                    int max_lds_bytes, const float* coeffs, float* work, const float* g_coeffs,
                                    const float* g_sol, float* gc, float* mu, float* tgrad, float* gx, void* stream);

/* The wave-parallel forward of the resident-band route (fem_csrc/fem_wave_fwd_kernels.hip; fem_forward='wave' in Python):
 * gadapt_fem_forward and gadapt_fem_modular_forward with their first and third launches replaced.  Arguments, checks, their
 * order and the refusals are those of the entry point without the suffix, before any launch (under this one's name where that
 * one reports under its own; gadapt_fem_modular_forward reports the shared checks under gadapt_fem_forward's name, and so does
 * gadapt_fem_modular_forward_wave); the factor launch and the loss launch are the same launches.  There is no windowed form.
 * These entry points were added without changing GADAPT_FEM_ABI (no existing signature changed).
 *
 * Ordering contract: rhs, coeffs, lfac, sol, loss and g_sol are those of the entry point without the suffix, bit for bit, for
 * every input it accepts.  The library is built without FMA contraction, and each result is a chain of fp32 operations in a
 * fixed order on addends that do not depend on each other:
 *   rhs[m]     on an interior node the 9 x 9 integrand values f(i, j) = out / div * forcing, each from its own point alone; nine
 *              y-rule sums s_i, each from zero over k = 0, 2, 4, 6 of hy3 * (f(i,k) + 4 f(i,k+1) + f(i,k+2)); the x-rule sum of
 *              the s_i in the same form.  A wave per node computes the 81 values on its lanes (64 + 17) into LDS, nine lanes
 *              form the s_i, one lane the result (372 B of static LDS).  A boundary node is u_true on one lane.
 *   sol[p]     from zero, over the triangles of p's bin in increasing id that contain p, over their corners l = 0, 1, 2 with
 *              inc != 0: coeffs[v] * (inc / div).  A lane scans the bin with the containment test alone and notes the
 *              containing triangles in four registers, then adds their terms in the noted order; a lane that meets a fifth
 *              adds the four first and goes on, so any number of overlapping triangles gives the same chain.  The lanes of a
 *              wave so run the expensive terms together.  A workgroup is one wave, and the lattice of a mesh is cut into
 *              min(ceil(nlat^2 / 64), max(2048 / n_meshes, 1)) chunks (sol[p] does not depend on the cut): one point per lane
 *              for a small batch.  The LDS is the bin mask of gadapt_fem_eval_lds_bytes, as for gadapt_fem_forward.
 * No float atomics, no scratch; a mesh's result does not depend on its batch. */
int gadapt_fem_forward_wave(int n_meshes, int n_nodes, int n_tris, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                            const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr, const int32_t* nt_idx,
                            const int32_t* gptr, const float* gpar, const float* x, const float* lat_x, const float* lat_y, int nlat,
                            int max_lds_bytes, int max_tris, float* rhs, float* coeffs, float* lfac, float* sol, void* stream);
int gadapt_fem_modular_forward_wave(int n_meshes, int n_nodes, int n_tris, const int32_t* meta, const int32_t* cells,
                                    const int32_t* node_mesh, const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                                    const int32_t* nt_idx, const int32_t* gptr, const float* gpar, const float* x, const float* lat_x,
                                    const float* lat_y, int nlat, int max_lds_bytes, int max_tris, int reduction, float* rhs,
                                    float* coeffs, float* lfac, float* sol, float* loss, float* g_sol, void* stream);

/* gadapt_fem_eval_errors on the wave-parallel kernels (fem_forward='wave' in the Python evaluation), resident band only, five
 * launches: the wave load vector, the factor launch as it is, the wave evaluation into sol_work, then fem_eval_err_kernel's
 * reduction reading sol_work (fem_err_lattice_kernel: the same cut of the lattice into chunks and lanes, the same statements,
 * the same butterfly and wave order), then the sum of the chunk partials as it is.
 *   sol_work [B * nlat * nlat]  caller-owned work buffer, no initialisation needed.  On this route sol DOES reach memory (40 KB a
 *                               mesh at nlat 101); gadapt_fem_eval_errors still never writes it.
 * The other arguments, the checks, their order and the refusals are gadapt_fem_eval_errors's, under this entry point's name;
 * a NULL sol_work is refused where a NULL partials or err is (after the LDS checks).  sol_work holds gadapt_fem_forward's sol
 * bit for bit, so rhs, coeffs, partials and err are gadapt_fem_eval_errors's, bit for bit, in any batch.  No float atomics.
 * Added without changing GADAPT_FEM_ABI (no existing signature changed). */
int gadapt_fem_eval_errors_wave(int n_meshes, int n_nodes, int n_tris, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                                const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr, const int32_t* nt_idx,
                                const int32_t* gptr, const float* gpar, const float* x, const float* lat_x, const float* lat_y, int nlat,
                                int max_lds_bytes, int max_tris, float* rhs, float* coeffs, float* lfac, float* sol_work, float* partials,
                                float* err, void* stream);

/* ------------------------------------------------------------------------------------------------ 1-D tails
 * Differentiable 1-D P1 FEM of the reference's modular loss (firedrake_difFEM/difFEM_1d.py): semi-implicit Burgers steps
 * (torch_FEM_Burgers_1D, get_Burgers_initial_coeffs) and Poisson (torch_FEM_1D), with the reference's trapezoid inner
 * products, literal hat functions (inclusive interval test, -1 at the node) and searchsorted point location.
 *
 * Meshes b = 0..B-1 are concatenated: nodes [node_off[b], node_off[b+1]), coordinates x [N].  Gaussians of mesh b are
 * gpar[gptr[b]..gptr[b+1]) as (centre, scale) pairs.  Evaluation points `pts` [P] are shared by all meshes; sol is [B,P].
 * One workgroup per mesh, the mesh's whole state in LDS, one launch forward and one backward.  The tridiagonal solves run
 * on one lane (Thomas, no pivoting: the Burgers matrix is strictly and the Poisson matrix weakly diagonally dominant;
 * the Poisson stiffness trapezoids and elimination in fp64: the system's condition grows as N^2).
 * No float atomics: results are bit-reproducible.
 *
 * Node cap.  A workgroup has one lane per node (GADAPT_FEM1D_MAX_NODES = 1024, the largest workgroup).  The Burgers
 * backward keeps 15 floats per node in LDS and the Poisson launches 64 bytes per node (their solve runs in fp64), 64 KB at
 * 1024 nodes, within GADAPT_FEM_LDS_BUDGET; gadapt_fem1d_lds_bytes gives the need.
 *
 * Non-monotone meshes.  Where a mesh folds, the reference's mass and stiffness matrices stop being tridiagonal; the
 * tridiagonal part is assembled and flags[b] gets bit GADAPT_FEM1D_F_NOT_INCREASING (some x[i+1] - x[i] < 0).  Point
 * location follows torch's CPU lower-bound search, so it matches the reference there too.
 *
 * Clamping.  fn_expansion's slope at index N-1 is 0 (as in the reference); dxfn_expansion clamps its index to N-2 (the
 * reference would index past its slope list), and soln (Poisson) uses the same evaluation as fn_expansion. */

#define GADAPT_FEM1D_MAX_NODES 1024
#define GADAPT_FEM1D_F_NOT_INCREASING 1

/* LDS bytes of the 1-D launches for meshes of up to max_nodes nodes and an n_fine-node fine mesh (0: none). */
int64_t gadapt_fem1d_lds_bytes(int max_nodes, int n_fine);

/* Burgers forward, one launch.
 *   u0 [N]: initial coefficients, or NULL to project amp * sum_g exp(-(x-c_g)^2/s_g^2) (mass with k_proj points, load with
 *           k_load, identity boundary rows with u0(0) and u0(1)); bc [B,2]: RHS boundary values, or NULL for u^n's end values
 *   n_fine > 1 also runs the same steps on linspace(0, 1, n_fine) (its projection's mass uses k_proj_fine points) -> fine_sol
 *   taunu = float(tau * nu) as the reference forms it; k_stiff: points of the stiffness trapezoid minus one
 * out hist [(T+1) N]: mesh b's u^0..u^T at hist[(T+1) node_off[b] + t n_b + i]; sol [B,P] = fn_expansion(u^T, x, pts);
 *     fine_sol [B,P] (if n_fine > 1); flags [B] */
int gadapt_fem1d_burgers_forward(int n_meshes, int max_nodes, const int32_t* node_off, const float* x, const float* u0,
                                 const float* bc, const int32_t* gptr, const float* gpar, float amp, float tau, float taunu,
                                 int k_load, int k_stiff, int k_proj, int k_proj_fine, int n_steps, int n_fine, int n_pts,
                                 const float* pts, float* hist, float* sol, float* fine_sol, int32_t* flags, void* stream);

/* Burgers backward, one launch: gx [N] = d L / d x and, if gu0 != NULL, gu0 [N] = d L / d u^0, from g_sol [B,P] and
 * g_last [N] (d L / d u^T); either may be NULL (zero).  bc as in the forward (explicit boundary values get no gradient). */
int gadapt_fem1d_burgers_backward(int n_meshes, int max_nodes, const int32_t* node_off, const float* x, const float* bc,
                                  float tau, float taunu, int k_load, int k_stiff, int n_steps, int n_pts, const float* pts,
                                  const float* hist, const float* g_sol, const float* g_last, float* gx, float* gu0,
                                  void* stream);

/* Poisson forward (torch_FEM_1D), one launch: coeffs [N] = (BC1, interior solution, BC2) per mesh, BC = u_true at the
 * end nodes (detached); sol [B,P]; flags [B]. */
int gadapt_fem1d_poisson_forward(int n_meshes, int max_nodes, const int32_t* node_off, const float* x, const int32_t* gptr,
                                 const float* gpar, int k_load, int k_stiff, int n_pts, const float* pts, float* coeffs,
                                 float* sol, int32_t* flags, void* stream);

/* Poisson forward with the reference's 1-D trapezium norms (evaluate_error_np, src/utils_eval.py:32-44) of e = sol - u_true over
 * pts [P >= 2] reduced in the same launch: err [B,2] = (L1, L2), L1 = sum_j (|e_j| + |e_j+1|) (pts_j+1 - pts_j) / 2 and L2 the
 * square root of the same sum over e^2; flags [B] as the forward sets them.  Neither coeffs nor sol is written.  The solve is the
 * forward's (stiffness in fp64: in fp32 its rounded row sums move the norms by up to 3e-4; load, boundary values, expansion in fp32). */
int gadapt_fem1d_poisson_eval_errors(int n_meshes, int max_nodes, const int32_t* node_off, const float* x, const int32_t* gptr,
                                     const float* gpar, int k_load, int k_stiff, int n_pts, const float* pts, float* err,
                                     int32_t* flags, void* stream);

/* Poisson backward, one launch: gx [N] from g_coeffs [N] and g_sol [B,P] (either may be NULL). */
int gadapt_fem1d_poisson_backward(int n_meshes, int max_nodes, const int32_t* node_off, const float* x, const int32_t* gptr,
                                  const float* gpar, int k_load, int k_stiff, int n_pts, const float* pts,
                                  const float* coeffs, const float* g_coeffs, const float* g_sol, float* gx, void* stream);

/* The 1-D pde_loss tail in one launch: the Poisson forward, the loss of sol against a target on the evaluation points, and the
 * gradient of that loss in the nodes (what gadapt_fem1d_poisson_forward, the loss launch of gadapt_hip.h and
 * gadapt_fem1d_poisson_backward give in three).  One workgroup per mesh b, sized as for the other Poisson launches; with
 * P = n_pts and inv = 1.0f / (float)(B * P), operation for operation:
 *   1. the solve of gadapt_fem1d_poisson_forward; coeffs [N] and flags [B] as it writes them
 *   2. sol[b,p] = fn_expansion(coeffs_b, x_b, pts[p]), the bits of gadapt_fem1d_poisson_forward; diff = sol[b,p] - target[b * P + p]
 *   3. partials[b] = sum_p |diff| (GADAPT_FEM1D_LOSS_L1) or sum_p diff * diff (GADAPT_FEM1D_LOSS_MSE), by the first wave: lane l
 *      adds points l, l + 64, ... in that order and the 64 lanes are added in a fixed butterfly, so the order follows P alone
 *   4. the seed d loss / d sol[b,p], kept in LDS:  L1: diff > 0 ? inv : diff < 0 ? -inv : 0;  MSE: 2.0f * diff * inv
 *      (the expressions of gadapt_loss_forward on [B * P, 1])
 *   5. gx [N]: gadapt_fem1d_poisson_backward with g_coeffs = NULL and g_sol = that seed, the same bits
 *   6. loss [1] = (partials[0] + partials[1] + ... + partials[B-1]) * inv, added in index order by the workgroup that
 *      finishes last; ticket [1] counts the finished workgroups and is left at 0 (it must be 0 on entry: zero it once)
 * Neither sums nor the gradient use float atomics: two calls give the same bits.  partials[b], like coeffs, sol and flags of mesh b,
 * does not depend on the rest of the batch; gx and loss do through inv alone.
 * LDS: the Poisson launches' 64 bytes per node and a seed row of 4 * n_pts bytes, gadapt_fem_poisson1d_loss_lds_bytes; within
 * GADAPT_FEM_LDS_BUDGET that is 1017 nodes at 101 points, not GADAPT_FEM1D_MAX_NODES, and GADAPT_FEM_E_LDS beyond, before any
 * launch.  (Named gadapt_fem_poisson1d_*, not gadapt_fem1d_*: that prefix is the eight entry points above with their shared
 * node cap, whose refusal table tests/test_fem1d_abi_host.py pins as complete.) */
#define GADAPT_FEM1D_LOSS_L1  0
#define GADAPT_FEM1D_LOSS_MSE 1
int64_t gadapt_fem_poisson1d_loss_lds_bytes(int max_nodes, int n_pts);
int gadapt_fem_poisson1d_loss(int n_meshes, int max_nodes, const int32_t* node_off, const float* x, const int32_t* gptr,
                              const float* gpar, int k_load, int k_stiff, int n_pts, const float* pts, const float* target,
                              int loss_kind, float* coeffs, float* sol, float* gx, int32_t* flags, float* partials, float* loss,
                              int32_t* ticket, void* stream);

/* fn_expansion(c, x, pts) per mesh (no gradient): sol [B,P]. */
int gadapt_fem1d_expand(int n_meshes, int max_nodes, const int32_t* node_off, const float* x, const float* c, int n_pts,
                        const float* pts, float* sol, void* stream);

/* Batched not-a-knot interpolating cubic splines (fem_csrc/spline_kernels.hip), one launch: scipy's
 * UnivariateSpline(x, y, s=0) / CubicSpline(bc_type='not-a-knot') of the Burgers rollout (src/utils_eval_Burgers.py:215-239),
 * the C2 piecewise cubic through all points whose third derivative is continuous at x[1] and x[n-2]; n = 4 is the cubic
 * through four points.
 *   sets b = 0..B-1 concatenated: points [set_off[b], set_off[b+1]) of x (strictly increasing) and y, 4 <= n_b <= max_nodes
 *   queries: q_off == NULL: q [Q] shared by all sets, out [B,Q];  else q [q_off[B]] per set, out laid out like q
 *   deriv 0, 1, 2: the value, first or second derivative; queries outside [x[0], x[n-1]] use the end pieces
 * One workgroup per set; x, y and the second derivatives in LDS as fp64 (32 bytes per point), elimination (one lane's Thomas
 * sweep) and evaluation in fp64, fp32 in and out.  status [B]: GADAPT_SPLINE_S_*; a flagged set writes NaN to its own
 * outputs and touches nothing else.  A set's output does not depend on the rest of the batch. */
#define GADAPT_SPLINE_S_OK             0
#define GADAPT_SPLINE_S_NOT_INCREASING 1   /* some x[i+1] <= x[i] */
#define GADAPT_SPLINE_S_NOT_FINITE     2   /* a NaN or infinity in x or y */
#define GADAPT_SPLINE_S_BAD_COUNT      3   /* n_b outside 4..max_nodes */
int gadapt_fem1d_spline(int n_sets, int max_nodes, const int32_t* set_off, const float* x, const float* y, int n_queries,
                        const float* q, const int32_t* q_off, int deriv, float* out, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------ mesh descent
 * The reference's backFEM baselines (train_step_adjoint, difFEM_2d.py:593-685; train_step_vec, difFEM_1d.py:241-292): gradient
 * descent of the node coordinates themselves on the FEM error, plain SGD, no network (fem_csrc/descent_kernels.hip).  One call
 * enqueues every epoch on the caller's stream: it neither synchronises nor allocates, and the host waits for nothing.  These
 * entry points were added without changing GADAPT_FEM_ABI (no existing signature changed).
 *
 * 2-D.  Arguments as gadapt_fem_modular_forward and gadapt_fem_backward (all their outputs and work buffers are the caller's,
 * with their sizes), and
 *   x [N,2]            in: the starting coordinates; out: the coordinates after `epochs` steps
 *   x_ref [N,2]        the mesh whose triangle orientations count as untangled; NULL: the starting coordinates
 *   epochs, lr         epoch j: the four launches of gadapt_fem_modular_forward (reduction GADAPT_FEM_LOSS_SIMPSON), the four of
 *                      gadapt_fem_backward (g_coeffs = NULL), then one step launch, a workgroup per mesh: x -= lr * gx on
 *                      interior nodes (the product rounded before the subtraction, as torch.optim.SGD); boundary nodes are not
 *                      touched.  epochs == 0 launches only the orientation pass.
 *   loss_hist [E,B]    loss of epoch j, i.e. on the mesh before that epoch's step (may be NULL when epochs == 0)
 *   mesh_hist [E,N,2]  coordinates after each step, or NULL
 *   first_tangled [B]  the first epoch after whose step min_t D_t(x) sign(D_t(x_ref)) <= 0 or NaN, D twice the signed triangle
 *                      area as the stiffness computes it; -1 if none.  The descent goes on regardless (as the reference, whose
 *                      FEM uses |D|).
 *   min_area [B]       that minimum after the latest step, kept from the first tangled epoch on; +inf before any step
 *   sign [T]           int8 scratch: the orientations on x_ref, written by a launch before epoch 0
 * coeffs, sol, loss, gx, ... are left as the last epoch's launches wrote them: coeffs is the solve on the mesh BEFORE the last
 * step (the reference returns that one too). */
int gadapt_fem_descend(int n_meshes, int n_nodes, int n_tris, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                       const int32_t* tri_mesh, const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                       const int32_t* nt_idx, const int32_t* gptr, const float* gpar, float* x, const float* x_ref, const float* lat_x,
                       const float* lat_y, int nlat, int max_lds_bytes, int max_tris, int epochs, float lr, float* rhs, float* coeffs,
                       float* lfac, float* sol, float* loss, float* g_sol, float* gc, float* mu, float* tgrad, float* gx,
                       float* loss_hist, float* mesh_hist, int32_t* first_tangled, float* min_area, int8_t* sign, void* stream);

/* gadapt_fem_descend with the wave-parallel kernels in its epochs.  routes: bit 0 (GADAPT_FEM_ROUTE_WAVE_FORWARD) runs an
 * epoch's forward as gadapt_fem_modular_forward_wave does, bit 1 (GADAPT_FEM_ROUTE_WAVE_ADJOINT) its backward as
 * gadapt_fem_backward_wave does; any other bit is GADAPT_FEM_E_BADARG, refused first.  routes == 0 is gadapt_fem_descend.  The
 * other arguments and the refusals are gadapt_fem_descend's, in its order, under this entry point's name where that one's
 * appears.  Every output has gadapt_fem_descend's bits for every value of routes.  Added without changing GADAPT_FEM_ABI. */
#define GADAPT_FEM_ROUTE_WAVE_FORWARD 1
#define GADAPT_FEM_ROUTE_WAVE_ADJOINT 2
int gadapt_fem_descend_wave(int n_meshes, int n_nodes, int n_tris, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                            const int32_t* tri_mesh, const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                            const int32_t* nt_idx, const int32_t* gptr, const float* gpar, float* x, const float* x_ref,
                            const float* lat_x, const float* lat_y, int nlat, int max_lds_bytes, int max_tris, int epochs, float lr,
                            float* rhs, float* coeffs, float* lfac, float* sol, float* loss, float* g_sol, float* gc, float* mu,
                            float* tgrad, float* gx, float* loss_hist, float* mesh_hist, int32_t* first_tangled, float* min_area,
                            int8_t* sign, int routes, void* stream);

/* 1-D.  Epoch j: gadapt_fem1d_poisson_forward, the seed launch (loss [B] = torch.trapezoid((sol - u_true)^2, pts), the loss of
 * gradient_meshpoints_1D's PDE_loss_direct_L2, and g_sol [B,P] = d loss / d sol), gadapt_fem1d_poisson_backward, the step.
 *   mesh_params  INTERNAL: nodes 1..n-2 move.  ALL: every node moves, then the mesh is rescaled to (x - min) / (max - min) and
 *                its ends are set to 0 and 1 (difFEM_1d.py:273-279; it is not sorted).
 *   n_nodes      N, the node total (the row length of mesh_hist [E,N])
 *   first_tangled / min_area watch min_i x[i+1] - x[i]; P >= 2; the rest as in 2-D and in the Poisson entry points. */
#define GADAPT_FEM1D_DESCEND_INTERNAL 0
#define GADAPT_FEM1D_DESCEND_ALL      1
int gadapt_fem1d_descend(int n_meshes, int max_nodes, const int32_t* node_off, float* x, const int32_t* gptr, const float* gpar,
                         int k_load, int k_stiff, int n_pts, const float* pts, int epochs, float lr, int mesh_params, int n_nodes,
                         float* coeffs, float* sol, int32_t* flags, float* loss, float* g_sol, float* gx, float* loss_hist,
                         float* mesh_hist, int32_t* first_tangled, float* min_area, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GADAPT_FEM_H */
