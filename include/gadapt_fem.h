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
 */
#ifndef GADAPT_FEM_H
#define GADAPT_FEM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GADAPT_FEM_ABI 1

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

/* Backward, four launches: d L / d x [N,2] from g_coeffs [N] and g_sol [B*nlat*nlat] (either may be NULL: zero).
 * Work buffers (caller-owned, no initialisation needed): gc [N], mu [N], tgrad [T,3,2]. */
int gadapt_fem_backward(int n_meshes, int n_nodes, int n_tris, const int32_t* meta, const int32_t* cells, const int32_t* node_mesh,
                        const int32_t* tri_mesh, const int32_t* int_idx, const int32_t* int_node, const int32_t* nt_ptr,
                        const int32_t* nt_idx, const int32_t* gptr, const float* gpar, const float* x, const float* lat_x,
                        const float* lat_y, int nlat, int max_lds_bytes, const float* coeffs, const float* lfac,
                        const float* g_coeffs, const float* g_sol, float* gc, float* mu, float* tgrad, float* gx, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GADAPT_FEM_H */
