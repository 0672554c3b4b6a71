"""Differentiable P1 FEM tail of loss_type='pde_loss' (2-D Poisson), MI355X-native.

The reference solves the Poisson problem of each sample on the moved mesh with a differentiable P1 FEM
(`firedrake_difFEM/difFEM_2d.py:320-372`, called from `src/GNN.py:307-342`) and trains on the error of that solve.  Here a
whole batch is one autograd node over `libgadapt_fem.so` (include/gadapt_fem.h): three launches forward (load vector, banded
Cholesky solve with the band in LDS, lattice evaluation), four backward (evaluation adjoint, adjoint solve on the kept factor,
per-triangle chain rule, per-node gather).

    torch_FEM_2D(opt, mesh, mesh_points, quad_points, num_meshpoints, c_list, s_list) -> (coeffs [N,1], mesh_points, sol)
    fem_poisson(x_phys, cells, boundary, node_counts, pde_params, lattice) -> (coeffs [N,1], sol [B*Q])
    gradient_meshpoints_2D(opt, data, x_phys) -> (loss, x_grads [N,2])     # loss_type='modular' (difFEM_2d.py:374-535)
    modular_loss_2d(x_phys, cells, boundary, node_counts, pde_params, n_lat, reduction) -> (loss [B], x_grads [N,2])

Limits: 2-D Poisson only; each mesh's banded factor must fit the LDS budget (`gadapt_fem_lds_budget()`, 64 KB: square
meshes up to 26 x 26 nodes); the evaluation points must be a uniform tensor-product lattice.

band='window' (`fem_poisson`, `modular_loss_2d`; opt['fem_band'] = 'window' for `torch_FEM_2D`, `gnn_pde_tail` and
`gradient_meshpoints_2D`) takes square meshes up to 81 x 81 nodes: the solve keeps a ring of band rows in LDS and streams the
fp64 factor through a global workspace, which the autograd node keeps for its adjoint solve in lfac's place
(gadapt_fem_forward_window, gadapt_fem_modular_forward_window, gadapt_fem_backward_window).  The default stays 'lds'.

What bounds a route is the half-bandwidth of the interior block in the node numbering the mesh is given in, not its side
length: `gadapt_fem_factor_lds_bytes(n_int, band)` ('lds') or `gadapt_fem_window_lds_bytes(n_int, band)` ('window') against
the 64 KB budget.  The sides quoted here are those of `square_mesh`'s row-major numbering (band n - 2).  A band of 79 is the
windowed maximum for any mesh; a reference-style numbering (`mesh.coordinates.cell_node_map()`) with a wider band than
row-major may be refused at a smaller size.  The nodes are not reordered here.

adjoint='wave' (`fem_poisson`, `modular_loss_2d`, `PdeBatch`; opt['fem_adjoint'] = 'wave' for `gnn_pde_tail` and
`gradient_meshpoints_2D`) runs the backward's two lattice walks with a wave per node and a wave per triangle instead of a lane
each (gadapt_fem_backward_wave, gadapt_fem_backward_window_wave): the same gradient, bit for bit.  The default stays 'lane'.

forward='wave' (the same functions; opt['fem_forward'] = 'wave' for `torch_FEM_2D`, `gnn_pde_tail`, `gradient_meshpoints_2D` and
`PdeBatch.from_data`) runs the load vector with a wave per node and the evaluation with a wave per chunk of the lattice and two
phases per point (gadapt_fem_forward_wave, gadapt_fem_modular_forward_wave): the same rhs, coeffs, factor and sol, bit for bit.
band='lds' only: with band='window' it is a ValueError.  The default stays 'lane'.  The same two keys reach the evaluation
(`evaluation.poisson_eval_errors(forward='wave')`, gadapt_fem_eval_errors_wave) and the mesh descent
(`descent.mesh_descent_2d(forward=..., adjoint=...)`, gadapt_fem_descend_wave), with the lane routes' bits.

`PdeBatch` is the tail of one batch topology with everything a call would rebuild kept on the device - the topology, the lattice
axes, the Gaussians' buffers: `gnn_pde_tail` on a batch that carries one (`data._pde_batch`) only launches, so it can be
captured in a hipGraph, and `set_params` feeds the Gaussians of the next batch into the same buffers
(`training.GraphedTrainStep` does both for a pde_loss model).

The argument contract (`_check_batch_2d` and `_check_cells`, called by every public entry point before anything is allocated,
before the device is looked at and before the library is loaded; tests/test_entry_contracts_host.py pins it row by row):

    lengths   x_phys is [N,2] with N == sum(node_counts), which is the topology's n_nodes; node_counts is not empty and every
              mesh has at least 3 nodes (one triangle); len(pde_params) == len(node_counts), and every Gaussian centre and
              scale has two components; cells is [T,3] of an integer dtype (a [3,T] or 1-D array is refused, never reshaped),
              T == sum(tri_counts) where those are given; boundary holds N flags
    dtypes    coordinates are fp32 or TypeError - nothing is cast (`gradient_meshpoints_2D` alone, which is handed the training
              loop's detached x_phys, takes any floating dtype and gives `modular_loss_2d` its fp32 cast; integer and complex
              tensors are a TypeError there too); cells may be any integer dtype, boundary bool or any integer dtype
    layouts   any strides and storage offset: what reaches a kernel is a contiguous tensor, and x_phys.grad has x_phys's shape
    errors    ValueError for lengths, TypeError for dtypes, with the function's name and the two numbers that disagree
              (an x_phys that is not [N,2] stays a NotImplementedError); a well-formed call on CPU tensors is a NativeError
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native_fem as _nf
from ._native import NativeError, current_stream
from .graph import content_fingerprint

__all__ = ['FemTopology', 'PdeBatch', 'fem_poisson', 'torch_FEM_2D', 'boundary_from_cells', 'gnn_pde_tail', 'gradient_meshpoints_2D',
           'modular_loss_2d', 'simpson_points_per_dim', 'GRAD_TYPES_2D']


BAND_ROUTES = ('lds', 'window')
ADJOINTS = ('lane', 'wave')
FORWARDS = ('lane', 'wave')
# appended to the refusals of the resident-band route
WINDOW_HINT = ("; the evaluation (poisson_eval_errors, evaluate_model_fine) takes larger meshes with band='window' "
               "(opt['fem_band'] = 'window')")


def _require_gpu(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise NativeError(f"{what}: the FEM tail runs on the MI355X only (got a {t.device} tensor); there is no CPU fallback")
    _check_fp32(what, t)


def _check_fp32(what: str, t):
    """The 2-D dtype rule, the one place it is enforced: fp32 coordinates or TypeError."""
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: the coordinates must be a tensor (got {type(t).__name__})")
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: fp32 expected, got {t.dtype}")


def _check_cells(what: str, cells, boundary, n_nodes: int, tri_counts: Optional[Sequence[int]] = None):
    """cells [T,3] integer and boundary [N] (tensors or numpy arrays), on the host alone."""
    shape = tuple(cells.shape)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{what}: cells must be [T,3] (got {shape}); a [3,T] or flat array is not reshaped")
    kind = cells.dtype.kind if isinstance(cells, np.ndarray) else ('f' if cells.dtype.is_floating_point or cells.dtype.is_complex
                                                                   or cells.dtype == torch.bool else 'i')
    if kind not in 'iu':
        raise TypeError(f"{what}: cells must hold integer node ids (got {cells.dtype})")
    if tri_counts is not None and shape[0] != int(sum(int(t) for t in tri_counts)):
        raise ValueError(f"{what}: {shape[0]} cells for tri_counts summing to {int(sum(int(t) for t in tri_counts))}")
    if boundary is not None:
        bshape = tuple(boundary.shape)
        if len(bshape) != 1 or bshape[0] != n_nodes:
            raise ValueError(f"{what}: {bshape} boundary flags for {n_nodes} nodes")


def _check_gaussians(what: str, pde_params: Sequence[dict], n_meshes: int):
    if len(pde_params) != n_meshes:
        raise ValueError(f"{what}: Gaussians of {len(pde_params)} meshes for node_counts of {n_meshes} meshes")
    for b, p in enumerate(pde_params):
        if len(p['centers']) != len(p['scales']):
            raise ValueError(f"{what}: mesh {b} has {len(p['centers'])} centres and {len(p['scales'])} scales")
        for name in ('centers', 'scales'):
            for v in p[name]:
                k = int(v.numel() if torch.is_tensor(v) else np.asarray(v).size)
                if k != 2:
                    raise ValueError(f"{what}: a Gaussian's {name[:-1]} of mesh {b} has {k} components; 2 in 2-D")


def _check_batch_2d(what: str, x_phys, node_counts: Sequence[int], pde_params: Optional[Sequence[dict]] = None, cells=None,
                    boundary=None, tri_counts: Optional[Sequence[int]] = None, cast: bool = False) -> list:
    """The 2-D argument contract (module docstring), on the host alone: nothing is allocated, no device or library is touched.
    `cast`: the caller casts a floating x_phys to fp32 (gradient_meshpoints_2D).  Returns the node counts as ints."""
    if cast:
        if not torch.is_tensor(x_phys) or not x_phys.dtype.is_floating_point:
            raise TypeError(f"{what}: x_phys must be a floating-point tensor (got "
                            f"{x_phys.dtype if torch.is_tensor(x_phys) else type(x_phys).__name__})")
    else:
        _check_fp32(what, x_phys)
    if x_phys.dim() != 2 or x_phys.shape[1] != 2:
        raise NotImplementedError(f"{what}: x_phys must be [N,2], 2-D meshes only (got {tuple(x_phys.shape)})")
    counts = [int(n) for n in node_counts]
    if not counts:
        raise ValueError(f"{what}: node_counts is empty (0 meshes for {x_phys.shape[0]} coordinates)")
    if min(counts) < 3:
        raise ValueError(f"{what}: every mesh needs at least 3 nodes (got {min(counts)})")
    if x_phys.shape[0] != sum(counts):
        raise ValueError(f"{what}: {x_phys.shape[0]} coordinates for {sum(counts)} nodes (the sum of node_counts)")
    if pde_params is not None:
        _check_gaussians(what, pde_params, len(counts))
    if cells is not None:
        _check_cells(what, cells, boundary, sum(counts), tri_counts)
    return counts


def boundary_from_cells(cells: np.ndarray, n_nodes: int) -> np.ndarray:
    """Nodes on an edge that belongs to one triangle only (Firedrake's DirichletBC(V, 0, 'on_boundary').nodes)."""
    cells = np.asarray(cells, dtype=np.int64)
    e = np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [2, 0]]], 0)
    e.sort(1)
    uniq, cnt = np.unique(e, axis=0, return_counts=True)
    out = np.zeros(n_nodes, dtype=bool)
    out[uniq[cnt == 1].reshape(-1)] = True
    return out


class FemTopology:
    """Interior numbering, band and node -> triangle CSR of a batch (gadapt_fem_topology_host), on the device."""

    def __init__(self, cells: np.ndarray, boundary: np.ndarray, node_counts: Sequence[int], tri_counts: Sequence[int], device,
                 band: str = 'lds'):
        """band='lds': each mesh's banded factor and the evaluation's bin mask must fit the LDS budget (every FEM tail).
        band='window': the ring of the windowed solve must (`poisson_eval_errors`, `fem_poisson` and `modular_loss_2d` with
        band='window': square meshes up to 81 x 81 nodes); `lds_bytes` is then the ring's."""
        if band not in BAND_ROUTES:
            raise ValueError(f"FEM topology: band must be one of {BAND_ROUTES} (got {band!r})")
        B = len(node_counts)
        if B < 1 or len(tri_counts) != B:
            raise ValueError(f"FEM topology: node_counts of {B} meshes and tri_counts of {len(tri_counts)}")
        cells, boundary = np.asarray(cells), np.asarray(boundary)
        _check_cells('FEM topology', cells, None, int(np.sum(node_counts)))
        if boundary.ndim != 1:
            raise ValueError(f"FEM topology: boundary must be [N] (got {boundary.shape})")
        lib = _nf.lib()
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        bnd = np.ascontiguousarray(boundary, dtype=np.uint8)
        node_off = np.zeros(B + 1, np.int32); node_off[1:] = np.cumsum(node_counts)
        tri_off = np.zeros(B + 1, np.int32); tri_off[1:] = np.cumsum(tri_counts)
        N, T = int(node_off[-1]), int(tri_off[-1])
        if cells.shape[0] != T or bnd.shape[0] != N:
            raise ValueError(f"FEM topology: {cells.shape[0]} cells / {bnd.shape[0]} boundary flags for {T} triangles / {N} nodes")
        meta = np.zeros((B, _nf.META), np.int32)
        node_mesh, int_idx, int_node, nt_ptr = (np.zeros(N, np.int32) for _ in range(4))
        nt_ptr = np.zeros(N + 1, np.int32)
        tri_mesh, nt_idx = np.zeros(T, np.int32), np.zeros(3 * T, np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = lib.gadapt_fem_topology_host(B, p(node_off), p(tri_off), p(cells), p(bnd), p(meta), p(node_mesh), p(tri_mesh),
                                          p(int_idx), p(int_node), p(nt_ptr), p(nt_idx))
        _nf.check(rc, 'gadapt_fem_topology_host')
        self.band_floats = max(int(rc), 1)
        self.n_meshes, self.n_nodes, self.n_tris = B, N, T
        self.n_int = meta[:, _nf.M_N_INT].copy()
        self.band = meta[:, _nf.M_BAND].copy()
        self.route = band
        budget = int(lib.gadapt_fem_lds_budget())
        self.max_tris = int(max(tri_counts))
        if band == 'window':
            need = [int(lib.gadapt_fem_window_lds_bytes(int(n), int(w))) for n, w in zip(self.n_int, self.band)]
            if max(need) > budget:
                b = int(np.argmax(need))
                raise NotImplementedError(f"windowed FEM solve: mesh {b} ({int(node_counts[b])} nodes, {int(self.n_int[b])} interior, "
                                          f"half-bandwidth {int(self.band[b])}) needs {need[b]} B of LDS for its ring of band rows; "
                                          f"the limit is {budget} B (square meshes up to 81 x 81 nodes)")
        else:
            need = [int(lib.gadapt_fem_factor_lds_bytes(int(n), int(w))) for n, w in zip(self.n_int, self.band)]
            if max(need) > budget:
                b = int(np.argmax(need))
                raise NotImplementedError(f"pde_loss FEM tail: mesh {b} ({int(node_counts[b])} nodes, {int(self.n_int[b])} interior, "
                                          f"half-bandwidth {int(self.band[b])}) needs {need[b]} B of LDS for its banded factor; the "
                                          f"limit is {budget} B (square meshes up to 26 x 26 nodes)" + WINDOW_HINT)
            eval_need = int(lib.gadapt_fem_eval_lds_bytes(self.max_tris))
            if eval_need > budget:
                raise NotImplementedError(f"pde_loss FEM tail: {self.max_tris} triangles per mesh need {eval_need} B of LDS for the "
                                          f"evaluation's bin mask; the limit is {budget} B" + WINDOW_HINT)
        self.lds_bytes = max(need)
        self.host = dict(meta=meta, cells=cells, node_mesh=node_mesh, tri_mesh=tri_mesh, int_idx=int_idx, int_node=int_node,
                         nt_ptr=nt_ptr, nt_idx=nt_idx, boundary=bnd.astype(bool))
        dev = torch.device(device)
        self.dev = {k: torch.from_numpy(v).to(dev) for k, v in self.host.items() if k != 'boundary'}
        names = ('meta', 'cells', 'node_mesh', 'tri_mesh', 'int_idx', 'int_node', 'nt_ptr', 'nt_idx')
        self._head = {tm: (B, N, T) + tuple(self.dev[k].data_ptr() for k in names if tm or k != 'tri_mesh') for tm in (False, True)}

    def head(self, gptr, gpar, x, lat_x, lat_y, nlat: int, tri_mesh: bool = False, max_tris: bool = True) -> tuple:
        """The arguments every 2-D entry point of include/gadapt_fem.h starts with, in its order: sizes, topology (with
        tri_mesh where the entry point differentiates), Gaussians, coordinates, lattice, max_lds_bytes and max_tris.
        The last guard before the addresses leave: the kernels read gptr[b + 1] of every mesh and x[2 n + 1] of every node."""
        if gptr.numel() != self.n_meshes + 1 or x.numel() != 2 * self.n_nodes or not x.is_contiguous():
            raise ValueError(f"FEM topology of {self.n_meshes} meshes and {self.n_nodes} nodes: Gaussians of {gptr.numel() - 1} meshes, "
                             f"{x.numel()} coordinate values{'' if x.is_contiguous() else ' (not contiguous)'}")
        return (self._head[tri_mesh] + (gptr.data_ptr(), gpar.data_ptr(), x.data_ptr(), lat_x.data_ptr(), lat_y.data_ptr(), nlat,
                                        self.lds_bytes) + ((self.max_tris,) if max_tris else ()))

    def factor_buffer(self, device) -> torch.Tensor:
        """What the solve leaves for the adjoint solve: 'lds' the fp32 band factors (lfac); 'window' the workspace (fp64
        factor rows and y of every mesh), as the fp32 buffer the C-ABI takes."""
        if self.route == 'window':
            floats = int(_nf.lib().gadapt_fem_window_workspace_floats(self.n_meshes, self.host['meta'].ctypes.data))
            return torch.empty(max(floats, 1), device=device)
        return torch.empty(self.band_floats, device=device)

    def backward_buffers(self, device) -> Tuple[torch.Tensor, ...]:
        """(gc [N], mu [N], tgrad [T*6], gx [N,2]) of gadapt_fem_backward[_window]; gx is its result."""
        N, T = self.n_nodes, self.n_tris
        return (torch.empty(N, device=device), torch.empty(N, device=device), torch.empty(T * 6, device=device),
                torch.empty(N, 2, device=device))


_topo_cache: Dict[Tuple, FemTopology] = {}


def _topology(cells: torch.Tensor, boundary: torch.Tensor, node_counts, tri_counts, device, band: str = 'lds') -> FemTopology:
    key = (tuple(int(n) for n in node_counts), tuple(int(t) for t in tri_counts), str(device),
           content_fingerprint([cells, boundary]), band)
    topo = _topo_cache.get(key)
    if topo is None:
        topo = FemTopology(cells.detach().cpu().numpy(), boundary.detach().cpu().numpy(), node_counts, tri_counts, device, band)
        if len(_topo_cache) >= 32:
            _topo_cache.pop(next(iter(_topo_cache)))
        _topo_cache[key] = topo
    return topo


def _check_route(what: str, band, tri_slab) -> int:
    """The route arguments of a FEM tail, before anything is launched: (band, tri_slab) -> tri_slab as an int."""
    if band not in BAND_ROUTES:
        raise ValueError(f"{what}: band must be one of {BAND_ROUTES} (got {band!r})")
    tri_slab = int(tri_slab)
    if tri_slab < 0 or tri_slab % 32:
        raise ValueError(f"{what}: tri_slab must be 0 or a positive multiple of 32 (got {tri_slab})")
    return tri_slab


def _check_adjoint(what: str, adjoint) -> str:
    """The form of the backward's lattice walks, before anything is launched."""
    if adjoint not in ADJOINTS:
        raise ValueError(f"{what}: adjoint must be one of {ADJOINTS} (got {adjoint!r})")
    return adjoint


def _check_forward(what: str, forward, band) -> str:
    """The form of the forward's load vector and evaluation, before anything is launched; 'wave' is built for band='lds'."""
    if forward not in FORWARDS:
        raise ValueError(f"{what}: forward must be one of {FORWARDS} (got {forward!r})")
    if forward == 'wave' and band == 'window':
        raise ValueError(f"{what}: forward='wave' is built for band='lds' only; band='window' has its own load-vector and "
                         "evaluation kernels (use forward='lane')")
    return forward


# operation -> route -> symbol of include/gadapt_fem.h (tests/test_fem_window_grad_host.py pins the pairing)
ENTRY_POINTS = {op: {'lds': f'gadapt_fem_{op}', 'window': f'gadapt_fem_{op}_window'}
                for op in ('forward', 'modular_forward', 'backward', 'eval_errors')}
ENTRY_POINTS['backward_wave'] = {'lds': 'gadapt_fem_backward_wave', 'window': 'gadapt_fem_backward_window_wave'}
ENTRY_POINTS['forward_wave'] = {'lds': 'gadapt_fem_forward_wave'}
ENTRY_POINTS['modular_forward_wave'] = {'lds': 'gadapt_fem_modular_forward_wave'}
ENTRY_POINTS['eval_errors_wave'] = {'lds': 'gadapt_fem_eval_errors_wave'}
_BACKWARD_OP = {'lane': 'backward', 'wave': 'backward_wave'}
_FORWARD_OP = {'lane': 'forward', 'wave': 'forward_wave'}
_MODULAR_OP = {'lane': 'modular_forward', 'wave': 'modular_forward_wave'}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _solve_tail(topo: FemTopology, rhs, coeffs, factor, tri_slab: int) -> tuple:
    """rhs, coeffs and the factor buffer (None: not kept) as the forward and evaluation entry points take them after the
    head; the windowed ones take tri_slab next."""
    return (rhs.data_ptr(), coeffs.data_ptr(), _ptr(factor)) + ((tri_slab,) if topo.route == 'window' else ())


def _host(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else v


def _gaussian_rows(pde_params: Sequence[dict]) -> Tuple[np.ndarray, np.ndarray]:
    """(cumulative counts [B+1] int32, rows [G,4] fp32 = (c0, c1, s0, s1)) on the host: per mesh its own number of Gaussians."""
    counts, rows = [0], []
    for p in pde_params:
        cs, ss = p['centers'], p['scales']
        for c, s in zip(cs, ss):
            c, s = np.asarray(_host(c), np.float32).reshape(-1), np.asarray(_host(s), np.float32).reshape(-1)
            if c.size != 2 or s.size != 2:
                raise ValueError(f"2-D Gaussians: a centre of {c.size} and a scale of {s.size} components; 2 each")
            rows.append([c[0], c[1], s[0], s[1]])
        counts.append(len(cs))
    return np.cumsum(counts).astype(np.int32), np.asarray(rows, np.float32).reshape(-1, 4)


def pack_gaussians(pde_params: Sequence[dict], device) -> Tuple[torch.Tensor, torch.Tensor]:
    """gptr [B+1] int32 and gpar [G,4] fp32 = (c0, c1, s0, s1): per mesh its own number of Gaussians."""
    ptr, rows = _gaussian_rows(pde_params)
    return torch.tensor(ptr, dtype=torch.int32, device=device), torch.tensor(rows, device=device)


def lattice_axes(quad_points, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lat_x, lat_y) of a tensor-product lattice given as [X, Y] = meshgrid(qx, qy, indexing='ij') (GNN.quad_points) or as
    the pair of axes; sol.view(-1)[i * nlat + j] is the point (lat_x[i], lat_y[j])."""
    X, Y = quad_points[0], quad_points[1]
    if X.dim() == 2:
        lx, ly = X[:, 0], Y[0, :]
        if not (torch.equal(X, lx[:, None].expand_as(X)) and torch.equal(Y, ly[None, :].expand_as(Y))):
            raise NotImplementedError("pde_loss FEM tail: quad_points must be meshgrid(qx, qy, indexing='ij') of a lattice")
    else:
        lx, ly = X, Y
    if lx.numel() != ly.numel() or lx.numel() < 2:
        raise NotImplementedError("pde_loss FEM tail: the evaluation lattice must be square (nlat x nlat, nlat >= 2)")
    for a in (lx, ly):
        d = a[1:] - a[:-1]
        if not bool((d > 0).all()) or float((d - d.mean()).abs().max()) > 1e-5 * float(a[-1] - a[0]):
            raise NotImplementedError("pde_loss FEM tail: the evaluation lattice must be uniform and increasing")
    return (lx.detach().to(device=device, dtype=torch.float32).contiguous(),
            ly.detach().to(device=device, dtype=torch.float32).contiguous())


class _FemPoisson(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, topo: FemTopology, gptr, gpar, lat_x, lat_y, tri_slab=0, adjoint='lane', fwd='lane'):
        _require_gpu(x, 'FEM node coordinates')
        x = x.detach().contiguous()
        dev, nlat = x.device, int(lat_x.numel())
        rhs, coeffs = torch.empty(topo.n_nodes, device=dev), torch.empty(topo.n_nodes, device=dev)
        sol = torch.empty(topo.n_meshes * nlat * nlat, device=dev)
        lfac = topo.factor_buffer(dev)                               # kept for the adjoint solve
        _nf.call(ENTRY_POINTS[_FORWARD_OP[fwd]][topo.route], *topo.head(gptr, gpar, x, lat_x, lat_y, nlat),
                 *_solve_tail(topo, rhs, coeffs, lfac, tri_slab), sol.data_ptr(), current_stream(dev))
        ctx.topo, ctx.nlat, ctx.adjoint = topo, nlat, adjoint
        ctx.save_for_backward(x, coeffs, lfac, gptr, gpar, lat_x, lat_y)
        return coeffs, sol

    @staticmethod
    def backward(ctx, g_coeffs, g_sol):
        x, coeffs, lfac, gptr, gpar, lat_x, lat_y = ctx.saved_tensors
        topo, dev = ctx.topo, x.device
        g_coeffs = None if g_coeffs is None else g_coeffs.contiguous().float()
        g_sol = None if g_sol is None else g_sol.contiguous().float()
        return _backward(topo, gptr, gpar, x, lat_x, lat_y, ctx.nlat, coeffs, lfac, g_coeffs, g_sol, current_stream(dev), ctx.adjoint), \
            None, None, None, None, None, None, None, None


def _backward(topo: FemTopology, gptr, gpar, x, lat_x, lat_y, nlat: int, coeffs, factor, g_coeffs, g_sol, stream,
              adjoint: str = 'lane') -> torch.Tensor:
    """gadapt_fem_backward[_window][_wave] on the kept factor: d / d x [N,2] of what g_coeffs and g_sol (None: nothing) seed."""
    gc, mu, tgrad, gx = topo.backward_buffers(x.device)
    _nf.call(ENTRY_POINTS[_BACKWARD_OP[adjoint]][topo.route], *topo.head(gptr, gpar, x, lat_x, lat_y, nlat, tri_mesh=True, max_tris=False),
             coeffs.data_ptr(), factor.data_ptr(), _ptr(g_coeffs), _ptr(g_sol), gc.data_ptr(), mu.data_ptr(), tgrad.data_ptr(),
             gx.data_ptr(), stream)
    return gx


def _tri_counts(cells: torch.Tensor, node_counts: Sequence[int]) -> List[int]:
    """Triangles per mesh of a batch whose cells are ordered mesh by mesh (as `collate` concatenates them)."""
    c0 = cells[:, 0].detach().cpu()
    ends = torch.tensor(np.cumsum(node_counts), dtype=c0.dtype)
    return np.diff(np.concatenate([[0], torch.searchsorted(c0.contiguous(), ends, right=False).numpy()])).tolist()


def fem_poisson(x_phys: torch.Tensor, cells: torch.Tensor, boundary: torch.Tensor, node_counts: Sequence[int],
                pde_params: Sequence[dict], quad_points, tri_counts: Optional[Sequence[int]] = None, band: str = 'lds',
                tri_slab: int = 0, adjoint: str = 'lane', *, forward: str = 'lane'):
    """Batched P1 Poisson solve on the meshes of `x_phys` [N,2] (differentiable wrt x_phys).

    cells [T,3] global node ids, mesh by mesh; boundary [N] bool; node_counts per mesh; pde_params per mesh
    ({'centers': [...], 'scales': [...]}, any number of Gaussians); quad_points the evaluation lattice (GNN.quad_points).
    Returns coeffs [N,1] and sol [B*nlat*nlat] (mesh by mesh, lattice row-major).

    band: 'lds' keeps each mesh's banded factor resident in LDS (square meshes up to 26 x 26 nodes); 'window' is the
    windowed solve of `poisson_eval_errors(band='window')` (fp64 ring, factor and substitutions, fp64 forcing in the load
    vector; square meshes up to 81 x 81 nodes) with its workspace kept for an fp64 adjoint solve in the backward, and the
    lattice evaluated over slabs of `tri_slab` triangle ids (a multiple of 32; 0: the largest slab the LDS budget leaves).
    Where both routes take a mesh their results agree to the rounding of an fp32 solve, not bitwise; the windowed result
    does not depend on `tri_slab`, bit for bit.

    adjoint: 'lane' walks the lattice in the backward with a lane per node and per triangle; 'wave' with a wave each
    (gadapt_fem_backward[_window]_wave).  The gradient is the same, bit for bit.

    forward: 'lane' computes the load vector with a lane per node and the evaluation with five lattice points per lane; 'wave'
    (band='lds' only) with a wave per node and a wave per chunk of the lattice, two phases per point
    (gadapt_fem_forward_wave).  coeffs, sol and the factor the backward reads are the same, bit for bit."""
    tri_slab = _check_route('pde_loss FEM tail', band, tri_slab)
    _check_adjoint('pde_loss FEM tail', adjoint)
    _check_forward('pde_loss FEM tail', forward, band)
    node_counts = _check_batch_2d('pde_loss FEM tail (fem_poisson)', x_phys, node_counts, pde_params, cells, boundary, tri_counts)
    _require_gpu(x_phys, 'pde_loss FEM tail')
    dev = x_phys.device
    if tri_counts is None:
        tri_counts = _tri_counts(cells, node_counts)
    topo = _topology(cells, boundary, node_counts, tri_counts, dev, band)
    gptr, gpar = pack_gaussians(pde_params, dev)
    lx, ly = lattice_axes(quad_points, dev)
    coeffs, sol = _FemPoisson.apply(x_phys, topo, gptr, gpar, lx, ly, tri_slab, adjoint, forward)
    return coeffs.unsqueeze(1), sol


def torch_FEM_2D(opt, mesh, mesh_points, quad_points, num_meshpoints, c_list, s_list):
    """The reference's entry point (`difFEM_2d.py:320-372`) on one mesh: (coeffs [N,1], mesh_points, sol shaped as
    quad_points[0]).  opt['fem_band'] = 'window' takes meshes beyond 26 x 26 nodes, up to 81 x 81 (`fem_poisson`);
    opt['fem_forward'] = 'wave' the wave-parallel forward (band 'lds')."""
    band = opt.get('fem_band', 'lds')
    _check_route('torch_FEM_2D', band, 0)
    forward = _check_forward("torch_FEM_2D (opt['fem_forward'])", opt.get('fem_forward', 'lane'), band)
    cells_np = np.asarray(mesh.coordinates.cell_node_map().values, dtype=np.int64)
    n = mesh_points.shape[0]
    if n != num_meshpoints ** 2:
        raise ValueError(f"torch_FEM_2D: {n} mesh points for num_meshpoints={num_meshpoints}")
    cells = torch.from_numpy(cells_np)
    boundary = torch.from_numpy(boundary_from_cells(cells_np, n))
    params = [{'centers': [np.asarray(c.detach().cpu() if torch.is_tensor(c) else c, np.float32) for c in c_list],
               'scales': [np.asarray(s.detach().cpu() if torch.is_tensor(s) else s, np.float32) for s in s_list]}]
    coeffs, sol = fem_poisson(mesh_points, cells, boundary, [n], params, quad_points, tri_counts=[cells_np.shape[0]], band=band,
                              forward=forward)
    shape = quad_points[0].shape if quad_points[0].dim() == 2 else (quad_points[0].numel(), quad_points[1].numel())
    return coeffs, mesh_points, sol.view(shape)


def _batch_counts(data, x_phys: torch.Tensor) -> Tuple[int, List[int]]:
    """(meshes, nodes per mesh) of a batch as `GNN.forward` is given it; reads `data.batch` back from the device."""
    batch = data.batch
    B = int(data.num_graphs) if hasattr(data, 'num_graphs') else int(batch.max()) + 1
    if batch is None:
        return B, [x_phys.shape[0]]
    return B, torch.bincount(batch.detach().cpu(), minlength=B).tolist()


def batch_params(opt, data, B: int) -> list:
    """The Gaussians of a batch, one dict per mesh: `data.batch_dict[i]['pde_params']` for randg_mix, else `data.pde_params`."""
    if opt.get('data_type') == 'randg_mix' and hasattr(data, 'batch_dict'):
        return [data.batch_dict[i]['pde_params'] for i in range(B)]
    return data.pde_params if isinstance(data.pde_params, (list, tuple)) else [data.pde_params]


def _batch_cells(model, data, node_counts: Sequence[int], B: int):
    """(cells, boundary, tri_counts or None) of a batch: `data.cells` / `data.boundary_nodes`, else the per-mesh topology
    objects (the reference's mesh / data.mesh[i]) and the edges that belong to one triangle."""
    cells = getattr(data, 'cells', None)
    tri_counts = None
    if cells is None:
        meshes = data.mesh if isinstance(getattr(data, 'mesh', None), (list, tuple)) else [model.dataset.mesh] * B
        parts, off = [], 0
        for m, n in zip(meshes, node_counts):
            parts.append(torch.as_tensor(np.asarray(m.coordinates.cell_node_map().values, np.int64)) + off)
            off += n
        cells, tri_counts = torch.cat(parts, 0), [p.shape[0] for p in parts]
    boundary = getattr(data, 'boundary_nodes', None)
    if boundary is None:
        boundary = torch.from_numpy(boundary_from_cells(cells.cpu().numpy(), sum(node_counts)))
    return cells, boundary, tri_counts


def _check_tail(model):
    """(band, adjoint) of a model's pde_loss tail; refuses what it is not built for before anything is launched."""
    o = model.opt
    band, adjoint = o.get('fem_band', 'lds'), o.get('fem_adjoint', 'lane')
    _check_route("loss_type='pde_loss'", band, 0)
    _check_adjoint("loss_type='pde_loss' (opt['fem_adjoint'])", adjoint)
    _check_forward("loss_type='pde_loss' (opt['fem_forward'])", o.get('fem_forward', 'lane'), band)
    if model.dim == 1 and o.get('pde_loss_1d') and o.get('pde_type', 'Poisson') == 'Poisson':
        return band, adjoint                                 # the 1-D tail (fem1d.gnn_pde_tail_1d): opt-in, one route
    if model.dim != 2:
        raise NotImplementedError("loss_type='pde_loss' is built for 2-D Poisson only; the 1-D tail (torch_FEM_1D) is out of scope "
                                  "unless opt['pde_loss_1d'] is set (1-D Poisson)")
    if o.get('pde_type', 'Poisson') != 'Poisson':
        raise NotImplementedError(f"loss_type='pde_loss' is built for 2-D Poisson only (pde_type={o.get('pde_type')!r})")
    return band, adjoint


def gnn_pde_tail(model, data, x_phys: torch.Tensor):
    """`GNN.forward`'s pde_loss branch (`src/GNN.py:307-342`) for a batch: (coeffs [N,1], x_phys, sol [B*Q]).
    opt['fem_band'] = 'window' takes meshes beyond 26 x 26 nodes, up to 81 x 81 (`fem_poisson`); opt['fem_adjoint'] = 'wave'
    the wave-parallel backward, opt['fem_forward'] = 'wave' the wave-parallel forward (band 'lds').  A batch that carries a
    `PdeBatch` (`data._pde_batch`) is solved through it: the launches alone, nothing read back from the device or sent to it
    (its route and Gaussians are the descriptor's)."""
    band, adjoint = _check_tail(model)
    if model.dim == 1:                                       # opt['pde_loss_1d']: torch_FEM_1D per mesh (src/GNN.py:319-325)
        from .fem1d import gnn_pde_tail_1d
        return gnn_pde_tail_1d(model, data, x_phys)
    pb = getattr(data, '_pde_batch', None)
    if pb is not None:
        coeffs, sol = pb.solve(x_phys)
        return coeffs, x_phys, sol
    B, node_counts = _batch_counts(data, x_phys)
    params = batch_params(model.opt, data, B)
    cells, boundary, tri_counts = _batch_cells(model, data, node_counts, B)
    coeffs, sol = fem_poisson(x_phys, cells, boundary, node_counts, params, model.quad_points, tri_counts=tri_counts, band=band,
                              adjoint=adjoint, forward=model.opt.get('fem_forward', 'lane'))
    return coeffs, x_phys, sol


class PdeBatch:
    """The pde_loss tail of ONE batch topology, ready to launch: the `FemTopology`, the lattice axes, the node and triangle
    counts, and the Gaussians' device buffers `gptr` [B+1] int32 and `gpar` [cap,4] fp32 with a pinned host copy to stage
    them in.  `solve` is `fem_poisson` without its per-call host work (no topology fingerprint, no tensors built from
    Python lists, nothing read back): it can be stream-captured.  `set_params` feeds another batch's Gaussians into the
    SAME device buffers, which is how a captured step sees them.

        pb = PdeBatch.from_data(model, data)      # may synchronise, once
        data._pde_batch = pb                      # `gnn_pde_tail` (GNN.forward) now solves through it
        pb.set_params(next_batch.pde_params)
    """

    def __init__(self, topo: FemTopology, lat_x: torch.Tensor, lat_y: torch.Tensor, cap: int, adjoint: str = 'lane', tri_slab: int = 0, *,
                 forward: str = 'lane'):
        _check_adjoint('PdeBatch', adjoint)
        self.tri_slab = _check_route('PdeBatch', topo.route, tri_slab)
        self.forward = _check_forward('PdeBatch', forward, topo.route)
        if int(cap) < 1:
            raise ValueError(f"PdeBatch: room for {cap} Gaussians")
        self.topo, self.lat_x, self.lat_y, self.adjoint = topo, lat_x, lat_y, adjoint
        self.n_meshes, self.n_nodes, self.n_tris, self.cap = int(topo.n_meshes), int(topo.n_nodes), int(topo.n_tris), int(cap)
        dev = lat_x.device
        self.gptr = torch.zeros(self.n_meshes + 1, dtype=torch.int32, device=dev)
        self.gpar = torch.zeros(self.cap, 4, dtype=torch.float32, device=dev)
        pin = dev.type == 'cuda'
        self.host_gptr = torch.zeros(self.n_meshes + 1, dtype=torch.int32, pin_memory=pin)
        self.host_gpar = torch.zeros(self.cap, 4, dtype=torch.float32, pin_memory=pin)
        self._staged = torch.cuda.Event() if pin else None       # recorded behind the copies out of the staging buffers

    @classmethod
    def from_data(cls, model, data, max_gauss: int = 8, adjoint: Optional[str] = None, forward: Optional[str] = None) -> 'PdeBatch':
        """The descriptor of `data`'s topology for `model`'s tail (opt['fem_band'], and opt['fem_adjoint'] and opt['fem_forward']
        unless `adjoint` and `forward` are given), with room for `max_gauss` Gaussians per mesh; the batch's own Gaussians are
        set if it carries any."""
        band, opt_adjoint = _check_tail(model)
        dev = torch.device(model.opt['device'])
        n = int(data.x_comp.shape[0])
        B, node_counts = _batch_counts(data, data.x_comp)
        cells, boundary, tri_counts = _batch_cells(model, data, node_counts, B)
        if tri_counts is None:
            tri_counts = _tri_counts(cells, node_counts)
        topo = _topology(cells, boundary, node_counts, tri_counts, dev, band)
        lx, ly = lattice_axes(model.quad_points, dev)
        pb = cls(topo, lx, ly, B * int(max_gauss), adjoint if adjoint is not None else opt_adjoint,
                 forward=forward if forward is not None else model.opt.get('fem_forward', 'lane'))
        if n != pb.n_nodes:
            raise ValueError(f"PdeBatch: {n} nodes in the batch, {pb.n_nodes} in its topology")
        try:
            params = batch_params(model.opt, data, B)
        except (AttributeError, KeyError):
            params = None
        if params is not None:
            pb.set_params(params)
        return pb

    def set_params(self, pde_params: Sequence[dict]):
        """The Gaussians of the next solve, `pack_gaussians`' layout and order: packed into the pinned buffers, then one
        non-blocking copy each into `gptr` and `gpar` on the current stream (rows past the last Gaussian keep what they
        held; nothing reads them)."""
        if len(pde_params) != self.n_meshes:
            raise ValueError(f"PdeBatch: Gaussians of {len(pde_params)} meshes for a batch of {self.n_meshes}")
        ptr, rows = _gaussian_rows(pde_params)
        if rows.shape[0] > self.cap:
            raise ValueError(f"PdeBatch: {rows.shape[0]} Gaussians in the batch, room for {self.cap} (from_data's max_gauss per mesh)")
        if self._staged is not None:
            self._staged.synchronize()                           # the previous copies have left the staging buffers
        self.host_gptr.copy_(torch.from_numpy(ptr))
        self.host_gpar[:rows.shape[0]].copy_(torch.from_numpy(rows))
        self.gptr.copy_(self.host_gptr, non_blocking=True)
        self.gpar.copy_(self.host_gpar, non_blocking=True)
        if self._staged is not None:
            self._staged.record()

    def solve(self, x_phys: torch.Tensor):
        """(coeffs [N,1], sol [B*Q]) of `fem_poisson` on this topology and the Gaussians last set: the same entry points on
        the same inputs, the same bits."""
        _check_fp32('PdeBatch', x_phys)
        if x_phys.dim() != 2 or x_phys.shape[1] != 2 or x_phys.shape[0] != self.n_nodes:
            raise ValueError(f"PdeBatch: x_phys {tuple(x_phys.shape)} for a topology of {self.n_nodes} nodes in 2-D")
        coeffs, sol = _FemPoisson.apply(x_phys, self.topo, self.gptr, self.gpar, self.lat_x, self.lat_y, self.tri_slab, self.adjoint,
                                        self.forward)
        return coeffs.unsqueeze(1), sol


# ------------------------------------------------------------------------------------------------ the 2-D modular loss
GRAD_TYPES_2D = ('PDE_loss_direct_mse', 'PDE_loss_direct_L2', 'PDE_loss_adjoint_L2')
_REDUCTIONS = {'mse': _nf.LOSS_MSE, 'simpson': _nf.LOSS_SIMPSON}


def simpson_points_per_dim(N: int, dim: int = 2) -> int:
    """Points per dimension of torchquad's Simpson().integrate(N=N, dim=dim): floor(N^(1/dim)), lowered to an odd count
    (the composite rule needs one), at least 3.  101 -> 9."""
    n = int(int(N) ** (1.0 / dim) + 1e-8)
    if n % 2 == 0:
        n -= 1
    return max(n, 3)


def modular_loss_2d(x_phys: torch.Tensor, cells: torch.Tensor, boundary: torch.Tensor, node_counts: Sequence[int],
                    pde_params: Sequence[dict], n_lat: int, reduction: str, n_load: Optional[int] = None,
                    tri_counts: Optional[Sequence[int]] = None, band: str = 'lds',
                    tri_slab: int = 0, adjoint: str = 'lane', *, forward: str = 'lane') -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-mesh 2-D modular loss and its gradient: (loss [B], x_grads [N,2]), x_grads on a node being the gradient of its
    own mesh's loss wrt all of that mesh's node coordinates.

    The P1 Poisson solve of `fem_poisson` on each mesh, evaluated on the lattice linspace(0, 1, n_lat)^2 (meshgrid 'ij'),
    and e = sol - u_true there: reduction 'mse' is mean e^2 (F.mse_loss), 'simpson' torchquad's composite Simpson rule of
    e^2 over [0,1]^2 (n_lat odd).  n_load: Simpson points per dimension of the load vector; only the compiled
    `gadapt_fem_simpson_points()` is built.  Five launches forward and backward, no autograd graph, no host wait.
    band, tri_slab, adjoint: as `fem_poisson` ('window': square meshes up to 81 x 81 nodes; 'wave': the wave-parallel lattice
    walks of the backward, the same bits).  forward: as `fem_poisson` ('wave', band='lds' only: gadapt_fem_modular_forward_wave,
    the same loss and gradient bits)."""
    tri_slab = _check_route('modular loss (2-D)', band, tri_slab)
    _check_adjoint('modular loss (2-D)', adjoint)
    _check_forward('modular loss (2-D)', forward, band)
    node_counts = _check_batch_2d('modular loss (2-D)', x_phys, node_counts, pde_params, cells, boundary, tri_counts)
    if reduction not in _REDUCTIONS:
        raise ValueError(f"modular loss (2-D): reduction must be one of {sorted(_REDUCTIONS)} (got {reduction!r})")
    n_lat = int(n_lat)
    if n_lat < 2 or (reduction == 'simpson' and (n_lat < 3 or n_lat % 2 == 0)):
        raise ValueError(f"modular loss (2-D): {n_lat} lattice points per dimension for reduction {reduction!r}")
    _require_gpu(x_phys, 'modular loss (2-D)')
    lib = _nf.lib()
    n_built = int(lib.gadapt_fem_simpson_points())
    if n_load is not None and int(n_load) != n_built:
        raise NotImplementedError(f"modular loss (2-D): the load vector's Simpson rule is built for {n_built} points per "
                                  f"dimension only (got {int(n_load)})")
    dev = x_phys.device
    x = x_phys.detach().contiguous()
    if tri_counts is None:
        tri_counts = _tri_counts(cells, node_counts)
    topo = _topology(cells, boundary, node_counts, tri_counts, dev, band)
    gptr, gpar = pack_gaussians(pde_params, dev)
    lat = torch.linspace(0, 1, n_lat).to(dev)              # torch's CPU linspace: the reference's lattice, point for point
    N, Q = topo.n_nodes, topo.n_meshes * n_lat * n_lat
    rhs, coeffs, lfac = torch.empty(N, device=dev), torch.empty(N, device=dev), topo.factor_buffer(dev)
    sol, g_sol, loss = torch.empty(Q, device=dev), torch.empty(Q, device=dev), torch.empty(topo.n_meshes, device=dev)
    stream = current_stream(dev)
    _nf.call(ENTRY_POINTS[_MODULAR_OP[forward]][topo.route], *topo.head(gptr, gpar, x, lat, lat, n_lat), _REDUCTIONS[reduction],
             *_solve_tail(topo, rhs, coeffs, lfac, tri_slab), sol.data_ptr(), loss.data_ptr(), g_sol.data_ptr(), stream)
    return loss, _backward(topo, gptr, gpar, x, lat, lat, n_lat, coeffs, lfac, None, g_sol, stream, adjoint)


def _modular_quadrature(opt, gt: str) -> Tuple[int, int, str]:
    """(load-vector Simpson points per dimension, loss lattice points per dimension, reduction) of a grad_type."""
    ev, ld = int(opt.get('eval_quad_points', 101)), int(opt.get('load_quad_points', 101))
    if gt == 'PDE_loss_direct_mse':                        # difFEM_2d.py:409, :424-435
        return simpson_points_per_dim(ev), ev, 'mse'
    n = simpson_points_per_dim(ev if gt == 'PDE_loss_direct_L2' else ld)   # :462/:476, adjoint :505/:523
    return n, n, 'simpson'


def _modular_batch(opt, data, n_nodes: int):
    """(cells, boundary, node_counts, tri_counts, pde_params) of a batch, as gnn_pde_tail reads them."""
    batch = getattr(data, 'batch', None)
    B = int(data.num_graphs) if hasattr(data, 'num_graphs') else (1 if batch is None else int(batch.max()) + 1)
    node_counts = [n_nodes] if batch is None else torch.bincount(batch.detach().cpu(), minlength=B).tolist()
    if opt.get('data_type') == 'randg_mix' and hasattr(data, 'batch_dict'):
        params = [data.batch_dict[i]['pde_params'] for i in range(B)]
    else:
        from .fem1d import _split_params
        params = _split_params(data.pde_params, B)
    cells, tri_counts = getattr(data, 'cells', None), None
    if cells is None:                                    # per-mesh topology objects, else the reference's UnitSquareMesh
        mesh = getattr(data, 'mesh', None)
        if isinstance(mesh, (list, tuple)):
            tops = [np.asarray(m.coordinates.cell_node_map().values, np.int64) for m in mesh]
        elif mesh is not None:
            tops = [np.asarray(mesh.coordinates.cell_node_map().values, np.int64)] * B
        else:
            from .mesh_graph import square_mesh
            tops = [square_mesh(int(opt['mesh_dims'][0])).cells.numpy()] * B
        parts, off = [], 0
        for t, n in zip(tops, node_counts):
            parts.append(torch.as_tensor(t) + off)
            off += n
        cells, tri_counts = torch.cat(parts, 0), [p.shape[0] for p in parts]
    boundary = getattr(data, 'boundary_nodes', None)
    if boundary is None:
        boundary = torch.from_numpy(boundary_from_cells(cells.cpu().numpy(), sum(node_counts)))
    return cells, boundary, node_counts, tri_counts, params


def gradient_meshpoints_2D(opt, data, x_phys):
    """The reference's 2-D modular loss (`difFEM_2d.py:374-535`, from `src/run_GNN.py:113-118`) for a batch:
    (loss, x_grads [N,2]); training back-propagates sum(x_phys * x_grads).

    Per mesh, as the reference at batch 1: x_grads on a node is the gradient of its own mesh's loss wrt all of that mesh's
    node coordinates, boundary nodes included; loss is the mean of the per-mesh losses, a 0-dim tensor on the device
    (the reference returns it on the CPU).  Nothing waits for the device.

    grad_type (opt['grad_type']):
      PDE_loss_direct_mse   mean over linspace(0, 1, eval_quad_points)^2 of (sol - u_true)^2; load vector with
                            eval_quad_points
      PDE_loss_direct_L2    torchquad's Simpson rule of (sol - u_true)^2 over [0,1]^2; load vector and loss with
                            eval_quad_points
      PDE_loss_adjoint_L2   the same loss with load_quad_points for both.  The reference solves without differentiating
                            and adds grad1 + grad2 from lambda = -A^-T dL/dc; in exact arithmetic that is the direct
                            gradient, and the backward here already is an adjoint solve on the kept factor, so the two
                            _L2 types share one path and differ only in the count they read.
    Quadrature counts N become torchquad's points per dimension (`simpson_points_per_dim`: 101 -> 9); the load vector is
    built for `gadapt_fem_simpson_points()` only (NotImplementedError otherwise), the loss lattice takes any count.
    Topology: data.cells (as collate offsets them), else data.mesh / data.mesh[i], else square_mesh(mesh_dims[0]).
    Limits as the pde_loss tail: 2-D Poisson, square meshes up to 26 x 26 nodes (the LDS budget of the banded factor), or
    up to 81 x 81 with opt['fem_band'] = 'window' (`modular_loss_2d(band='window')`).  opt['fem_adjoint'] = 'wave': the
    wave-parallel backward (`modular_loss_2d(adjoint='wave')`), the same bits; opt['fem_forward'] = 'wave': the wave-parallel
    forward (`modular_loss_2d(forward='wave')`, band 'lds'), the same bits.
    The reference's build_mass_matrix is called with three of its four arguments there (a TypeError as shipped); this
    builds the evident intent, the stiffness of torch_FEM_2D."""
    if 'grad_type' not in opt:
        raise ValueError("Error: opt['grad_type'] not specified")
    gt = opt['grad_type']
    if gt not in GRAD_TYPES_2D:
        raise ValueError("Error: opt['grad_type'] incorrectly specified")
    if x_phys.dim() != 2 or x_phys.shape[1] != 2:
        raise NotImplementedError(f"gradient_meshpoints_2D: x_phys must be [N,2] (got {tuple(x_phys.shape)}); "
                                  "1-D meshes take gradient_meshpoints_1D")
    band = opt.get('fem_band', 'lds')
    _check_route('gradient_meshpoints_2D', band, 0)
    adjoint = _check_adjoint("gradient_meshpoints_2D (opt['fem_adjoint'])", opt.get('fem_adjoint', 'lane'))
    forward = _check_forward("gradient_meshpoints_2D (opt['fem_forward'])", opt.get('fem_forward', 'lane'), band)
    n_load, n_lat, reduction = _modular_quadrature(opt, gt)
    cells, boundary, node_counts, tri_counts, params = _modular_batch(opt, data, x_phys.shape[0])
    _check_batch_2d('gradient_meshpoints_2D', x_phys, node_counts, params, cells, boundary, tri_counts, cast=True)
    loss, x_grads = modular_loss_2d(x_phys.detach().float(), cells, boundary, node_counts, params, n_lat, reduction,
                                    n_load=n_load, tri_counts=tri_counts, band=band, adjoint=adjoint,
                                    forward=forward)
    return loss.mean(), x_grads
