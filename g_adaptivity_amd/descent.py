"""Gradient descent of the mesh nodes on the FEM error, all epochs enqueued by one call (the reference's backFEM loops).

The reference's `backFEM_*` baselines move the mesh points themselves by SGD on the L2 error of the Poisson solve, with no
network: `train_step_adjoint` (`firedrake_difFEM/difFEM_2d.py:593-685`) and `train_step_vec` (`difFEM_1d.py:241-292`).  Here
a whole batch descends at once and the loop lives behind the C-ABI (`gadapt_fem_descend[_wave]`, `gadapt_fem1d_descend`;
fem_csrc/descent_kernels.hip): per epoch the launches of the modular loss (`modular_loss_2d`: nine; 1-D: forward, L2 seed,
backward) and one step launch that does the optimizer's update, keeps the epoch's loss and mesh and watches for tangling.
Nothing waits for the device between epochs or at the end.

    mesh_descent_2d(x0, cells, boundary, node_counts, pde_params, epochs, lr, ...) -> DescentResult
    mesh_descent_1d(x0, node_counts, pde_params, opt, epochs, lr, mesh_params='internal', ...) -> DescentResult

Limits as the FEM tails: 2-D square meshes up to 26 x 26 nodes and the built 9-point load rule; 1-D up to 1024 nodes.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import _native_fem as _nf
from ._native import NativeError, current_stream
from .fem import _check_adjoint, _check_forward, _ptr, _topology, _tri_counts, pack_gaussians
from .fem1d import _Batch, _points, _watch_flags

__all__ = ['DescentResult', 'mesh_descent_2d', 'mesh_descent_1d', 'LAUNCHES_PER_EPOCH_2D', 'LAUNCHES_PER_EPOCH_1D']

LAUNCHES_PER_EPOCH_2D = 9             # modular forward 4, backward 4, step 1 (plus one orientation launch per call)
LAUNCHES_PER_EPOCH_1D = 4             # forward, L2 seed, backward, step (plus one initialising launch per call)
_MESH_PARAMS = {'internal': _nf.DESCEND_INTERNAL, 'all': _nf.DESCEND_ALL}


@dataclass
class DescentResult:
    """What a descent leaves, all on the device.

    x              the coordinates after the last step ([N,2], or [N] in 1-D)
    coeffs [N]     the FEM coefficients of the LAST EPOCH'S solve, i.e. on the mesh before the last step: the reference
                   returns `out_nograd` / `out` of its last iteration, and so does this (None when epochs == 0)
    loss_hist      [E,B]: loss of epoch j on the mesh before that epoch's step
    mesh_hist      [E,N,2] / [E,N]: the coordinates after each step, or None
    first_tangled  [B] int32: the first epoch whose step left a triangle with the wrong orientation (1-D: an interval of
                   length <= 0) or a NaN, -1 if none; the descent goes on regardless, as the reference's does
    min_area       [B]: the smallest oriented triangle determinant (1-D: interval) after the latest step, frozen at the first
                   tangled epoch; +inf when no step ran
    sol            1-D only: [B,P], the last epoch's solution at the evaluation points"""
    x: torch.Tensor
    coeffs: Optional[torch.Tensor]
    loss_hist: torch.Tensor
    mesh_hist: Optional[torch.Tensor]
    first_tangled: torch.Tensor
    min_area: torch.Tensor
    sol: Optional[torch.Tensor] = None


def _require_gpu(t, what: str):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise NativeError(f"{what}: the mesh descent runs on the MI355X only (got a "
                          f"{t.device if torch.is_tensor(t) else type(t).__name__} tensor); there is no CPU fallback")


def mesh_descent_2d(x0: torch.Tensor, cells: torch.Tensor, boundary: torch.Tensor, node_counts: Sequence[int],
                    pde_params: Sequence[dict], epochs: int, lr: float, n_lat: Optional[int] = None, n_load: Optional[int] = None,
                    x_ref: Optional[torch.Tensor] = None, keep_meshes: bool = False,
                    tri_counts: Optional[Sequence[int]] = None, *, forward: str = 'lane', adjoint: str = 'lane') -> DescentResult:
    """`epochs` steps of x[interior] -= lr * d loss_b / d x on every mesh of x0 [N,2] at once, loss_b the Simpson L2 error of
    mesh b's Poisson solve against its own Gaussians (`modular_loss_2d(..., n_lat, 'simpson')`; n_lat defaults to the
    reference's 9 points per dimension, what torchquad makes of load_quad_points = 101).  Bit-identical to that loop written
    with `modular_loss_2d` and a torch update.  x0 is not modified.

    x_ref: the mesh whose triangle orientations count as untangled (default x0).  keep_meshes: also return every epoch's
    mesh.  Refuses what `modular_loss_2d` refuses: meshes beyond the LDS budget (26 x 26 nodes), a load rule other than the
    built one.  epochs == 0 is valid.

    forward, adjoint: 'lane' (the default: `gadapt_fem_descend`) or 'wave', the wave-parallel form of every epoch's load
    vector and evaluation (`modular_loss_2d(forward='wave')`) and of its backward's two lattice walks
    (`modular_loss_2d(adjoint='wave')`), through `gadapt_fem_descend_wave` when either is 'wave'.  Every field of the result
    has the same bits whichever pair is chosen."""
    _check_forward('mesh_descent_2d', forward, 'lds')
    _check_adjoint('mesh_descent_2d', adjoint)
    _require_gpu(x0, 'mesh_descent_2d')
    if x0.dtype != torch.float32:
        raise TypeError(f"mesh_descent_2d: fp32 expected, got {x0.dtype}")
    if x0.dim() != 2 or x0.shape[1] != 2:
        raise NotImplementedError(f"mesh_descent_2d: x0 must be [N,2] (got {tuple(x0.shape)}); 1-D meshes take mesh_descent_1d")
    epochs = int(epochs)
    if epochs < 0:
        raise ValueError("mesh_descent_2d: epochs >= 0")
    lib = _nf.lib()
    n_built = int(lib.gadapt_fem_simpson_points())
    if n_load is not None and int(n_load) != n_built:
        raise NotImplementedError(f"mesh_descent_2d: the load vector's Simpson rule is built for {n_built} points per dimension "
                                  f"only (got {int(n_load)})")
    n_lat = n_built if n_lat is None else int(n_lat)
    if n_lat < 3 or n_lat % 2 == 0:
        raise ValueError(f"mesh_descent_2d: {n_lat} lattice points per dimension; the Simpson rule needs an odd count >= 3")
    dev = x0.device
    if tri_counts is None:
        tri_counts = _tri_counts(cells, node_counts)
    topo = _topology(cells, boundary, node_counts, tri_counts, dev)          # refuses meshes beyond the LDS budget
    N, T, B = topo.n_nodes, topo.n_tris, topo.n_meshes
    if x0.shape[0] != N:
        raise ValueError(f"mesh_descent_2d: {x0.shape[0]} coordinates for {N} nodes")
    if x_ref is not None:
        _require_gpu(x_ref, 'mesh_descent_2d (x_ref)')
        if x_ref.shape != x0.shape:
            raise ValueError(f"mesh_descent_2d: x_ref {tuple(x_ref.shape)} for x0 {tuple(x0.shape)}")
        x_ref = x_ref.detach().float().contiguous()
    gptr, gpar = pack_gaussians(pde_params, dev)
    lat = torch.linspace(0, 1, n_lat).to(dev)                                # the lattice of modular_loss_2d, point for point
    x = x0.detach().clone().contiguous()
    Q = n_lat * n_lat
    f = lambda *shape: torch.empty(*shape, device=dev)
    rhs, coeffs, lfac, sol, g_sol, loss = f(N), f(N), topo.factor_buffer(dev), f(B * Q), f(B * Q), f(B)
    gc, mu, tgrad, gx = topo.backward_buffers(dev)
    loss_hist = f(epochs, B)
    mesh_hist = f(epochs, N, 2) if keep_meshes else None
    first_tangled = torch.empty(B, dtype=torch.int32, device=dev)
    min_area = f(B)
    sign = torch.empty(T, dtype=torch.int8, device=dev)
    head = topo.head(gptr, gpar, x, lat, lat, n_lat, tri_mesh=True)
    routes = (_nf.ROUTE_WAVE_FORWARD if forward == 'wave' else 0) | (_nf.ROUTE_WAVE_ADJOINT if adjoint == 'wave' else 0)
    args = (*head[:-5], _ptr(x_ref), *head[-5:],                                # x_ref comes after x, before the lattice
            epochs, float(lr), rhs.data_ptr(), coeffs.data_ptr(), lfac.data_ptr(), sol.data_ptr(), loss.data_ptr(), g_sol.data_ptr(),
            gc.data_ptr(), mu.data_ptr(), tgrad.data_ptr(), gx.data_ptr(), loss_hist.data_ptr() if epochs else None, _ptr(mesh_hist),
            first_tangled.data_ptr(), min_area.data_ptr(), sign.data_ptr())
    if routes:
        _nf.call('gadapt_fem_descend_wave', *args, routes, current_stream(dev))
    else:
        _nf.call('gadapt_fem_descend', *args, current_stream(dev))
    return DescentResult(x=x, coeffs=coeffs if epochs else None, loss_hist=loss_hist, mesh_hist=mesh_hist,
                         first_tangled=first_tangled, min_area=min_area)


def mesh_descent_1d(x0: torch.Tensor, node_counts: Sequence[int], pde_params: Sequence[dict], opt, epochs: int, lr: float,
                    mesh_params: str = 'internal', keep_meshes: bool = False, points=None) -> DescentResult:
    """`epochs` SGD steps on every 1-D mesh of x0 [N] at once (`train_step_vec`), the loss of mesh b being
    torch.trapezoid((sol - u_true)^2, points) of its Poisson solve (`gradient_meshpoints_1D` with PDE_loss_direct_L2).

    mesh_params 'internal': the end nodes stay.  'all': every node moves, then the mesh is rescaled to
    (x - min) / (max - min) and its ends set to 0 and 1, as the reference does (it does not sort, despite its comment).
    opt supplies load_quad_points, stiff_quad_points and eval_quad_points as `fem_poisson_1d` reads them.  The result also
    carries `sol` [B,P] of the last epoch.  x0 is not modified."""
    _require_gpu(x0, 'mesh_descent_1d')
    if x0.dim() == 2 and x0.shape[1] == 1:
        x0 = x0[:, 0]
    if x0.dim() != 1:
        raise ValueError(f"mesh_descent_1d: x0 must be [N] (got {tuple(x0.shape)})")
    if mesh_params not in _MESH_PARAMS:
        raise ValueError(f"mesh_descent_1d: mesh_params must be 'internal' or 'all' (got {mesh_params!r})")
    epochs = int(epochs)
    if epochs < 0:
        raise ValueError("mesh_descent_1d: epochs >= 0")
    dev = x0.device
    bt = _Batch(node_counts, pde_params, dev)                                # refuses meshes beyond 1024 nodes
    if min(bt.counts) < 3:
        raise ValueError("mesh_descent_1d: every mesh needs at least 3 nodes")
    N = sum(bt.counts)
    if x0.shape[0] != N:
        raise ValueError(f"mesh_descent_1d: {x0.shape[0]} coordinates for node_counts summing to {N}")
    pts = _points(opt, dev, points)
    P, B = pts.numel(), bt.B
    if P < 2:
        raise ValueError("mesh_descent_1d: at least 2 evaluation points")
    x = x0.detach().float().clone().contiguous()
    f = lambda *shape: torch.empty(*shape, device=dev)
    coeffs, sol, loss, g_sol, gx = f(N), f(B, P), f(B), f(B, P), f(N)
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    loss_hist = f(epochs, B)
    mesh_hist = f(epochs, N) if keep_meshes else None
    first_tangled = torch.empty(B, dtype=torch.int32, device=dev)
    min_area = f(B)
    _nf.call('gadapt_fem1d_descend', *bt.head(x), int(opt.get('load_quad_points', 101)), int(opt.get('stiff_quad_points', 3)), P,
             pts.data_ptr(), epochs, float(lr), _MESH_PARAMS[mesh_params], N, coeffs.data_ptr(), sol.data_ptr(), flags.data_ptr(),
             loss.data_ptr(), g_sol.data_ptr(), gx.data_ptr(), loss_hist.data_ptr() if epochs else None, _ptr(mesh_hist),
             first_tangled.data_ptr(), min_area.data_ptr(), current_stream(dev))
    if epochs:
        _watch_flags(flags)
    return DescentResult(x=x, coeffs=coeffs if epochs else None, loss_hist=loss_hist, mesh_hist=mesh_hist,
                         first_tangled=first_tangled, min_area=min_area, sol=sol if epochs else None)
