"""Differentiable 1-D P1 FEM tails of the modular loss (Burgers steps and Poisson), MI355X-native.

The reference's 1-D modular training (`src/run_GNN.py:115-120`) calls `gradient_meshpoints_1D` (firedrake_difFEM/difFEM_1d.py)
for the mesh gradient of a differentiable torch FEM computation and back-propagates `sum(x_phys * x_grads)`.  Here each
batch is one launch forward and one backward over `libgadapt_fem.so` (include/gadapt_fem.h, 1-D part): one workgroup per
mesh, the mesh's state in LDS.

    burgers_1d(x, node_counts, pde_params, opt, n_steps) -> (coeffs [N] = u^T, sol [B,P], fine_sol [B,P])
    fem_poisson_1d(x, node_counts, pde_params, opt) -> (coeffs [N], sol [B,P])
    gradient_meshpoints_1D(opt, data, x_phys) -> (loss, x_grads)
    torch_FEM_Burgers_1D, get_Burgers_initial_coeffs, fn_expansion, torch_FEM_1D: the reference's signatures on GPU tensors
    burgers_project(x, node_counts, pde_params, opt, k_proj=None) -> u^0 [N]: get_Burgers_initial_coeffs for a batch

Gradients are with respect to the node coordinates (and, for `torch_FEM_Burgers_1D`, the incoming coefficients).  The
Burgers initial projection and the Poisson boundary values are detached, as in the reference.  There is no CPU fallback.

The argument contract (`_check_batch`, called by every public entry point before anything is allocated, before the device is
looked at and before the library is loaded; tests/test_entry_contracts_host.py pins it row by row):

    lengths   x is [N] with N == sum(node_counts); node_counts is not empty and every count is at least the entry point's
              minimum (2 for the Burgers steps, the projection and `fn_expansion`, 3 for the Poisson solves);
              len(pde_params) == len(node_counts); u0, un_coeffs and coeffs hold N values; bc holds 2 per mesh; a target holds
              B * P values; there is at least one evaluation point (the kernels' loops over P = 0 points would be empty, but
              the [B, 0] result has no address to hand to the C-ABI, which refuses a null `sol`: P = 0 is refused here)
    dtypes    every tensor argument is cast to fp32 (`_f32`: any floating dtype, fp32 is passed through untouched), and the
              gradient returns in the caller's dtype; integer, bool and complex tensors are a TypeError
    layouts   any strides and storage offset: what reaches a kernel is a contiguous fp32 tensor, and x.grad has x's shape
    errors    ValueError for lengths, TypeError for dtypes, with the function's name and the two numbers that disagree; a
              well-formed call on CPU tensors is a NativeError.  More than 1024 nodes per mesh stays a NotImplementedError.
"""
from __future__ import annotations

import warnings
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native_fem as _nf
from ._native import NativeError, current_stream

__all__ = ['burgers_1d', 'fem_poisson_1d', 'gradient_meshpoints_1D', 'torch_FEM_Burgers_1D', 'get_Burgers_initial_coeffs',
           'burgers_project', 'fn_expansion', 'torch_FEM_1D', 'last_flags', 'GRAD_TYPES', 'poisson_loss_1d', 'Pde1dBatch',
           'gnn_pde_tail_1d']

GRAD_TYPES = ('PDE_loss_direct_mse', 'PDE_loss_direct_L2', 'burgers_timestep_loss_direct_mse')
MAX_NODES = 1024                      # GADAPT_FEM1D_MAX_NODES
F_NOT_INCREASING = 1                  # GADAPT_FEM1D_F_NOT_INCREASING
BURGERS_STIFF_POINTS = 3              # torch_FEM_Burgers_1D passes load_quad_points into the unused num_meshpoints slot of
                                      # build_stiffness_matrix, so its stiffness always takes the default stiff_quad_points = 3


def _require_gpu(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise NativeError(f"{what}: the 1-D FEM tail runs on the MI355X only (got a {t.device} tensor); there is no CPU fallback")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _check_float(what: str, name: str, t):
    """The 1-D dtype rule's refusing half: a tensor of a floating dtype, or TypeError."""
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: {name} must be a tensor (got {type(t).__name__})")
    if not t.dtype.is_floating_point:
        raise TypeError(f"{what}: {name} must be a floating-point tensor, which is cast to fp32 (got {t.dtype})")


def _f32(t: torch.Tensor) -> torch.Tensor:
    """The 1-D dtype rule's casting half, the one place it is done: fp32 of any floating dtype, differentiably, so that
    autograd hands the gradient back in the caller's dtype.  An fp32 tensor is returned as it is."""
    return t.float()


def _check_batch(what: str, x, node_counts: Sequence[int], pde_params: Optional[Sequence[dict]] = None, *, min_nodes: int = 2,
                 n_points: Optional[int] = None, **per_node) -> list:
    """The 1-D argument contract (module docstring), on the host alone: nothing is allocated, no device or library is touched.
    `per_node` are the tensors that hold one value per node (u0=..., un_coeffs=..., coeffs=...; None is skipped).  Returns the
    node counts as a list of ints."""
    _check_float(what, 'x', x)
    if x.dim() != 1:
        raise ValueError(f"{what}: x must be [N] (got {tuple(x.shape)})")
    counts = [int(n) for n in node_counts]
    if not counts:
        raise ValueError(f"{what}: node_counts is empty (0 meshes for {x.shape[0]} coordinates)")
    if min(counts) < min_nodes:
        raise ValueError(f"{what}: every mesh needs at least {min_nodes} nodes (got {min(counts)})")
    if x.shape[0] != sum(counts):
        raise ValueError(f"{what}: {x.shape[0]} coordinates for node_counts summing to {sum(counts)}")
    if pde_params is not None and len(pde_params) != len(counts):
        raise ValueError(f"{what}: Gaussians of {len(pde_params)} meshes for node_counts of {len(counts)} meshes")
    for name, t in per_node.items():
        if t is None:
            continue
        _check_float(what, name, t)
        if t.numel() != sum(counts):
            raise ValueError(f"{what}: {name} holds {t.numel()} values for {sum(counts)} nodes")
    if n_points is not None and n_points < 1:
        raise ValueError(f"{what}: {n_points} evaluation points; at least 1 (a [B, 0] result has no address for the kernel)")
    return counts


class _Batch:
    """node_off, the node cap and the packed Gaussians of one call, on the device, and the arguments every 1-D entry point of
    include/gadapt_fem.h starts with (`head`).  The pointers of its own tensors are taken once, here."""

    def __init__(self, node_counts: Sequence[int], pde_params: Optional[Sequence[dict]], device, n_fine: int = 0):
        counts = [int(n) for n in node_counts]
        if not counts:
            raise ValueError("1-D FEM tail: node_counts is empty")
        if pde_params is not None and len(pde_params) != len(counts):                # the kernels read gptr[b + 1] of every mesh
            raise ValueError(f"1-D FEM tail: Gaussians of {len(pde_params)} meshes for node_counts of {len(counts)} meshes")
        self.counts, self.B, self.nmax, self.n_fine = counts, len(counts), max(counts), n_fine
        self.device = device
        lib = _nf.lib()
        need = int(lib.gadapt_fem1d_lds_bytes(self.nmax, n_fine))
        budget = int(lib.gadapt_fem_lds_budget())
        if self.nmax > MAX_NODES or need > budget:
            raise NotImplementedError(f"1-D FEM tail: {self.nmax} nodes per mesh (fine mesh {n_fine}) need {need} B of LDS and "
                                      f"one lane per node; the limits are {budget} B of LDS and {MAX_NODES} nodes")
        if min(counts) < 2:
            raise ValueError(f"1-D FEM tail: every mesh needs at least 2 nodes (got {min(counts)})")
        self.node_off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=device)
        self.gptr = self.gpar = None
        if pde_params is not None:
            ptr, rows = _gaussian_rows(pde_params)
            self.gptr = torch.tensor(ptr, dtype=torch.int32, device=device)
            self.gpar = torch.tensor(rows, device=device)
        self._sizes = (self.B, self.nmax, self.node_off.data_ptr())
        self.gauss = (_ptr(self.gptr), _ptr(self.gpar))                  # (gptr, gpar), NULL without pde_params

    def head(self, x: torch.Tensor, gauss: bool = True) -> tuple:
        """n_meshes, max_nodes, node_off and x, then the Gaussians where the entry point takes them right after x
        (gadapt_fem1d_burgers_forward has u0 and bc in between and appends `gauss` itself)."""
        return self._sizes + (x.data_ptr(),) + (self.gauss if gauss else ())

    def last_index(self, T: int) -> torch.Tensor:
        """Positions of u^T in the step history ((T+1) n_b floats per mesh), built on the host."""
        off = np.concatenate([[0], np.cumsum(self.counts)])
        idx = np.concatenate([(T + 1) * o + T * n + np.arange(n) for o, n in zip(off[:-1], self.counts)])
        return torch.from_numpy(idx).to(self.device, non_blocking=True)


def _host(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else v


def _gaussian_rows(pde_params: Sequence[dict]):
    """(cumulative counts [B+1], rows [G,2] fp32 = (centre, scale)) on the host: per mesh its own number of Gaussians."""
    cnt, rows = [0], []
    for p in pde_params:
        for c, s in zip(p['centers'], p['scales']):
            rows.append([float(np.asarray(_host(c), np.float32).reshape(-1)[0]),
                         float(np.asarray(_host(s), np.float32).reshape(-1)[0])])
        cnt.append(len(p['centers']))
    return np.cumsum(cnt).astype(np.int32), np.asarray(rows, np.float32).reshape(-1, 2)


_last_flags: Optional[torch.Tensor] = None
_pending = []                         # (event, pinned flags) of earlier calls, checked without waiting


def _watch_flags(flags: torch.Tensor):
    """Keep the per-mesh flags of this call and warn, once their copy has landed, about meshes that are not increasing
    (build_stiffness_matrix's warning).  Never waits for the device."""
    global _last_flags
    _last_flags = flags
    host = torch.empty(flags.shape, dtype=flags.dtype, pin_memory=True)
    host.copy_(flags, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    _pending.append((ev, host))
    while _pending and _pending[0][0].query():
        _, h = _pending.pop(0)
        bad = (h & F_NOT_INCREASING).nonzero().flatten().tolist()
        if bad:
            warnings.warn(f"WARNING: negative diffs in build_stiffness_matrix (meshes {bad})", RuntimeWarning, stacklevel=3)
    del _pending[:-64]


def _keep_flags(flags: torch.Tensor, bt):
    """`_watch_flags`, or for a descriptor that may be launched under stream capture (`Pde1dBatch`: `watch` False) only the
    device tensor for `last_flags()`: no pinned copy and no event inside a capture."""
    global _last_flags
    if getattr(bt, 'watch', True):
        _watch_flags(flags)
    else:
        _last_flags = flags


def last_flags() -> Optional[torch.Tensor]:
    """Per-mesh flags [B] int32 of the latest forward (bit 1: some x[i+1] - x[i] < 0), on the device."""
    return _last_flags


def _points(opt, device, points=None) -> torch.Tensor:
    if points is None:
        points = torch.linspace(0, 1, int(opt.get('eval_quad_points', 101)))
    return torch.as_tensor(points).detach().to(device=device, dtype=torch.float32).contiguous().view(-1)


def _burgers_forward(bt: _Batch, x, u0, bc, cfg: dict, T: int, pts, hist, sol, fine, flags):
    """gadapt_fem1d_burgers_forward: T steps from u0 (None: from the projection of the batch's Gaussians) into hist and sol."""
    _nf.call('gadapt_fem1d_burgers_forward', *bt.head(x, gauss=False), _ptr(u0), _ptr(bc), *bt.gauss, cfg['amp'], cfg['tau'],
             cfg['taunu'], cfg['k_load'], BURGERS_STIFF_POINTS, cfg['k_proj'], cfg['k_proj_fine'], T, bt.n_fine, pts.numel(),
             pts.data_ptr(), hist.data_ptr(), sol.data_ptr(), _ptr(fine), flags.data_ptr(), current_stream(x.device))


class _Burgers(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, u0, bt: _Batch, cfg: dict, pts, bc):
        x = x.detach().contiguous()
        dev, B, P, T = x.device, bt.B, pts.numel(), cfg['T']
        N = x.shape[0]
        hist = torch.empty((T + 1) * N, device=dev)
        sol = torch.empty(B, P, device=dev)
        fine = torch.empty(B, P, device=dev) if bt.n_fine > 1 else None
        flags = torch.empty(B, dtype=torch.int32, device=dev)
        u0c = None if u0 is None else u0.detach().contiguous()
        _burgers_forward(bt, x, u0c, bc, cfg, T, pts, hist, sol, fine, flags)
        _watch_flags(flags)
        ctx.bt, ctx.cfg, ctx.has_u0 = bt, cfg, u0 is not None
        ctx.save_for_backward(x, hist, pts, bc)
        last = hist[bt.last_index(T)]                 # u^T of every mesh, concatenated
        if fine is not None:
            ctx.mark_non_differentiable(fine)
        return last, sol, fine

    @staticmethod
    def backward(ctx, g_last, g_sol, g_fine):
        x, hist, pts, bc = ctx.saved_tensors
        bt, cfg, dev = ctx.bt, ctx.cfg, x.device
        gx = torch.empty_like(x)
        gu0 = torch.empty_like(x) if ctx.has_u0 and ctx.needs_input_grad[1] else None
        g_last = None if g_last is None else g_last.contiguous().float()
        g_sol = None if g_sol is None else g_sol.contiguous().float()
        _nf.call('gadapt_fem1d_burgers_backward', *bt.head(x, gauss=False), _ptr(bc), cfg['tau'], cfg['taunu'], cfg['k_load'],
                 BURGERS_STIFF_POINTS, cfg['T'], pts.numel(), pts.data_ptr(), hist.data_ptr(), _ptr(g_sol), _ptr(g_last), gx.data_ptr(),
                 _ptr(gu0), current_stream(dev))
        return gx, gu0, None, None, None, None


def _burgers_cfg(opt, n_steps: int, k_proj: Optional[int] = None) -> dict:
    tau, nu = float(opt['tau']), float(opt['nu'])
    ev = int(opt.get('eval_quad_points', 101))
    return dict(amp=float(opt.get('gauss_amplitude', 1.0)), tau=tau, taunu=float(np.float32(tau * nu)),
                k_load=int(opt.get('load_quad_points', 101)), k_proj=int(k_proj or ev), k_proj_fine=10 * ev, T=int(n_steps))


def burgers_1d(x: torch.Tensor, node_counts: Sequence[int], pde_params: Optional[Sequence[dict]], opt, n_steps: int,
               points=None, u0: Optional[torch.Tensor] = None, bc: Optional[torch.Tensor] = None, fine: bool = True):
    """n_steps semi-implicit Burgers steps (torch_FEM_Burgers_1D) on every mesh of x [N] (concatenated, node_counts per mesh).

    u0=None starts from the detached projection of gauss_amplitude * sum exp(-(x-c)^2/s^2) of each mesh's pde_params
    (get_Burgers_initial_coeffs) and, with fine=True, runs the same steps on linspace(0, 1, num_fine_mesh_points).
    Returns coeffs [N] (u^T), sol [B,P] (u^T at the points, default linspace(0, 1, eval_quad_points)) and fine_sol [B,P]
    (or None).  Differentiable in x and u0."""
    pts = _points(opt, x.device if torch.is_tensor(x) else None, points)
    counts = _check_batch('burgers_1d', x, node_counts, pde_params, n_points=pts.numel(), u0=u0)
    if int(n_steps) < 1:
        raise ValueError("burgers_1d: n_steps >= 1")
    if u0 is None and pde_params is None:
        raise ValueError("burgers_1d: neither u0 nor pde_params: nothing to start from")
    if bc is not None:
        _check_float('burgers_1d', 'bc', bc)
        if bc.numel() != 2 * len(counts):
            raise ValueError(f"burgers_1d: bc holds {bc.numel()} values for {len(counts)} meshes (2 per mesh)")
    _require_gpu(x, 'burgers_1d')
    n_fine = int(opt.get('num_fine_mesh_points', 0)) if (fine and u0 is None) else 0
    bt = _Batch(counts, pde_params if u0 is None or n_fine > 1 else None, x.device, n_fine)
    if bc is not None:
        bc = _f32(bc.detach()).to(device=x.device).reshape(bt.B, 2).contiguous()
    if u0 is not None:
        u0 = _f32(u0).reshape(-1)
    last, sol, fsol = _Burgers.apply(_f32(x), u0, bt, _burgers_cfg(opt, n_steps), pts, bc)
    return last, sol, fsol


class _Poisson(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bt: _Batch, k_load, k_stiff, pts):
        x = x.detach().contiguous()
        dev, B, P = x.device, bt.B, pts.numel()
        coeffs = torch.empty_like(x)
        sol = torch.empty(B, P, device=dev)
        flags = torch.empty(B, dtype=torch.int32, device=dev)
        _nf.call('gadapt_fem1d_poisson_forward', *bt.head(x), k_load, k_stiff, P, pts.data_ptr(), coeffs.data_ptr(), sol.data_ptr(),
                 flags.data_ptr(), current_stream(dev))
        _keep_flags(flags, bt)
        ctx.bt, ctx.k = bt, (k_load, k_stiff)
        ctx.save_for_backward(x, pts, coeffs)
        return coeffs, sol

    @staticmethod
    def backward(ctx, g_coeffs, g_sol):
        x, pts, coeffs = ctx.saved_tensors
        bt = ctx.bt
        gx = torch.empty_like(x)
        g_coeffs = None if g_coeffs is None else g_coeffs.contiguous().float()
        g_sol = None if g_sol is None else g_sol.contiguous().float()
        _nf.call('gadapt_fem1d_poisson_backward', *bt.head(x), ctx.k[0], ctx.k[1], pts.numel(), pts.data_ptr(), coeffs.data_ptr(),
                 _ptr(g_coeffs), _ptr(g_sol), gx.data_ptr(), current_stream(x.device))
        return gx, None, None, None, None


def _poisson_on(bt: _Batch, x: torch.Tensor, opt, points=None):
    """fem_poisson_1d on a built batch (one with Gaussians)."""
    if min(bt.counts) < 3:
        raise ValueError("fem_poisson_1d: every mesh needs at least 3 nodes")
    pts = _points(opt, x.device, points)
    return _Poisson.apply(_f32(x), bt, int(opt.get('load_quad_points', 101)), int(opt.get('stiff_quad_points', 3)), pts)


def fem_poisson_1d(x: torch.Tensor, node_counts: Sequence[int], pde_params: Sequence[dict], opt, points=None):
    """torch_FEM_1D on every mesh of x [N]: coeffs [N] (u_true at the end nodes, detached; the solve inside) and sol [B,P].
    Differentiable in x.  At least one evaluation point: P = 0 is refused (module docstring)."""
    counts = _check_batch('fem_poisson_1d', x, node_counts, pde_params, min_nodes=3, n_points=_points(opt, None, points).numel())
    _require_gpu(x, 'fem_poisson_1d')
    return _poisson_on(_Batch(counts, pde_params, x.device), x, opt, points)


# ---------------------------------------------------------------------------------------------- the 1-D pde_loss tail
LOSS_KINDS = {'l1': _nf.FEM1D_LOSS_L1, 'mse': _nf.FEM1D_LOSS_MSE}
_tickets = {}                         # (device, stream) -> the launch's ticket counter [1] int32, zero between launches


def _check_loss_size(nmax: int, n_pts: int):
    need, budget = int(_nf.lib().gadapt_fem_poisson1d_loss_lds_bytes(nmax, n_pts)), int(_nf.lib().gadapt_fem_lds_budget())
    if need > budget:
        raise NotImplementedError(f"fused 1-D Poisson tail: {nmax} nodes per mesh and {n_pts} evaluation points need {need} B of LDS "
                                  f"(64 per node and the seed row), the budget is {budget} B; the split tail takes up to {MAX_NODES} nodes")


class _PoissonLoss(torch.autograd.Function):
    """gadapt_fem_poisson1d_loss: solve, loss and node gradient in one launch; backward is g * gx."""

    @staticmethod
    def forward(ctx, x, bt, k_load, k_stiff, pts, target, kind):
        x = x.detach().contiguous()
        dev, B, P = x.device, bt.B, pts.numel()
        coeffs, gx = torch.empty_like(x), torch.empty_like(x)
        sol = torch.empty(B * P, device=dev)
        flags = torch.empty(B, dtype=torch.int32, device=dev)
        partials, loss = torch.empty(B, device=dev), torch.empty((), device=dev)
        key = (dev, torch.cuda.current_stream(dev).cuda_stream)
        ticket = _tickets.get(key)
        if ticket is None:
            ticket = _tickets[key] = torch.zeros(1, dtype=torch.int32, device=dev)
        _nf.call('gadapt_fem_poisson1d_loss', *bt.head(x), k_load, k_stiff, P, pts.data_ptr(), target.data_ptr(), kind, coeffs.data_ptr(),
                 sol.data_ptr(), gx.data_ptr(), flags.data_ptr(), partials.data_ptr(), loss.data_ptr(), ticket.data_ptr(),
                 current_stream(dev))
        _keep_flags(flags, bt)
        ctx.save_for_backward(gx)
        ctx.mark_non_differentiable(coeffs, sol, partials)
        return loss, coeffs, sol, partials

    @staticmethod
    def backward(ctx, g, *_):
        (gx,) = ctx.saved_tensors
        from .functional import _unit_grads
        unit = _unit_grads.get(g.device)
        if unit is not None and g.data_ptr() == unit.data_ptr():
            return (gx,) + (None,) * 6           # the caller passed unit_gradient(): nothing to multiply
        return (gx * g,) + (None,) * 6


def _poisson_loss_on(bt, x: torch.Tensor, target: torch.Tensor, k_load: int, k_stiff: int, pts: torch.Tensor, loss: str):
    if loss not in LOSS_KINDS:
        raise ValueError(f"fused 1-D Poisson tail: loss must be one of {sorted(LOSS_KINDS)} (got {loss!r})")
    if min(bt.counts) < 3:
        raise ValueError("poisson_loss_1d: every mesh needs at least 3 nodes")
    _check_target('poisson_loss_1d', target, bt.B, pts.numel())
    _require_gpu(x, 'poisson_loss_1d')
    target = _f32(target.detach()).to(device=x.device).reshape(-1).contiguous()
    _check_loss_size(bt.nmax, pts.numel())
    return _PoissonLoss.apply(_f32(x), bt, k_load, k_stiff, pts, target, LOSS_KINDS[loss])


def _check_target(what: str, target, B: int, P: int):
    _check_float(what, 'target', target)
    if target.numel() != B * P:
        raise ValueError(f"{what}: target of {target.numel()} values for {B} meshes x {P} evaluation points")


def poisson_loss_1d(x: torch.Tensor, node_counts: Sequence[int], pde_params: Sequence[dict], target: torch.Tensor, opt, loss: str = 'l1',
                    points=None):
    """`fem_poisson_1d`, the package's `l1_loss` / `mse_loss` of sol [B*P,1] against `target` [B*P] and that loss's backward
    through the solve, in ONE launch (gadapt_fem_poisson1d_loss): (loss, coeffs [N], sol [B*P]).  `loss` is differentiable in x
    (its backward is g * gx, gx written by the same launch); coeffs and sol are detached, with the bits of `fem_poisson_1d`, and
    x.grad has the bits of the three launches.  The seed row shares the LDS with the solve: 1017 nodes per mesh at 101 points."""
    pts = _points(opt, x.device if torch.is_tensor(x) else None, points)
    counts = _check_batch('poisson_loss_1d', x, node_counts, pde_params, min_nodes=3, n_points=pts.numel())
    if loss not in LOSS_KINDS:
        raise ValueError(f"fused 1-D Poisson tail: loss must be one of {sorted(LOSS_KINDS)} (got {loss!r})")
    _check_target('poisson_loss_1d', target, len(counts), pts.numel())
    _require_gpu(x, 'poisson_loss_1d')
    out = _poisson_loss_on(_Batch(counts, pde_params, x.device), x, target, int(opt.get('load_quad_points', 101)),
                           int(opt.get('stiff_quad_points', 3)), pts, loss)
    return out[0], out[1], out[2]


class Pde1dBatch:
    """The 1-D pde_loss tail of ONE batch shape, ready to launch (what `fem.PdeBatch` is in 2-D): the node counts, `node_off`, the
    evaluation points and the quadrature counts, and the Gaussians' device buffers `gptr` [B+1] int32 and `gpar` [cap,2] fp32
    (centre, scale) with a pinned host copy to stage them in.  `solve` / `solve_loss` are `fem_poisson_1d` / `poisson_loss_1d`
    without their per-call host work, so they can be stream-captured: the flags stay on the device (`last_flags()`), no pinned
    copy and no event.  `set_params` feeds another batch's Gaussians into the SAME device buffers."""

    watch = False                     # `_keep_flags`: never `_watch_flags` (a pinned copy and an event) from a descriptor's launch
    # (target field, 'l1' | 'mse'), set by training.GraphedTrainStep for opt['fem1d_tail'] = 'fused': `gnn_pde_tail_1d` then takes
    # `solve_loss` against that field of the batch and leaves the loss in `loss`
    fused = None
    loss = None

    def __init__(self, node_counts: Sequence[int], points: torch.Tensor, cap: int, device='cpu', k_load: int = 101, k_stiff: int = 3):
        counts = [int(n) for n in node_counts]
        if not counts or min(counts) < 3:
            raise ValueError("Pde1dBatch: every mesh needs at least 3 nodes")
        if max(counts) > MAX_NODES:
            raise NotImplementedError(f"Pde1dBatch: {max(counts)} nodes per mesh; the limit is {MAX_NODES} (one lane per node)")
        if int(cap) < 1:
            raise ValueError(f"Pde1dBatch: room for {cap} Gaussians")
        dev = torch.device(device)
        self.counts, self.B, self.nmax, self.cap, self.device = counts, len(counts), max(counts), int(cap), dev
        self.n_meshes, self.n_nodes = self.B, sum(counts)
        self.k_load, self.k_stiff = int(k_load), int(k_stiff)
        self.node_off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=dev)
        self.pts = _points({}, dev, points)
        self.gptr = torch.zeros(self.B + 1, dtype=torch.int32, device=dev)
        self.gpar = torch.zeros(self.cap, 2, dtype=torch.float32, device=dev)
        pin = dev.type == 'cuda'
        self.host_gptr = torch.zeros(self.B + 1, dtype=torch.int32, pin_memory=pin)
        self.host_gpar = torch.zeros(self.cap, 2, dtype=torch.float32, pin_memory=pin)
        self._staged = torch.cuda.Event() if pin else None       # recorded behind the copies out of the staging buffers
        self._sizes = (self.B, self.nmax, self.node_off.data_ptr())
        self.gauss = (self.gptr.data_ptr(), self.gpar.data_ptr())
        self.interior = _interior_index(counts, dev)             # positions of the coefficients GNN.forward returns

    def head(self, x: torch.Tensor, gauss: bool = True) -> tuple:
        return self._sizes + (x.data_ptr(),) + (self.gauss if gauss else ())

    @classmethod
    def from_data(cls, model, data, max_gauss: int = 8) -> 'Pde1dBatch':
        """The descriptor of `data`'s node counts for `model`'s tail (its evaluation points and quadrature), with room for
        `max_gauss` Gaussians per mesh; the batch's own Gaussians are set if it carries any.  May synchronise, once."""
        from .fem import _batch_counts, _check_tail, batch_params
        _check_tail(model)
        o = model.opt
        B, counts = _batch_counts(data, data.x_comp)
        pb = cls(counts, model.quad_points, B * int(max_gauss), torch.device(o['device']), int(o.get('load_quad_points', 101)),
                 int(o.get('stiff_quad_points', 3)))
        try:
            params = batch_params(o, data, B)
        except (AttributeError, KeyError):
            params = None
        if params is not None:
            pb.set_params(params)
        return pb

    def set_params(self, pde_params: Sequence[dict]):
        """The Gaussians of the next solve: packed into the pinned buffers, then one non-blocking copy each into `gptr` and `gpar`
        on the current stream (rows past the last Gaussian keep what they held; nothing reads them)."""
        if len(pde_params) != self.B:
            raise ValueError(f"PdeBatch: Gaussians of {len(pde_params)} meshes for a batch of {self.B}")
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

    def _x(self, x_phys: torch.Tensor) -> torch.Tensor:
        _check_float('Pde1dBatch', 'x_phys', x_phys)
        if x_phys.numel() != self.n_nodes:
            raise ValueError(f"Pde1dBatch: x_phys {tuple(x_phys.shape)} for a batch of {self.n_nodes} nodes in 1-D")
        _require_gpu(x_phys, 'Pde1dBatch')
        return _f32(x_phys.reshape(-1))

    def solve(self, x_phys: torch.Tensor):
        """(coeffs [N], sol [B*P]) of `fem_poisson_1d` on these node counts and the Gaussians last set: the same entry point on
        the same inputs, the same bits."""
        coeffs, sol = _Poisson.apply(self._x(x_phys), self, self.k_load, self.k_stiff, self.pts)
        return coeffs, sol.view(-1)

    def solve_loss(self, x_phys: torch.Tensor, target: torch.Tensor, loss: str = 'l1'):
        """(loss, coeffs [N], sol [B*P]) of `poisson_loss_1d`: the one-launch tail."""
        _check_target('Pde1dBatch.solve_loss', target, self.B, self.pts.numel())
        out = _poisson_loss_on(self, self._x(x_phys), target, self.k_load, self.k_stiff, self.pts, loss)
        return out[0], out[1], out[2]


def _interior_index(counts: Sequence[int], device) -> torch.Tensor:
    """Positions of the interior nodes (1..n_b-2 of every mesh) in the concatenated batch."""
    off = np.concatenate([[0], np.cumsum(counts)])
    return torch.from_numpy(np.concatenate([o + np.arange(1, n - 1) for o, n in zip(off[:-1], counts)])).to(device, non_blocking=True)


def gnn_pde_tail_1d(model, data, x_phys: torch.Tensor):
    """`GNN.forward`'s pde_loss branch in 1-D (`src/GNN.py:319-325,338-342`): torch_FEM_1D per mesh, as one launch for the batch.
    (coeffs [sum(n_b - 2), 1], the interior coefficients; x_phys [N]; sol [B*P]).  A batch that carries a `Pde1dBatch`
    (`data._pde_batch`) is solved through it: the launch alone, nothing read back from the device or sent to it."""
    from .fem import _batch_counts, batch_params
    x = x_phys.reshape(-1)
    pb = getattr(data, '_pde_batch', None)
    if pb is not None:
        if pb.fused is not None:
            pb.loss, coeffs, sol = pb.solve_loss(x, getattr(data, pb.fused[0]), pb.fused[1])
        else:
            coeffs, sol = pb.solve(x)
        return coeffs[pb.interior].unsqueeze(1), x, sol
    B, counts = _batch_counts(data, x)
    params = batch_params(model.opt, data, B)
    _check_batch('gnn_pde_tail_1d', x, counts, params, min_nodes=3)
    coeffs, sol = _poisson_on(_Batch(counts, params, x.device), x, model.opt, model.quad_points)
    return coeffs[_interior_index(counts, x.device)].unsqueeze(1), x, sol.view(-1)


# ---------------------------------------------------------------------------------------------- the reference's names
def _params_of(c_list, s_list):
    return [{'centers': [np.asarray(_host(c), np.float32).reshape(-1) for c in c_list],
             'scales': [np.asarray(_host(s), np.float32).reshape(-1) for s in s_list]}]


def torch_FEM_Burgers_1D(opt, mesh_points, quad_points, num_meshpoints, un_coeffs, BC1=None, BC2=None):
    """One Burgers step from un_coeffs on one mesh (difFEM_1d.py's signature): (unp1_coeffs, mesh_points, sol, BC1, BC2).
    Differentiable in mesh_points and un_coeffs; explicit BC1/BC2 are taken as constants."""
    _check_float('torch_FEM_Burgers_1D', 'un_coeffs', un_coeffs)
    n = _check_batch('torch_FEM_Burgers_1D', mesh_points, [mesh_points.shape[0]] if torch.is_tensor(mesh_points) else [],
                     n_points=_points(opt, None, quad_points).numel(), un_coeffs=un_coeffs)[0]
    _require_gpu(mesh_points, 'torch_FEM_Burgers_1D')
    bc = None
    if BC1 is not None or BC2 is not None:
        b1 = un_coeffs[0] if BC1 is None else torch.as_tensor(BC1, device=mesh_points.device).reshape(-1)[0]
        b2 = un_coeffs[-1] if BC2 is None else torch.as_tensor(BC2, device=mesh_points.device).reshape(-1)[0]
        bc = torch.stack([b1.detach().float(), b2.detach().float()])
    unp1, sol, _ = burgers_1d(mesh_points, [n], None, opt, 1, points=quad_points, u0=un_coeffs.reshape(-1), bc=bc, fine=False)
    return unp1, mesh_points, sol.view(-1), (un_coeffs[0] if BC1 is None else BC1), (un_coeffs[-1] if BC2 is None else BC2)


def get_Burgers_initial_coeffs(fine_mesh_points, num_fine_meshpoints, mesh_points, num_meshpoints, u0, load_quad_points, opt):
    """(u0_coeffs, u0_coeffs_fine): the detached L2 projections of the initial state on the mesh (mass with eval_quad_points
    points) and on the fine mesh (10 * eval_quad_points).  u0 is the state's pde_params ({'centers', 'scales'}) or a
    (c_list, s_list) pair; it is scaled by opt['gauss_amplitude'] as the reference's u0 lambda is."""
    if isinstance(u0, dict):
        params = [u0]
    elif isinstance(u0, (list, tuple)) and len(u0) == 1 and isinstance(u0[0], dict):
        params = list(u0)
    else:
        params = _params_of(*u0)
    meshes = []
    for name, pts in (('mesh_points', mesh_points), ('fine_mesh_points', fine_mesh_points)):
        what = f'get_Burgers_initial_coeffs ({name})'
        pts = torch.as_tensor(pts)
        _check_float(what, name, pts)
        x = pts.detach().reshape(-1)
        _check_batch(what, x, [x.shape[0]], params)
        meshes.append(x)
    _require_gpu(mesh_points, 'get_Burgers_initial_coeffs')
    o = dict(opt)
    o['load_quad_points'] = int(load_quad_points)
    ev = int(opt.get('eval_quad_points', 101))
    out = []
    for x, kp in zip(meshes, (ev, 10 * ev)):
        x = _f32(x).to(mesh_points.device)
        out.append(_project(x, [x.shape[0]], params, o, kp)[0])
    return out[0], out[1]


def _project(x: torch.Tensor, counts: Sequence[int], params: Sequence[dict], opt, k_proj: Optional[int]):
    """The projection-only call of gadapt_fem1d_burgers_forward: one step on one dummy point, no fine mesh, of which only u^0
    is kept.  Returns (u^0 [N], flags [B])."""
    dev = x.device
    x = x.contiguous()
    bt = _Batch(counts, params, dev)
    N = x.shape[0]
    if x.dim() != 1 or N != sum(bt.counts):
        raise ValueError(f"1-D Burgers projection: x {tuple(x.shape)} for node_counts summing to {sum(bt.counts)}")
    hist, sol = torch.empty(2 * N, device=dev), torch.empty(bt.B, 1, device=dev)
    flags, p1 = torch.empty(bt.B, dtype=torch.int32, device=dev), torch.zeros(1, device=dev)
    _burgers_forward(bt, x, None, None, _burgers_cfg(opt, 1, k_proj=k_proj), 1, p1, hist, sol, None, flags)
    off = np.concatenate([[0], np.cumsum(bt.counts)])
    idx = np.concatenate([2 * o + np.arange(n) for o, n in zip(off[:-1], bt.counts)])       # u^0 of the (u^0, u^1) history
    return hist[torch.from_numpy(idx).to(dev, non_blocking=True)], flags


def burgers_project(x: torch.Tensor, counts: Sequence[int], params: Sequence[dict], opt, k_proj: Optional[int] = None) -> torch.Tensor:
    """`get_Burgers_initial_coeffs` for a batch of meshes in one launch: the L2 projection of
    gauss_amplitude * sum exp(-(x-c)^2/s^2) of each mesh's own Gaussians on its mesh, [N] concatenated.  The mass matrix
    takes `k_proj` points per interval (eval_quad_points, as for a coarse mesh, unless given; the reference's fine mesh takes
    10 * eval_quad_points)."""
    counts = _check_batch('burgers_project', x, counts, params)
    _require_gpu(x, 'burgers_project')
    u0, flags = _project(_f32(x.detach()), counts, params, opt, k_proj)
    _watch_flags(flags)
    return u0


def fn_expansion(coeffs, mesh, quad_points, num_solpoints=None):
    """Piecewise-linear expansion of coeffs on mesh at quad_points (values only, no gradient), with the reference's
    searchsorted point location."""
    _check_float('fn_expansion', 'mesh', mesh)
    coeffs = torch.as_tensor(coeffs)
    pts = _points({}, mesh.device, quad_points)
    _check_batch('fn_expansion', mesh.reshape(-1), [mesh.numel()], n_points=pts.numel(), coeffs=coeffs)
    _require_gpu(mesh, 'fn_expansion')
    x = _f32(mesh.detach()).reshape(-1).contiguous()
    c = _f32(coeffs.detach()).to(x.device).reshape(-1).contiguous()
    bt = _Batch([x.shape[0]], None, x.device)
    sol = torch.empty(pts.numel(), device=x.device)
    _nf.call('gadapt_fem1d_expand', *bt.head(x, gauss=False), c.data_ptr(), pts.numel(), pts.data_ptr(), sol.data_ptr(),
             current_stream(x.device))
    return sol


def torch_FEM_1D(opt, mesh_points, quad_points, num_meshpoints, c_list, s_list):
    """The reference's 1-D Poisson solve on one mesh: (coeffs [N-2,1], mesh_points, sol, BC1, BC2), differentiable in
    mesh_points; BC1/BC2 are u_true at the end nodes (detached)."""
    params = _params_of(c_list, s_list)
    n = _check_batch('torch_FEM_1D', mesh_points, [mesh_points.shape[0]] if torch.is_tensor(mesh_points) else [], params, min_nodes=3,
                     n_points=_points(opt, None, quad_points).numel())[0]
    _require_gpu(mesh_points, 'torch_FEM_1D')
    coeffs, sol = fem_poisson_1d(mesh_points, [n], params, opt, points=quad_points)
    return coeffs[1:-1].unsqueeze(1), mesh_points, sol.view(-1), coeffs[:1].detach(), coeffs[-1:].detach()


# ------------------------------------------------------------------------------------------------ the modular loss
def _split_params(pde_params, B: int):
    if isinstance(pde_params, (list, tuple)):
        return list(pde_params)
    cs, ss = pde_params['centers'], pde_params['scales']
    if B > 1 or (len(cs) and isinstance(cs[0], (list, tuple))):   # PyG-batched dict: one list of Gaussians per mesh
        return [{'centers': cs[b], 'scales': ss[b]} for b in range(B)]
    return [pde_params]


def _gauss_on(points: torch.Tensor, bt: _Batch) -> torch.Tensor:
    """u_true [B,P] = sum_g exp(-(p-c)^2/s^2) per mesh, on the device."""
    c, s = bt.gpar[:, 0], bt.gpar[:, 1]
    e = torch.exp(-(points[None, :] - c[:, None]) ** 2 / s[:, None] ** 2)        # [G,P]
    seg = torch.repeat_interleave(torch.arange(bt.B, device=points.device),
                                  (bt.gptr[1:] - bt.gptr[:-1]).long(), output_size=e.shape[0])
    return torch.zeros(bt.B, points.numel(), device=points.device).index_add_(0, seg, e)


def gradient_meshpoints_1D(opt, data, x_phys):
    """(loss, x_grads) of the reference's modular 1-D loss for a batch: x_grads on a node is the gradient of its own mesh's
    loss, loss is the mean over meshes.  Nothing waits for the device."""
    if 'grad_type' not in opt:
        raise ValueError("Error: opt['grad_type'] not specified")
    gt = opt['grad_type']
    if gt not in GRAD_TYPES:
        raise ValueError("Error: opt['grad_type'] incorrectly specified")
    _check_float('gradient_meshpoints_1D', 'x_phys', x_phys)
    x = x_phys.detach().reshape(-1)
    pp = data.pde_params
    B = int(data.__dict__.get('_num_graphs') or (len(pp) if isinstance(pp, (list, tuple)) else getattr(data, 'num_graphs', 1)))
    n = int(opt['mesh_dims'][0]) if 'mesh_dims' in opt else x.shape[0] // B
    if B * n == x.shape[0]:
        counts = [n] * B
    elif getattr(data, 'batch', None) is not None:
        counts = torch.bincount(data.batch.detach().cpu(), minlength=B).tolist()
    else:
        raise ValueError(f"gradient_meshpoints_1D: {x.shape[0]} coordinates for {B} meshes of {n} nodes, and the batch carries no "
                         "`batch` vector to count them by")
    params = _split_params(pp, B)
    counts = _check_batch('gradient_meshpoints_1D', x, counts, params, min_nodes=2 if gt == 'burgers_timestep_loss_direct_mse' else 3)
    _require_gpu(x, 'gradient_meshpoints_1D')
    x = _f32(x).requires_grad_(True)
    pts = _points(opt, x.device)
    with torch.enable_grad():
        if gt == 'burgers_timestep_loss_direct_mse':
            _, sol, fine = burgers_1d(x, counts, params, opt, int(opt['num_time_steps']), points=pts)
            per_mesh = ((sol - fine) ** 2).mean(1)
        else:
            bt = _Batch(counts, params, x.device)
            _, sol = _poisson_on(bt, x, opt, pts)
            err = sol - _gauss_on(pts, bt)
            if gt == 'PDE_loss_direct_mse':
                per_mesh = (err ** 2).mean(1)
            else:
                per_mesh = torch.trapezoid(err.abs() ** 2, pts, dim=1)
        per_mesh.sum().backward()
    return per_mesh.detach().mean(), x.grad.to(x_phys.dtype)                      # the gradient in the caller's dtype
