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
"""
from __future__ import annotations

import warnings
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native_fem as _nf
from ._native import NativeError, current_stream

__all__ = ['burgers_1d', 'fem_poisson_1d', 'gradient_meshpoints_1D', 'torch_FEM_Burgers_1D', 'get_Burgers_initial_coeffs',
           'burgers_project', 'fn_expansion', 'torch_FEM_1D', 'last_flags', 'GRAD_TYPES']

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


class _Batch:
    """node_off, the node cap and the packed Gaussians of one call, on the device, and the arguments every 1-D entry point of
    include/gadapt_fem.h starts with (`head`).  The pointers of its own tensors are taken once, here."""

    def __init__(self, node_counts: Sequence[int], pde_params: Optional[Sequence[dict]], device, n_fine: int = 0):
        counts = [int(n) for n in node_counts]
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
            cnt, rows = [0], []
            for p in pde_params:
                for c, s in zip(p['centers'], p['scales']):
                    rows.append([float(np.asarray(_host(c), np.float32).reshape(-1)[0]),
                                 float(np.asarray(_host(s), np.float32).reshape(-1)[0])])
                cnt.append(len(p['centers']))
            self.gptr = torch.tensor(np.cumsum(cnt), dtype=torch.int32, device=device)
            self.gpar = torch.tensor(np.asarray(rows, np.float32).reshape(-1, 2), device=device)
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
        u0c = None if u0 is None else u0.detach().float().contiguous()
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
    _require_gpu(x, 'burgers_1d')
    if x.dim() != 1:
        raise ValueError(f"burgers_1d: x must be [N] (got {tuple(x.shape)})")
    if int(n_steps) < 1:
        raise ValueError("burgers_1d: n_steps >= 1")
    n_fine = int(opt.get('num_fine_mesh_points', 0)) if (fine and u0 is None) else 0
    bt = _Batch(node_counts, pde_params if u0 is None or n_fine > 1 else None, x.device, n_fine)
    pts = _points(opt, x.device, points)
    if bc is not None:
        bc = bc.detach().to(device=x.device, dtype=torch.float32).contiguous().view(bt.B, 2)
    last, sol, fsol = _Burgers.apply(x.float(), u0, bt, _burgers_cfg(opt, n_steps), pts, bc)
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
        _watch_flags(flags)
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
    return _Poisson.apply(x.float(), bt, int(opt.get('load_quad_points', 101)), int(opt.get('stiff_quad_points', 3)), pts)


def fem_poisson_1d(x: torch.Tensor, node_counts: Sequence[int], pde_params: Sequence[dict], opt, points=None):
    """torch_FEM_1D on every mesh of x [N]: coeffs [N] (u_true at the end nodes, detached; the solve inside) and sol [B,P].
    Differentiable in x."""
    _require_gpu(x, 'fem_poisson_1d')
    if x.dim() != 1:
        raise ValueError(f"fem_poisson_1d: x must be [N] (got {tuple(x.shape)})")
    return _poisson_on(_Batch(node_counts, pde_params, x.device), x, opt, points)


# ---------------------------------------------------------------------------------------------- the reference's names
def _params_of(c_list, s_list):
    return [{'centers': [np.asarray(_host(c), np.float32).reshape(-1) for c in c_list],
             'scales': [np.asarray(_host(s), np.float32).reshape(-1) for s in s_list]}]


def torch_FEM_Burgers_1D(opt, mesh_points, quad_points, num_meshpoints, un_coeffs, BC1=None, BC2=None):
    """One Burgers step from un_coeffs on one mesh (difFEM_1d.py's signature): (unp1_coeffs, mesh_points, sol, BC1, BC2).
    Differentiable in mesh_points and un_coeffs; explicit BC1/BC2 are taken as constants."""
    _require_gpu(mesh_points, 'torch_FEM_Burgers_1D')
    n = mesh_points.shape[0]
    bc = None
    if BC1 is not None or BC2 is not None:
        b1 = un_coeffs[0] if BC1 is None else torch.as_tensor(BC1, device=mesh_points.device).reshape(-1)[0]
        b2 = un_coeffs[-1] if BC2 is None else torch.as_tensor(BC2, device=mesh_points.device).reshape(-1)[0]
        bc = torch.stack([b1.detach().float(), b2.detach().float()])
    unp1, sol, _ = burgers_1d(mesh_points, [n], None, opt, 1, points=quad_points, u0=un_coeffs.view(-1), bc=bc, fine=False)
    return unp1, mesh_points, sol.view(-1), (un_coeffs[0] if BC1 is None else BC1), (un_coeffs[-1] if BC2 is None else BC2)


def get_Burgers_initial_coeffs(fine_mesh_points, num_fine_meshpoints, mesh_points, num_meshpoints, u0, load_quad_points, opt):
    """(u0_coeffs, u0_coeffs_fine): the detached L2 projections of the initial state on the mesh (mass with eval_quad_points
    points) and on the fine mesh (10 * eval_quad_points).  u0 is the state's pde_params ({'centers', 'scales'}) or a
    (c_list, s_list) pair; it is scaled by opt['gauss_amplitude'] as the reference's u0 lambda is."""
    _require_gpu(mesh_points, 'get_Burgers_initial_coeffs')
    if isinstance(u0, dict):
        params = [u0]
    elif isinstance(u0, (list, tuple)) and len(u0) == 1 and isinstance(u0[0], dict):
        params = list(u0)
    else:
        params = _params_of(*u0)
    o = dict(opt)
    o['load_quad_points'] = int(load_quad_points)
    ev = int(opt.get('eval_quad_points', 101))
    out = []
    for pts, kp in ((mesh_points, ev), (fine_mesh_points, 10 * ev)):
        x = torch.as_tensor(pts, device=mesh_points.device).detach().float().view(-1)
        out.append(_project(x, [x.shape[0]], params, o, kp)[0])
    return out[0], out[1]


def _project(x: torch.Tensor, counts: Sequence[int], params: Sequence[dict], opt, k_proj: Optional[int]):
    """The projection-only call of gadapt_fem1d_burgers_forward: one step on one dummy point, no fine mesh, of which only u^0
    is kept.  Returns (u^0 [N], flags [B])."""
    dev = x.device
    x = x.contiguous()
    bt = _Batch(counts, params, dev)
    N = x.shape[0]
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
    _require_gpu(x, 'burgers_project')
    u0, flags = _project(x.detach().float(), counts, params, opt, k_proj)
    _watch_flags(flags)
    return u0


def fn_expansion(coeffs, mesh, quad_points, num_solpoints=None):
    """Piecewise-linear expansion of coeffs on mesh at quad_points (values only, no gradient), with the reference's
    searchsorted point location."""
    _require_gpu(mesh, 'fn_expansion')
    x = mesh.detach().float().contiguous().view(-1)
    c = torch.as_tensor(coeffs, device=x.device).detach().float().contiguous().view(-1)
    pts = _points({}, x.device, quad_points)
    bt = _Batch([x.shape[0]], None, x.device)
    sol = torch.empty(pts.numel(), device=x.device)
    _nf.call('gadapt_fem1d_expand', *bt.head(x, gauss=False), c.data_ptr(), pts.numel(), pts.data_ptr(), sol.data_ptr(),
             current_stream(x.device))
    return sol


def torch_FEM_1D(opt, mesh_points, quad_points, num_meshpoints, c_list, s_list):
    """The reference's 1-D Poisson solve on one mesh: (coeffs [N-2,1], mesh_points, sol, BC1, BC2), differentiable in
    mesh_points; BC1/BC2 are u_true at the end nodes (detached)."""
    _require_gpu(mesh_points, 'torch_FEM_1D')
    n = mesh_points.shape[0]
    coeffs, sol = fem_poisson_1d(mesh_points, [n], _params_of(c_list, s_list), opt, points=quad_points)
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
    x = x_phys.detach()
    _require_gpu(x, 'gradient_meshpoints_1D')
    x = x.float().reshape(-1)
    pp = data.pde_params
    B = int(data.__dict__.get('_num_graphs') or (len(pp) if isinstance(pp, (list, tuple)) else getattr(data, 'num_graphs', 1)))
    n = int(opt['mesh_dims'][0]) if 'mesh_dims' in opt else x.shape[0] // B
    if B * n == x.shape[0]:
        counts = [n] * B
    else:
        counts = torch.bincount(data.batch.detach().cpu(), minlength=B).tolist()
    params = _split_params(pp, B)
    x = x.requires_grad_(True)
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
    return per_mesh.detach().mean(), x.grad
