"""Monge-Ampere target meshes on the GPU: the reference's default 2-D target (`classical_meshing/ma_mesh_2d.py:163-295`,
`src/data.py:208-210`, `mesh_type = 'ma'`), batched.

The reference hands the problem to Firedrake and `movement.MongeAmpereMover`.  Neither runs here, so its finite-element
discretisation is not reproduced and PARITY WITH `movement` IS NOT PINNED.  What it solves is: a convex potential phi on the
computational square with

    x = xi + grad phi,    m(x) det(I + H phi) = theta,    grad phi . n = 0,

and this module relaxes that equation by finite differences in pseudo-time (`include/gadapt_mesh.h` has the iteration operation
for operation): phi += cfl h^2 min(1, lambda_min) (r - mean r) with r = log(m det), until max |r - mean r| <= tol.  The
monitor is evaluated at the moving coordinates, from the sample's Gaussians, inside the kernel.  Its yardsticks are its own
fp64 restatement (`tests/ma_restatement.py`) and the equidistribution it has to achieve, not the reference's meshes.

`ma_batch` is the batched form: one launch of `libgadapt_mesh.so`, one workgroup per mesh, each to its own stopping step.
`MA2d` and `deform_mesh_ma2d` keep the reference's names, argument lists and return tuples.  2-D only (the reference has no
1-D MA), 3 <= N <= 32 a side, at most 8 Gaussians; anything else raises `ValueError`.  The iteration runs on the GPU only:
`NativeError` without one.

Two monitors, chosen per call from `pde_params[b].get('mesh_type', 'ma')`; all meshes of one call share one (one launch per call).
`'ma'` is `monitor_ma`.  `'M2N'` is the reference's M2N branch of `MA2d` (`ma_mesh_2d.py:178-278`) with `fast_M2N_monitor =
'fast'`, the value the reference's run parameters select for M2N: `monitor_m2n`, mon_reg + beta F / max F with
F = sqrt(u_xx^2 + 2 u_xy^2 + u_yy^2) and the maximum over the mesh's CURRENT nodes, reduced inside the kernel at every update
(`ma_m2n_kernel`, `ma_m2n_strided_kernel`).  u_xy IS THE LAST GAUSSIAN'S ONLY: the reference assigns it with `=` inside its loop
(`ma_mesh_2d.py:133,151`), and that is kept.  `mon_reg` is required and > 0, `M2N_beta` defaults to 1.5 and is >= 0; `mon_power`
and `M2N_alpha` are accepted and ignored, as that branch of the reference does not read them.  'slow' and 'superslow' add
alpha |u_h - u|^2 / max from a Poisson solve on the moving mesh at every monitor evaluation.  'slow' IS OPT-IN: it raises
`NotImplementedError` unless the call passes `m2n_solve='p1'`, which runs `ma_m2n_slow_kernel` (`monitor_m2n_slow` is its readable
statement): the P1 solve with nodal forcing and nodal boundary values inside the update loop, a banded Cholesky in LDS, lane
route only, 3 <= N <= 24 (`SLOW_MAX_SIDE`), `M2N_alpha` and `M2N_beta` both defaulting to 1.0, result `MASlowResult` with the
last monitor.  The reference L2-projects f and u into P1 and solves with Firedrake; that is not reproduced.  'superslow'
(it differentiates a high-order solution) IS NOT BUILT.  Parity with `movement` is unpinned for M2N as for 'ma'; the yardsticks
are `tests/ma_m2n_restatement.py` and `tests/ma_m2n_slow_restatement.py`.
A contrast of mon_reg against beta that is too strong for the mesh loses convexity at the first update and comes back as
NONCONVEX, which means "lower `cfl`": two Gaussians drawn with seed 15 on 15 x 15 with mon_reg = 0.01, beta = 1.0 and
cfl = 0.2 do (min lambda -0.18, in fp32 and fp64 alike).

Two routes (`ROUTES`).  `route='lane'`, the default, holds one node per lane and phi in fp32: 3 <= N <= 32.  Its residual floor
reaches `tol` near 64 x 64 (at 81 x 81 the fp32 restatement stops 12 % late), so sides above 32 are not the same kernel with
more nodes: `route='strided'` (`ma_batch`, `attach_ma_targets` and through it the datasets' `target_params['solver']`) holds
K = ceil(N^2 / 1024) <= 7 nodes per lane and phi in fp64, 3 <= N <= 81, everything after the five stencil expressions in the
lane route's fp32.  THE TWO ROUTES DO NOT SHARE BITS at N <= 32: phi is fp64 on one and fp32 on the other; each is within its
own noise bar of the fp64 restatement.  Nothing changes its route unasked; `MA2d` and `deform_mesh_ma2d` stay on 'lane'.
The defaults `cfl=0.2, tol=1e-4, max_steps=20000` hold on both routes: 64 x 64 wanted 17 500 to 25 500 updates in the cases
tried and 81 x 81 28 000 to 32 000, so large meshes need `max_steps` raised (40 000 covered both), and the default call can
return CAP there.

A TABULATED MONITOR (`ma_table_batch`, `ma_table_kernel` and `ma_table_strided_kernel`): the same iteration on both routes with
the monitor read bilinearly from a table M [T, T] on a lattice of the physical unit square, M[i, j] at (i / (T-1), j / (T-1)),
2 <= T <= 1024, each mesh its own T, instead of from the Gaussians.  `monitor_table` tabulates a closed-form monitor,
`monitor_from_nodal` builds the `diag_hessian_ma` monitor from the second differences of ANY nodal field on a uniform lattice,
and `attach_ma_targets(..., {'monitor_source': 'uu'})` (the datasets' `target_params`) drives every sample's mesh by its own
`uu_tensor`: the classical competitor that knows the computed coarse solution, not the exact one.  The reference approximates
that with a high-order Firedrake solve ('superslow', `ma_mesh_2d.py:182-225`), which is not built; a second difference of the
coarse P1 solution is the STATED DEVIATION, and parity with `movement` is unpinned here as for the other monitors.  The table
does not move with the mesh, so `mesh_type: 'M2N'` (whose maximum does) is refused under `monitor_source: 'uu'`.
"""
from __future__ import annotations

import ctypes as C
import time
import warnings
from collections import namedtuple
from typing import Optional, Sequence

import torch

from . import _native_mesh
from ._native import NativeError, current_stream
from .mmpde5 import _gauss_dd, unit_grid, warn_unconverged, write_back_to_nodes

CONVERGED, CAP, NONCONVEX = _native_mesh.MA_CONVERGED, _native_mesh.MA_CAP, _native_mesh.MA_NONCONVEX
STATUS_NAMES = {CONVERGED: 'converged', CAP: 'cap reached', NONCONVEX: 'convexity lost'}
MAX_SIDE, MAX_GAUSS = _native_mesh.MA_MAX_SIDE, _native_mesh.MA_MAX_GAUSS
STRIDED_MAX_SIDE = _native_mesh.MA_STRIDED_MAX_SIDE
SLOW_MAX_SIDE = _native_mesh.MA_M2N_SLOW_MAX_SIDE
TABLE_MAX_SIDE = _native_mesh.MA_TABLE_MAX_SIDE
ROUTES = ('lane', 'strided')
MONITOR_SOURCES = ('analytic', 'uu')
M2N_SOLVES = ('p1',)

MAResult = namedtuple('MAResult', 'coords steps residual status')
MASlowResult = namedtuple('MASlowResult', 'coords steps residual status monitor')


def monitor_constants(params):
    """(mon_reg, mon_power) of `MA2d`'s monitor (`ma_mesh_2d.py:172-176`): with 'mon_power' the pair given ('mon_reg' is then
    required, as in the reference, where its absence is a KeyError), else (1, 0.2)."""
    if 'mon_power' in params:
        if 'mon_reg' not in params:
            raise ValueError("the Monge-Ampere monitor reads 'mon_reg' whenever 'mon_power' is given: pass both or neither")
        return float(params['mon_reg']), float(params['mon_power'])
    return 1.0, 0.2


def monitor_ma(x: torch.Tensor, y: torch.Tensor, params) -> torch.Tensor:
    """`MA2d`'s monitor: (mon_reg + sqrt(u_xx^2 + u_yy^2))^mon_power, or (1 + sqrt(...))^0.2 without 'mon_power', where u_xx and
    u_yy are the SIGNED sums over the Gaussians (`diag_hessian_ma`), not `monitor_2d`'s per-Gaussian absolute values."""
    reg, power = monitor_constants(params)
    uxx, uyy = torch.zeros_like(x), torch.zeros_like(x)
    for c, s in zip(params['centers'], params['scales']):
        c0, c1, s0, s1 = float(c[0]), float(c[1]), float(s[0]), float(s[1])
        g = torch.exp(-(x - c0) ** 2 / s0 ** 2 - (y - c1) ** 2 / s1 ** 2)
        uxx = uxx + _gauss_dd(x, c0, s0) * g
        uyy = uyy + _gauss_dd(y, c1, s1) * g
    return (reg + torch.sqrt(uxx ** 2 + uyy ** 2)) ** power


MONITORS = ('ma', 'M2N')


def monitor_kind(b: int, params, m2n_solve: Optional[str] = None) -> str:
    """'ma', 'M2N' or 'M2N slow' from `params.get('mesh_type', 'ma')`, with the checks of the M2N branch of the reference's `MA2d`.
    'M2N slow' is `fast_M2N_monitor = 'slow'` under `m2n_solve='p1'`; without that keyword 'slow' is refused as before."""
    if m2n_solve is not None and m2n_solve not in M2N_SOLVES:
        raise ValueError(f"m2n_solve = {m2n_solve!r}; None or one of {M2N_SOLVES}")
    kind = params.get('mesh_type', 'ma')
    if kind not in MONITORS:
        raise ValueError(f"mesh {b}: mesh_type = {kind!r}; one of {MONITORS}")
    if kind == 'M2N':
        fast = params.get('fast_M2N_monitor')
        if fast == 'slow' and m2n_solve == 'p1':
            return 'M2N slow'
        if fast == 'superslow':
            raise NotImplementedError(f"mesh {b}: fast_M2N_monitor = 'superslow' differentiates a high-order FEM solution on the moving "
                                      "mesh at every monitor evaluation, which is not built; 'fast' is, and 'slow' with m2n_solve='p1'")
        if fast == 'slow':
            raise NotImplementedError(f"mesh {b}: fast_M2N_monitor = 'slow' adds |u_h - u|^2 from a P1 FEM Poisson solve on the moving "
                                      "mesh at every monitor evaluation, which runs only when asked for: pass m2n_solve='p1' "
                                      f"(nodal forcing, up to {SLOW_MAX_SIDE} a side); 'fast' needs nothing")
        if fast != 'fast':
            raise ValueError(f"mesh {b}: Please specify fast_M2N_monitor in params (got {fast!r}; 'fast' is built)")
    return kind


def m2n_constants(params):
    """(mon_reg, beta) of the M2N 'fast' monitor (`ma_mesh_2d.py:263-272`): 'mon_reg' is read unconditionally there, so it is
    required here, and > 0 (the monitor is mon_reg where F vanishes); 'M2N_beta' defaults to 1.5 and is >= 0."""
    if 'mon_reg' not in params:
        raise ValueError("the M2N monitor reads 'mon_reg': pass it (the reference's run parameters use 0.1)")
    reg, beta = float(params['mon_reg']), float(params.get('M2N_beta', 1.5))
    if not (0 < reg < float('inf')):
        raise ValueError(f"mon_reg = {reg}; the M2N monitor needs mon_reg > 0")
    if not (0 <= beta < float('inf')):
        raise ValueError(f"M2N_beta = {beta}; >= 0 expected")
    return reg, beta


def monitor_m2n(x: torch.Tensor, y: torch.Tensor, params) -> torch.Tensor:
    """`MA2d`'s M2N 'fast' monitor on the points given: mon_reg + beta F / max(F) with F = sqrt(u_xx^2 + 2 u_xy^2 + u_yy^2), the
    maximum over THE POINTS GIVEN (the reference takes it over the mesh's current nodes).  u_xx and u_yy are the signed sums of
    `monitor_ma`; u_xy is the last Gaussian's only, as in the reference.  Points where no F is positive get mon_reg."""
    reg, beta = m2n_constants(params)
    uxx, uyy, uxy = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    for c, s in zip(params['centers'], params['scales']):
        c0, c1, s0, s1 = float(c[0]), float(c[1]), float(s[0]), float(s[1])
        g = torch.exp(-(x - c0) ** 2 / s0 ** 2 - (y - c1) ** 2 / s1 ** 2)
        uxx = uxx + _gauss_dd(x, c0, s0) * g
        uyy = uyy + _gauss_dd(y, c1, s1) * g
        uxy = 16 * ((x - c0) * (y - c1)) / s0 ** 2 / s1 ** 2 * g          # `=`, not `+=`: ma_mesh_2d.py:133
    F = torch.sqrt(uxx ** 2 + 2 * uxy ** 2 + uyy ** 2)
    top = F.max() if F.numel() else F.new_zeros(())
    return reg + beta * F / top if top > 0 else reg + torch.zeros_like(F)


def m2n_slow_constants(params):
    """(mon_reg, alpha, beta) of the M2N 'slow' monitor (`ma_mesh_2d.py:227-261`): 'mon_reg' is required and > 0; 'M2N_alpha' and
    'M2N_beta' both default to 1.0 there and are >= 0."""
    if 'mon_reg' not in params:
        raise ValueError("the M2N monitor reads 'mon_reg': pass it (the reference's run parameters use 0.1)")
    reg, alpha, beta = float(params['mon_reg']), float(params.get('M2N_alpha', 1.0)), float(params.get('M2N_beta', 1.0))
    if not (0 < reg < float('inf')):
        raise ValueError(f"mon_reg = {reg}; the M2N monitor needs mon_reg > 0")
    if not (0 <= alpha < float('inf')):
        raise ValueError(f"M2N_alpha = {alpha}; >= 0 expected")
    if not (0 <= beta < float('inf')):
        raise ValueError(f"M2N_beta = {beta}; >= 0 expected")
    return reg, alpha, beta


def p1_error(x: torch.Tensor, y: torch.Tensor, u: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
    """u_h - u on the N x N node set (x, y), node (i, j) of `square_mesh(N)`: u_h is the P1 solution of -Laplace(u_h) = f with
    u_h = u on the boundary, the load being the consistent mass matrix applied to the nodal f.  Dense, in the dtype given;
    exactly 0 on the boundary."""
    from .mesh_graph import square_mesh
    N = x.shape[0]
    cells = square_mesh(N).cells.to(x.device)
    px, py = x.reshape(-1)[cells], y.reshape(-1)[cells]                  # [T, 3]
    rx = torch.stack([py[:, 1] - py[:, 2], py[:, 2] - py[:, 0], py[:, 0] - py[:, 1]], 1)   # tri_geometry of fem_kernels.hip
    ry = torch.stack([px[:, 2] - px[:, 1], px[:, 0] - px[:, 2], px[:, 1] - px[:, 0]], 1)
    D = (px * rx).sum(1).abs()                                           # twice the area
    Pe = (rx[:, :, None] * rx[:, None, :] + ry[:, :, None] * ry[:, None, :]) / (2 * D)[:, None, None]
    K = x.new_zeros(N * N, N * N)
    K.index_put_((cells[:, :, None].expand(-1, 3, 3), cells[:, None, :].expand(-1, 3, 3)), Pe, accumulate=True)
    ff = f.reshape(-1)[cells]
    b = x.new_zeros(N * N).index_add_(0, cells.reshape(-1), ((D / 24)[:, None] * (ff + ff.sum(1, keepdim=True))).reshape(-1))
    i, j = torch.meshgrid(torch.arange(N, device=x.device), torch.arange(N, device=x.device), indexing='ij')
    inner = ((i > 0) & (i < N - 1) & (j > 0) & (j < N - 1)).reshape(-1)
    uf = u.reshape(-1)
    c = torch.linalg.solve(K[inner][:, inner], b[inner] - K[inner][:, ~inner] @ uf[~inner])
    e = x.new_zeros(N * N)
    e[inner] = c - uf[inner]
    return e.reshape(N, N)


def monitor_m2n_slow(x: torch.Tensor, y: torch.Tensor, params) -> torch.Tensor:
    """`MA2d`'s M2N 'slow' monitor on the N x N node set given, which is its own mesh (`square_mesh(N)`'s triangles on these
    nodes): mon_reg + alpha E / max(E) + beta F / max(F) with E = (u_h - u)^2 from `p1_error`, u the sum of the Gaussians,
    f = -(u_xx + u_yy), and F as in `monitor_m2n`; both maxima over the nodes given, a term whose maximum is not positive being 0.
    What `ma_m2n_slow_kernel` computes at every update, in torch, with a dense solve, in any dtype."""
    if x.dim() != 2 or x.shape[0] != x.shape[1] or x.shape != y.shape or x.shape[0] < 3:
        raise ValueError(f"monitor_m2n_slow: x of shape {tuple(x.shape)} and y of {tuple(y.shape)}; two [N, N] node arrays, N >= 3")
    reg, alpha, beta = m2n_slow_constants(params)
    uxx, uyy, uxy, u = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    for c, s in zip(params['centers'], params['scales']):
        c0, c1, s0, s1 = float(c[0]), float(c[1]), float(s[0]), float(s[1])
        g = torch.exp(-(x - c0) ** 2 / s0 ** 2 - (y - c1) ** 2 / s1 ** 2)
        u = u + g
        uxx = uxx + _gauss_dd(x, c0, s0) * g
        uyy = uyy + _gauss_dd(y, c1, s1) * g
        uxy = 16 * ((x - c0) * (y - c1)) / s0 ** 2 / s1 ** 2 * g          # `=`, not `+=`: ma_mesh_2d.py:133
    F = torch.sqrt(uxx ** 2 + 2 * uxy ** 2 + uyy ** 2)
    E = p1_error(x, y, u, -(uxx + uyy)) ** 2
    m = reg + torch.zeros_like(F)
    if E.max() > 0:
        m = m + alpha * E / E.max()
    if F.max() > 0:
        m = m + beta * F / F.max()
    return m


def _side(b: int, size, route: str = 'lane') -> int:
    if isinstance(size, (tuple, list)):
        if len(size) != 2 or int(size[0]) != int(size[1]):
            raise ValueError(f"mesh {b}: size {tuple(size)}; square grids only")
        size = size[0]
    n = int(size)
    if n < 3:
        raise ValueError(f"mesh {b}: N = {n}; at least 3 nodes a side")
    if route == 'strided':
        if n > STRIDED_MAX_SIDE:
            raise ValueError(f"mesh {b}: N = {n}; route='strided' goes up to {STRIDED_MAX_SIDE} a side (one workgroup per mesh)")
    elif n > MAX_SIDE:
        raise ValueError(f"mesh {b}: N = {n}; Monge-Ampere meshes go up to {MAX_SIDE} a side (one lane per node, one workgroup per mesh); "
                         f"route='strided' goes up to {STRIDED_MAX_SIDE}")
    return n


def _gaussians(b: int, params):
    cs, ss = list(params.get('centers', [])), list(params.get('scales', []))
    if len(cs) != len(ss):
        raise ValueError(f"mesh {b}: {len(cs)} centres and {len(ss)} scales")
    if len(cs) > MAX_GAUSS:
        raise ValueError(f"mesh {b}: {len(cs)} Gaussians; at most {MAX_GAUSS}")
    rows = []
    for c, s in zip(cs, ss):
        if len(c) != 2 or len(s) != 2:
            raise ValueError(f"mesh {b}: a Gaussian of a 2-D mesh has two centre coordinates and two scales")
        rows.append([float(c[0]), float(c[1]), float(s[0]), float(s[1])])
    return rows


def _prepare_common(sizes: Sequence, fields: Sequence, fields_name: str, describe, *, cfl, tol, max_steps, device, route):
    """What `_prepare` and `_prepare_table` share: the scalar checks, the sides, the device, the batch's descriptors and output
    buffers on the GPU, the argument list and the (launch, collect) closures.  `describe(ns)` is the caller's own part, run after the
    sides are checked and before a device is asked for: -> (word 3 of every descriptor, what word 2 advances by per mesh,
    inputs(dev) -> the device tensors whose pointers follow the descriptors in the argument list, entry point, overflow text,
    whether the monitor is written out)."""
    if route not in ROUTES:
        raise ValueError(f"route = {route!r}; one of {ROUTES}")
    if len(sizes) == 0 or len(sizes) != len(fields):
        raise ValueError(f"{len(sizes)} mesh sizes and {len(fields)} {fields_name}")
    if not (0 <= int(max_steps) <= _native_mesh.MAX_STEPS):
        raise ValueError(f"max_steps = {max_steps}; 0..{_native_mesh.MAX_STEPS} (the loop has to end)")
    if not (0 < cfl < float('inf') and 0 <= tol < float('inf')):
        raise ValueError(f"cfl = {cfl}, tol = {tol}; cfl > 0 and tol >= 0 expected")
    ns = [_side(b, s, route) for b, s in enumerate(sizes)]
    counts, strides, inputs, entry, overflow, slow = describe(ns)
    B = len(ns)

    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device() if torch.cuda.is_available() else 0)
    if dev.type != 'cuda' or not torch.cuda.is_available():
        raise NativeError("Monge-Ampere meshes are built on the GPU only (libgadapt_mesh.so): no CUDA/HIP device is visible; "
                          "there is no CPU fallback")

    desc, noff, off = [], 0, 0
    for n, count, stride in zip(ns, counts, strides):
        desc += [n, noff, off, count]
        noff, off = noff + n * n, off + stride
    if noff >= 2 ** 31 or off >= 2 ** 31:
        raise ValueError(overflow)
    desc_host = (C.c_int32 * len(desc))(*desc)
    desc_dev = torch.tensor(desc, dtype=torch.int32).to(dev)
    ins = inputs(dev)
    x = torch.empty(noff, dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    steps = torch.empty(B, dtype=torch.int32, device=dev)
    residual = torch.empty(B, dtype=torch.float32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    monitor = torch.empty_like(x) if slow else None
    args = (B, C.cast(desc_host, C.c_void_p), desc_dev.data_ptr(), *(t.data_ptr() for t in ins), float(cfl), float(tol), int(max_steps),
            x.data_ptr(), y.data_ptr(), steps.data_ptr(), residual.data_ptr(), status.data_ptr()) + ((monitor.data_ptr(),) if slow else ())
    keep = (desc_host, desc_dev, ins)                                    # what the argument list points into

    def launch(_keep=keep):                                              # the closure keeps the inputs alive
        with torch.cuda.device(dev):
            _native_mesh.check(getattr(_native_mesh.lib(), entry)(*args, current_stream(dev)), entry)

    def collect():
        out, mons, o = [], [], 0
        for n in ns:
            out.append(torch.stack([x[o:o + n * n].view(n, n), y[o:o + n * n].view(n, n)]))
            if slow:
                mons.append(monitor[o:o + n * n].view(n, n))
            o += n * n
        return MASlowResult(out, steps, residual, status, mons) if slow else MAResult(out, steps, residual, status)

    return launch, collect


def _prepare(sizes: Sequence, pde_params: Sequence, *, cfl: float = 0.2, tol: float = 1e-4, max_steps: int = 20000, device=None,
             route: str = 'lane', m2n_solve: Optional[str] = None):
    """The host side of `ma_batch`: checks, the batch's descriptors and Gaussians on the GPU, the argument list.  Returns
    (launch, collect): `launch()` issues the one kernel (it may be issued again), `collect()` gives the MAResult (the
    MASlowResult under the 'slow' monitor)."""
    def describe(ns):
        gauss = [_gaussians(b, p) for b, p in enumerate(pde_params)]
        kinds = [monitor_kind(b, p, m2n_solve) for b, p in enumerate(pde_params)]
        if len(set(kinds)) != 1:
            if 'M2N slow' not in kinds:
                raise ValueError(f"mesh_type 'ma' for {kinds.count('ma')} meshes and 'M2N' for {kinds.count('M2N')}: all meshes of one call "
                                 "share one monitor (one launch per call); split the batch")
            raise ValueError("monitors " + ', '.join(f"{k!r} for {kinds.count(k)}" for k in sorted(set(kinds))) + " meshes: all meshes of one "
                             "call share one monitor (one launch per call); split the batch")
        m2n, slow = kinds[0] == 'M2N', kinds[0] == 'M2N slow'
        if slow:
            if route != 'lane':
                raise ValueError(f"route = {route!r}: the M2N 'slow' monitor runs on route='lane' only (its band solve lives in LDS)")
            for b, n in enumerate(ns):
                if n > SLOW_MAX_SIDE:
                    raise ValueError(f"mesh {b}: N = {n}; the M2N 'slow' monitor goes up to {SLOW_MAX_SIDE} a side (the band of the P1 solve "
                                     "stays in LDS)")
        mon = [(m2n_slow_constants if slow else m2n_constants if m2n else monitor_constants)(p) for p in pde_params]
        rows = [r for g in gauss for r in g] or [[0.0] * 4]              # never an empty allocation behind the pointer
        if slow:
            entry = 'gadapt_ma_m2n_slow_batch'
        else:
            entry = ('gadapt_ma_m2n_batch' if m2n else 'gadapt_ma_batch') + ('_strided' if route == 'strided' else '')
        counts = [len(g) for g in gauss]
        return (counts, counts, lambda dev: (torch.tensor(rows, dtype=torch.float32).to(dev), torch.tensor(mon, dtype=torch.float32).to(dev)),
                entry, "more than 2^31 nodes in one batch", slow)

    return _prepare_common(sizes, pde_params, 'parameter sets', describe, cfl=cfl, tol=tol, max_steps=max_steps, device=device, route=route)


def ma_batch(sizes: Sequence, pde_params: Sequence, *, cfl: float = 0.2, tol: float = 1e-4, max_steps: int = 20000,
             device=None, route: str = 'lane', m2n_solve: Optional[str] = None) -> MAResult:
    """Monge-Ampere meshes of many samples, mixed sizes in one launch.

    sizes[b]       N (or a pair (N, N)): the mesh is the N x N grid on the unit square, node (i, j) of meshgrid(..., indexing='ij')
    pde_params[b]  'centers' and 'scales' of the sample's Gaussians (at most 8; none gives a constant monitor and the grid itself),
                   optionally 'mon_reg' and 'mon_power' (`monitor_ma`).  With 'mesh_type': 'M2N' (and 'fast_M2N_monitor': 'fast',
                   'mon_reg' > 0, optionally 'M2N_beta', default 1.5) the monitor is `monitor_m2n` with its maximum over the
                   mesh's current nodes at every update; 'mon_power' and 'M2N_alpha' are accepted and ignored there.  All
                   meshes of a call share one 'mesh_type' ('ma' when absent); a mixed batch is a `ValueError`
    cfl            the pseudo-time step is cfl h^2 min(1, lambda_min); 0.2 converged in every case tried up to 32 x 32, 0.5
                   oscillates into the cap, 1 loses convexity at once
    tol            stop when max |r - mean r| <= tol; 0 runs exactly `max_steps` updates
    max_steps      the cap (32 x 32 needed up to 8 200 residual evaluations; 64 x 64 wanted 17 500 to 25 500 updates and
                   81 x 81 28 000 to 32 000: raise it there, the default can return CAP)
    route          'lane' (3 <= N <= 32, phi in fp32) or 'strided' (3 <= N <= 81, phi in fp64, K = ceil(N^2 / 1024) nodes per
                   lane).  The two do not give the same bits at N <= 32; any other value is a `ValueError`
    m2n_solve      None (the default: 'fast_M2N_monitor': 'slow' is a `NotImplementedError`, as ever) or 'p1': 'slow' then runs
                   `monitor_m2n_slow` inside the kernel ('mon_reg' > 0, 'M2N_alpha' and 'M2N_beta' >= 0, both 1.0 by default;
                   route 'lane' only, N <= 24, else `ValueError`).  'ma' and 'fast' ignore it; 'superslow' stays unbuilt

    Returns MAResult(coords, steps, residual, status) on the GPU: coords[b] is [2, N, N], and per-mesh tensors of the number of
    updates (int32), the last residual and CONVERGED / CAP / NONCONVEX.  A mesh's result does not depend on its batch.  Under
    the 'slow' monitor it is MASlowResult(coords, steps, residual, status, monitor), monitor[b] [N, N] being m of the last
    evaluation (with `max_steps=0, tol=0`: the monitor of the uniform grid).
    """
    launch, collect = _prepare(sizes, pde_params, cfl=cfl, tol=tol, max_steps=max_steps, device=device, route=route,
                               m2n_solve=m2n_solve)
    launch()
    return collect()


# --------------------------------------------------------------------------
# a tabulated monitor
# --------------------------------------------------------------------------

def monitor_table(params, T: int, dtype=torch.float64) -> torch.Tensor:
    """The closed-form monitor of `params` on the T x T lattice of the unit square, [T, T] with entry (i, j) at
    (i / (T-1), j / (T-1)): `monitor_ma`, or `monitor_m2n` for `mesh_type: 'M2N'` with `fast_M2N_monitor: 'fast'`, its maximum
    taken over the lattice (a table does not move with the mesh).  What `ma_table_batch` takes for a monitor that is known."""
    T = int(T)
    if not (2 <= T <= TABLE_MAX_SIDE):
        raise ValueError(f"T = {T}; a monitor table has 2..{TABLE_MAX_SIDE} points a side")
    kind = monitor_kind(0, params)
    lin = torch.arange(T, dtype=dtype) / (T - 1)
    gx, gy = torch.meshgrid(lin, lin, indexing='ij')
    return (monitor_m2n if kind == 'M2N' else monitor_ma)(gx, gy, params)


def monitor_from_nodal(u: torch.Tensor, *, mon_reg: float = 1.0, mon_power: float = 0.2) -> torch.Tensor:
    """The `diag_hessian_ma` monitor (mon_reg + sqrt(u_xx^2 + u_yy^2)) ** mon_power of a nodal field u [T, T] on the uniform
    lattice of the unit square (entry (i, j) at (i / (T-1), j / (T-1))), T >= 3.  u_xx and u_yy are second differences with spacing
    1 / (T-1); a boundary row or column takes the value of its interior neighbour, so a quadratic u gives the exact monitor
    everywhere.  Plain torch, in the dtype and on the device of u."""
    if not torch.is_tensor(u) or u.dim() != 2 or u.shape[0] != u.shape[1] or u.shape[0] < 3 or not u.is_floating_point():
        raise ValueError(f"monitor_from_nodal: u of shape {tuple(u.shape) if torch.is_tensor(u) else type(u)}; a floating [T, T] "
                         "lattice, T >= 3")
    inv_h2 = float((u.shape[0] - 1) ** 2)
    dxx = ((u[2:, :] - 2.0 * u[1:-1, :]) + u[:-2, :]) * inv_h2
    dyy = ((u[:, 2:] - 2.0 * u[:, 1:-1]) + u[:, :-2]) * inv_h2
    uxx = torch.cat([dxx[:1], dxx, dxx[-1:]], 0)
    uyy = torch.cat([dyy[:, :1], dyy, dyy[:, -1:]], 1)
    return (mon_reg + torch.sqrt(uxx * uxx + uyy * uyy)) ** mon_power


def _table_side(b: int, table) -> int:
    if not torch.is_tensor(table) or table.dim() != 2 or table.shape[0] != table.shape[1] or not table.is_floating_point():
        what = tuple(table.shape) if torch.is_tensor(table) else type(table).__name__
        raise ValueError(f"mesh {b}: monitor table {what}; a square [T, T] floating-point tensor")
    T = int(table.shape[0])
    if not (2 <= T <= TABLE_MAX_SIDE):
        raise ValueError(f"mesh {b}: T = {T}; a monitor table has 2..{TABLE_MAX_SIDE} points a side")
    return T


def _prepare_table(sizes: Sequence, tables: Sequence, *, cfl: float = 0.2, tol: float = 1e-4, max_steps: int = 20000, device=None,
                   route: str = 'lane'):
    """The host side of `ma_table_batch`, split like `_prepare`: checks, the batch's descriptors and tables on the GPU, the
    argument list.  Returns (launch, collect)."""
    def describe(ns):
        ts = [_table_side(b, t) for b, t in enumerate(tables)]
        return (ts, [t * t for t in ts],
                lambda dev: (torch.cat([t.detach().to(device=dev, dtype=torch.float32).reshape(-1) for t in tables]).contiguous(),),
                'gadapt_ma_table_batch' + ('_strided' if route == 'strided' else ''), "more than 2^31 nodes or table entries in one batch", False)

    return _prepare_common(sizes, tables, 'monitor tables', describe, cfl=cfl, tol=tol, max_steps=max_steps, device=device, route=route)


def ma_table_batch(sizes: Sequence, tables: Sequence, *, cfl: float = 0.2, tol: float = 1e-4, max_steps: int = 20000,
                   route: str = 'lane', device=None) -> MAResult:
    """Monge-Ampere meshes of many samples from TABULATED monitors, mixed mesh sizes and mixed table sizes in one launch.

    sizes[b]    N (or a pair (N, N)), as in `ma_batch`
    tables[b]   [T, T], any float dtype, any device (copied to fp32 on the GPU): the monitor at the physical points
                (i / (T-1), j / (T-1)), 2 <= T <= 1024, read bilinearly at the moving nodes (`include/gadapt_mesh.h`).  The entries
                have to be positive and finite: one that is not comes back as NONCONVEX, never as a fault
    cfl, tol, max_steps, route   as in `ma_batch`: 'lane' for 3 <= N <= 32, 'strided' for 3 <= N <= 81

    Returns `ma_batch`'s MAResult.  A mesh's result does not depend on its batch; a constant table gives 0 updates and the grid.
    """
    launch, collect = _prepare_table(sizes, tables, cfl=cfl, tol=tol, max_steps=max_steps, device=device, route=route)
    launch()
    return collect()


def warn_status(status, what: str = 'Monge-Ampere'):
    """NONCONVEX and CAP as warnings (the reference swallows the mover's exception and prints nothing)."""
    st = status.tolist() if torch.is_tensor(status) else list(status)
    if NONCONVEX in st:
        warnings.warn(f"{what} lost convexity for {st.count(NONCONVEX)} of {len(st)} meshes (min eigenvalue of I + H phi <= 0, or a "
                      "residual that is not finite), please choose a smaller cfl", RuntimeWarning, stacklevel=3)
    warn_unconverged([_native_mesh.CAP if s == CAP else _native_mesh.CONVERGED for s in st], what)


def _solver_kwargs(solver: dict, allowed=('cfl', 'tol', 'max_steps', 'm2n_solve', 'device')) -> dict:
    extra = set(solver) - set(allowed)
    if extra:
        raise TypeError(f"unexpected keyword arguments {sorted(extra)}; {', '.join(allowed[:-1])} and {allowed[-1]} go to ma_batch")
    return solver


def _dataset_solver_kwargs(solver: dict) -> dict:
    """The dataset path also takes `route`; `MA2d` and `deform_mesh_ma2d` keep the reference-shaped keyword set."""
    return _solver_kwargs(solver, ('cfl', 'tol', 'max_steps', 'route', 'm2n_solve', 'device'))


# --------------------------------------------------------------------------
# the reference's entry points
# --------------------------------------------------------------------------

def MA2d(x_comp: torch.Tensor, N: int, params, **solver):
    """`MA2d(x_comp, N, params)` -> (x_phys, j, build_time): the Monge-Ampere mesh of the N x N grid written back in the node
    order of `x_comp` [N*N, 2] (`mmpde5.write_back_to_nodes`), j the number of updates.  Lost convexity warns and gives zeros
    and j = 0, as the reference's `except` branch does; a reached cap warns.  Keyword-only `cfl`, `tol`, `max_steps` and `m2n_solve`
    go to `ma_batch`.  `params['mesh_type'] == 'M2N'` selects the M2N 'fast' monitor (`monitor_m2n`), as in the reference, or, with
    `fast_M2N_monitor = 'slow'` and `m2n_solve='p1'`, the 'slow' one (`monitor_m2n_slow`); absent, it is 'ma'."""
    _solver_kwargs(solver)
    if x_comp.dim() != 2 or tuple(x_comp.shape) != (N * N, 2):
        raise ValueError(f"MA2d: x_comp of shape {tuple(x_comp.shape)}; [{N * N}, 2] expected (square grids only)")
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    t0 = time.time()
    res = ma_batch([N], [params], **solver)
    status = res.status.tolist()                           # waits for the device
    build_time = time.time() - t0
    warn_status(status)
    if status[0] == NONCONVEX:
        return torch.zeros_like(x_comp), 0, build_time
    gx, gy = unit_grid(N, x_comp.device)
    xy = res.coords[0].to(x_comp.device)
    return write_back_to_nodes(x_comp, gx, gy, xy[0], xy[1]), int(res.steps[0]), build_time


def deform_mesh_ma2d(x_comp: torch.Tensor, n: int, m: int, pde_params, **solver):
    """`src/data.py` `deform_mesh_ma2d`: `MA2d` on the n x m grid -> (x_phys, j + 1, build_time), the count plus one "to account
    for the initial mesh".  Square grids only."""
    if n != m:
        raise ValueError(f"deform_mesh_ma2d: {n} x {m} grid; square grids only")
    x_phys, j, build_time = MA2d(x_comp, n, pde_params, **solver)
    return x_phys, j + 1, build_time


# --------------------------------------------------------------------------
# dataset targets
# --------------------------------------------------------------------------

def nodal_grid(x_comp: torch.Tensor, values: torch.Tensor, n: int) -> torch.Tensor:
    """A nodal field [n*n] in the node order of `x_comp` [n*n, 2] laid out as [n, n] on `unit_grid(n)`: entry (i, j) is the value
    at the node nearest to the grid point (i, j), the mapping of `write_back_to_nodes` read the other way."""
    gx, gy = unit_grid(n, x_comp.device)
    lo, hi = x_comp.min(0).values, x_comp.max(0).values
    scaled = ((x_comp - lo) / (hi - lo)).to(torch.float32)
    node = torch.cdist(torch.stack([gx.reshape(-1), gy.reshape(-1)], 1), scaled).argmin(1)
    return values.reshape(-1)[node].reshape(n, n)


def attach_ma_targets(samples, monitor_params: Optional[dict] = None, **solver):
    """`x_phys` of every sample := its Monge-Ampere mesh, all samples in ONE batched call; `ma_its` = updates + 1 and
    `build_time` (the batched call's wall time shared out evenly) as `attach_mmpde5_targets` sets them.  The monitor of a
    sample is `monitor_ma` of its own `pde_params` with `monitor_params` (`mon_reg`, `mon_power`) added, or `monitor_m2n` where
    `monitor_params` carries `mesh_type: 'M2N'` (`fast_M2N_monitor`, `mon_reg`, `M2N_beta`).  The samples' meshes
    must be square grids in grid order (`square_mesh`).  A sample that lost convexity gets zeros and `ma_its` = 1.
    Keyword-only `cfl`, `tol`, `max_steps`, `route`, `m2n_solve` and `device` go to `ma_batch` (`route='strided'` for 33..81 a side;
    `m2n_solve='p1'` for `fast_M2N_monitor: 'slow'`).
    `monitor_params['monitor_source']`: 'analytic' (the default: the path above) or 'uu': each sample's monitor is then
    `monitor_from_nodal` of its own `uu_tensor` laid out on its N x N grid (`nodal_grid`), with `mon_reg` / `mon_power` from
    `monitor_params`, as a table of T = N for `ma_table_batch`; `route`, `cfl`, `tol` and `max_steps` work as above.  'uu' with
    `mesh_type: 'M2N'` is a `ValueError`: that monitor's maximum moves with the mesh, a table does not."""
    _dataset_solver_kwargs(solver)
    monitor_params = dict(monitor_params or {})
    source = monitor_params.pop('monitor_source', 'analytic')
    if source not in MONITOR_SOURCES:
        raise ValueError(f"monitor_source = {source!r}; one of {MONITOR_SOURCES}")
    if source == 'uu':
        if monitor_params.get('mesh_type', 'ma') != 'ma':
            raise ValueError(f"monitor_source = 'uu' with mesh_type = {monitor_params['mesh_type']!r}: the M2N monitor's maximum moves "
                             "with the mesh, a tabulated monitor does not; use mesh_type 'ma' (mon_reg, mon_power)")
        if solver.get('m2n_solve') is not None:
            raise ValueError("monitor_source = 'uu' has no M2N solve: leave m2n_solve out")
        solver = {k: v for k, v in solver.items() if k != 'm2n_solve'}
        reg, power = monitor_constants(monitor_params)
    sizes, params = [], []
    for d in samples:
        if d.x_comp.dim() != 2 or d.x_comp.shape[1] != 2:
            raise ValueError("Monge-Ampere targets are 2-D only (the reference has no 1-D MA): use target='mmpde5' for 1-D meshes")
        n = int(round(d.x_comp.shape[0] ** 0.5))
        if n * n != d.x_comp.shape[0]:
            raise ValueError(f"{d.x_comp.shape[0]} nodes: not a square grid")
        sizes.append(n)
        params.append(dict(d.pde_params, **(monitor_params or {})))
    t0 = time.time()
    if source == 'uu':
        tables = [monitor_from_nodal(nodal_grid(d.x_comp, d.uu_tensor, n).double(), mon_reg=reg, mon_power=power)
                  for d, n in zip(samples, sizes)]
        res = ma_table_batch(sizes, tables, **solver)
    else:
        res = ma_batch(sizes, params, **solver)
    steps, status = res.steps.tolist(), res.status.tolist()   # waits for the device: the batched call is done
    build_time = (time.time() - t0) / max(len(samples), 1)
    warn_status(status, 'Monge-Ampere (dataset targets)')
    for d, xy, j, st in zip(samples, res.coords, steps, status):
        x_phys = xy.reshape(2, -1).t().contiguous().to(device=d.x_comp.device, dtype=d.x_comp.dtype)
        d.x_phys, d.ma_its = (torch.zeros_like(x_phys), 1) if st == NONCONVEX else (x_phys, j + 1)
        d.build_time = build_time
    return res
