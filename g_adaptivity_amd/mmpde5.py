"""MMPDE5 target meshes on the GPU: the reference's classical mesh generator (`classical_meshing/ma_mesh_1d.py:7-134`,
`ma_mesh_2d.py:11-103`, `src/data.py:394-416`), batched.

The moving-mesh PDE is relaxed by explicit RK4 in pseudo-time until one step moves the nodes by less than `tol` in the l1
sense.  The monitor function is evaluated on the fixed computational grid, so it is computed once per mesh here, in torch
(`monitor_1d`, `monitor_2d`, or any callable), and the whole iteration of a batch of meshes runs in one launch of
`libgadapt_mesh.so` (`include/gadapt_mesh.h`): one workgroup per mesh, each to its own stopping step.

`mmpde5_batch` is the batched form; `MMPDE5_1d`, `MMPDE5_2d`, `MMPDE5_1d_burgers`, `deform_mesh_mmpde1d` and
`deform_mesh_mmpde2d` keep the reference's names, argument lists and return tuples.  Tensors may live on the CPU or the GPU;
the iteration always runs on the GPU (there is no CPU fallback: `NativeError` without one) and results come back on the
device of the input.

Two routes run the same arithmetic.  `route='lane'` (the default) holds one node per lane of the workgroup: 1-D N <= 1024,
2-D N <= 32.  `route='strided'` holds up to 7 nodes per lane and takes 2-D meshes up to 81 x 81, the limit of the windowed
FEM route (`fem_band='window'`); a mesh of at most 1024 nodes gives the same bits on both.  Sizes beyond a route's limit raise
`ValueError`; nothing changes its route unasked.

The reference's step is cfl / N^3 with cfl = 0.05, so the diffusion number falls like 1 / N and the step count grows like
N^3: with two Gaussians and the default monitor the fp32 iteration needs 20 046 steps at 33 x 33 (beyond the reference's cap
of 10 000, so the default call returns CAP as the reference would) and has a measure of 2.3e-4 left after 50 000 steps at
64 x 64, where `cfl=0.5` is stable and converges after 15 556.  Large meshes want `max_steps` or `cfl` raised; a STIFF status
says when `cfl` was too much.  The defaults are the reference's at every size.
"""
from __future__ import annotations

import ctypes as C
import time
import warnings
from collections import namedtuple
from typing import Callable, Optional, Sequence

import torch

from . import _native_mesh
from ._native import NativeError, current_stream

CONVERGED, CAP, STIFF = _native_mesh.CONVERGED, _native_mesh.CAP, _native_mesh.STIFF
STATUS_NAMES = {CONVERGED: 'converged', CAP: 'cap reached', STIFF: 'too stiff'}

MMPDE5Result = namedtuple('MMPDE5Result', 'coords steps measure status')


# --------------------------------------------------------------------------
# monitor functions
# --------------------------------------------------------------------------

def _gauss_dd(t, c, s):
    """d^2/dt^2 of exp(-(t - c)^2 / s^2), without the exponential: (4 (t - c)^2 - 2 s^2) / s^4."""
    return (4.0 * (t - c) ** 2 - 2.0 * s * s) / s ** 4


def monitor_1d(xi: torch.Tensor, params) -> torch.Tensor:
    """The reference's 1-D monitor `m(x, params)` for u = sum_k exp(-(x - c_k)^2 / s_k^2):

        dh = u_xx^2 / max(u_xx^2)            (the maximum over THIS grid: two grids are normalised by two maxima)
        m  = (mon_reg + dh)^mon_power        if both keys are given
             (1 + dh)^mon_power              if only mon_power is
             (1 + dh)^0.2                    otherwise
    """
    uxx = torch.zeros_like(xi)
    for c, s in zip(params['centers'], params['scales']):
        c0, s0 = float(c[0]), float(s[0])
        uxx = uxx + _gauss_dd(xi, c0, s0) * torch.exp(-(xi - c0) ** 2 / s0 ** 2)
    dh = uxx ** 2 / torch.max(uxx ** 2)
    if 'mon_reg' in params and 'mon_power' in params:
        return (params['mon_reg'] + dh) ** params['mon_power']
    return (1 + dh) ** params.get('mon_power', 0.2)


def monitor_2d(x: torch.Tensor, y: torch.Tensor, params) -> torch.Tensor:
    """The reference's 2-D monitor `m(x, y, params)`: (1 + (sum_k |u_xx,k|)^2 + (sum_k |u_yy,k|)^2)^mon_power with
    mon_power = 0.2 unless given.  `mon_reg` is not read in 2-D, as in the reference."""
    axx, ayy = torch.zeros_like(x), torch.zeros_like(x)
    for c, s in zip(params['centers'], params['scales']):
        c0, c1, s0, s1 = float(c[0]), float(c[1]), float(s[0]), float(s[1])
        g = torch.exp(-(x - c0) ** 2 / s0 ** 2 - (y - c1) ** 2 / s1 ** 2)
        axx = axx + torch.abs(_gauss_dd(x, c0, s0) * g)
        ayy = ayy + torch.abs(_gauss_dd(y, c1, s1) * g)
    return (1 + axx ** 2 + ayy ** 2) ** params.get('mon_power', 0.2)


def monitor_arrays_1d(m: Callable, n: int, device=None):
    """(`ms`, `m2`) of the right-hand side: `m` on linspace(0, 1, 2n - 1) at the odd indices (cell centres) and on the n nodes."""
    return m(torch.linspace(0, 1, 2 * n - 1, device=device))[1:2 * n - 1:2], m(torch.linspace(0, 1, n, device=device))


def monitor_arrays_2d(m: Callable, n: int, device=None):
    lin, fine = torch.linspace(0, 1, n, device=device), torch.linspace(0, 1, 2 * n - 1, device=device)
    xf, yf = torch.meshgrid(fine, fine, indexing='ij')
    xn, yn = torch.meshgrid(lin, lin, indexing='ij')
    return m(xf, yf)[1:2 * n - 1:2, 1:2 * n - 1:2], m(xn, yn)


# --------------------------------------------------------------------------
# the batched iteration
# --------------------------------------------------------------------------

ROUTES = ('lane', 'strided')


def _shape_of(b: int, xy, ms, m2, route: str = 'lane'):
    """(dim, N) of mesh b; ValueError for anything the kernel of `route` does not take."""
    if xy.dim() == 1:
        dim, n = 1, xy.shape[0]
        want_ms, want_m2 = (n - 1,), (n,)
    elif xy.dim() == 3 and xy.shape[0] == 2 and xy.shape[1] == xy.shape[2]:
        dim, n = 2, xy.shape[1]
        want_ms, want_m2 = (n - 1, n - 1), (n, n)
    else:
        raise ValueError(f"mesh {b}: coordinates of shape {tuple(xy.shape)}; [N] (1-D) or [2, N, N] (2-D, square) expected")
    if n < 3:
        raise ValueError(f"mesh {b}: N = {n}; at least 3 nodes a side")
    if route == 'strided':
        if n > (_native_mesh.MAX_NODES if dim == 1 else _native_mesh.STRIDED_MAX_SIDE):
            raise ValueError(f"mesh {b}: N = {n} in {dim}-D; route='strided' takes 1-D N <= {_native_mesh.MAX_NODES} and "
                             f"2-D N <= {_native_mesh.STRIDED_MAX_SIDE} a side (one workgroup holds a mesh)")
    elif n ** dim > _native_mesh.MAX_NODES:
        raise ValueError(f"mesh {b}: N = {n} in {dim}-D; at most {_native_mesh.MAX_NODES} nodes per mesh "
                         "(1-D N <= 1024, 2-D N <= 32: one workgroup holds a mesh; route='strided' takes 2-D up to 81 a side)")
    if tuple(ms.shape) != want_ms or tuple(m2.shape) != want_m2:
        raise ValueError(f"mesh {b}: monitor arrays of shapes {tuple(ms.shape)}, {tuple(m2.shape)}; {want_ms}, {want_m2} expected")
    return dim, n


def _prepare(coords: Sequence, monitors: Sequence, *, cfl: float = 0.05, step=None, tol: float = 1e-6,
             max_steps: int = 10000, tau: float = 0.1, device=None, route: str = 'lane'):
    """The host side of `mmpde5_batch`: checks, one concatenated copy of the batch on the GPU, the argument list.  Returns
    (launch, collect, keep): `launch()` issues the one kernel (it may be issued again: inputs are not overwritten),
    `collect()` gives the MMPDE5Result."""
    if route not in ROUTES:
        raise ValueError(f"route = {route!r}; one of {ROUTES}")
    if len(coords) == 0 or len(coords) != len(monitors):
        raise ValueError(f"{len(coords)} meshes and {len(monitors)} monitor pairs")
    if not (0 <= int(max_steps) <= _native_mesh.MAX_STEPS):
        raise ValueError(f"max_steps = {max_steps}; 0..{_native_mesh.MAX_STEPS} (the loop has to end)")
    if not (tol >= 0 and tau > 0):
        raise ValueError(f"tol = {tol}, tau = {tau}; tol >= 0 and tau > 0 expected")
    xs = [torch.stack([torch.as_tensor(c[0]), torch.as_tensor(c[1])]) if isinstance(c, (tuple, list)) else c for c in coords]
    shapes = [_shape_of(b, xy, ms, m2, route) for b, (xy, (ms, m2)) in enumerate(zip(xs, monitors))]
    B = len(xs)
    if step is None:
        steps_in = [cfl / n ** 3 for _, n in shapes]
    else:
        steps_in = [float(s) for s in step] if isinstance(step, (list, tuple)) or torch.is_tensor(step) and step.dim() else [float(step)] * B
    if len(steps_in) != B or not all(0 < s < float('inf') for s in steps_in):
        raise ValueError("step: one positive finite number, or one per mesh")

    home = xs[0].device
    if device is not None:
        dev = torch.device(device)
    else:
        dev = home if home.type == 'cuda' else torch.device('cuda', torch.cuda.current_device() if torch.cuda.is_available() else 0)
    if dev.type != 'cuda' or not torch.cuda.is_available():
        raise NativeError("MMPDE5 runs on the GPU only (libgadapt_mesh.so): no CUDA/HIP device is visible; there is no CPU fallback")

    def flat(parts):
        return torch.cat([p.detach().reshape(-1).to(torch.float32) for p in parts]).to(dev).contiguous()

    x0 = flat([xy if d == 1 else xy[0] for xy, (d, _) in zip(xs, shapes)])
    y0 = flat([torch.zeros_like(xy) if d == 1 else xy[1] for xy, (d, _) in zip(xs, shapes)])
    ms = flat([m[0] for m in monitors])
    m2 = flat([m[1] for m in monitors])
    desc, noff, coff = [], 0, 0
    for d, n in shapes:
        desc += [d, n, noff, coff]
        noff, coff = noff + n ** d, coff + (n - 1) ** d
    if noff >= 2 ** 31:
        raise ValueError("more than 2^31 nodes in one batch")
    desc_host = (C.c_int32 * len(desc))(*desc)
    desc_dev = torch.tensor(desc, dtype=torch.int32).to(dev)
    step_dev = torch.tensor(steps_in, dtype=torch.float64).to(dev)
    x, y = torch.empty_like(x0), torch.empty_like(y0)
    n_steps = torch.empty(B, dtype=torch.int32, device=dev)
    measure = torch.empty(B, dtype=torch.float32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    args = (B, C.cast(desc_host, C.c_void_p), desc_dev.data_ptr(), x0.data_ptr(), y0.data_ptr(), ms.data_ptr(), m2.data_ptr(),
            step_dev.data_ptr(), float(tau), float(tol), int(max_steps), x.data_ptr(), y.data_ptr(), n_steps.data_ptr(),
            measure.data_ptr(), status.data_ptr())
    keep = (desc_host, desc_dev, x0, y0, ms, m2, step_dev)               # what the argument list points into

    entry = 'gadapt_mmpde5_batch' if route == 'lane' else 'gadapt_mmpde5_batch_strided'

    def launch(_keep=keep):                                              # the closure keeps the inputs alive
        with torch.cuda.device(dev):
            _native_mesh.check(getattr(_native_mesh.lib(), entry)(*args, current_stream(dev)), entry)

    def collect():
        out, o = [], 0
        for xy, (d, n) in zip(xs, shapes):
            k = n ** d
            res = x[o:o + k] if d == 1 else torch.stack([x[o:o + k].view(n, n), y[o:o + k].view(n, n)])
            out.append(res.to(device=xy.device, dtype=xy.dtype))
            o += k
        return MMPDE5Result(out, n_steps.to(home), measure.to(home), status.to(home))

    return launch, collect, keep


def mmpde5_batch(coords: Sequence, monitors: Sequence, *, cfl: float = 0.05, step=None, tol: float = 1e-6,
                 max_steps: int = 10000, tau: float = 0.1, device=None, route: str = 'lane') -> MMPDE5Result:
    """MMPDE5 on many meshes of mixed sizes and dimensions, one launch.

    coords[b]    start coordinates: a tensor [N] (1-D), or [2, N, N] / a pair (X, Y) of [N, N] (2-D, node (i, j) of
                 meshgrid(..., indexing='ij'))
    monitors[b]  (ms, m2): the monitor at the cell centres ([N-1] or [N-1, N-1]) and at the nodes ([N] or [N, N])
    cfl / step   RK4 step: cfl / N^3 per mesh (the reference's, cfl = 0.05), or `step` (a number or one per mesh)
    tol          stop when sum |new - old| <= tol; 0 runs exactly `max_steps` steps
    max_steps    the reference's cap is 10 000;  tau: the reference's 0.1
    route        'lane' (default): one node per lane, 2-D N <= 32.  'strided': several nodes per lane, 2-D N <= 81; the same
                 bits as 'lane' for a mesh of at most 1024 nodes.  1-D N <= 1024 on both.

    Returns MMPDE5Result(coords, steps, measure, status): the coordinates in the shapes given, and per-mesh tensors of the
    step count (int32), the last measure and CONVERGED / CAP / STIFF.  A mesh's result does not depend on its batch.
    """
    launch, collect, _ = _prepare(coords, monitors, cfl=cfl, step=step, tol=tol, max_steps=max_steps, tau=tau, device=device,
                                  route=route)
    launch()
    return collect()


def warn_unconverged(status, what: str = 'MMPDE5'):
    """The reference prints these two lines; here they are warnings."""
    st = status.tolist() if torch.is_tensor(status) else list(status)
    if STIFF in st:
        warnings.warn(f"{what} is too stiff for {st.count(STIFF)} of {len(st)} meshes, please choose a smaller CFL", RuntimeWarning, stacklevel=3)
    if CAP in st:
        warnings.warn(f"{what} has not yet converged to a stationary solution for {st.count(CAP)} of {len(st)} meshes "
                      "(step cap reached)", RuntimeWarning, stacklevel=3)


def _timed_single(xy, ms, m2, **solver):
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    t0 = time.time()
    res = mmpde5_batch([xy], [(ms, m2)], **solver)
    torch.cuda.synchronize()
    build_time = time.time() - t0
    warn_unconverged(res.status)
    return res.coords[0], int(res.steps[0]), build_time


# --------------------------------------------------------------------------
# the reference's entry points
# --------------------------------------------------------------------------

def MMPDE5_1d(X: torch.Tensor, N: int, params):
    """`MMPDE5_1d(X, N, params)` -> (X, j, build_time): Gaussian monitor `monitor_1d`, CFL 0.05, tol 1e-6, at most 10 000 steps."""
    ms, m2 = monitor_arrays_1d(lambda t: monitor_1d(t, params), N, X.device)
    return _timed_single(X, ms, m2)


def MMPDE5_1d_burgers(m: Callable, X: torch.Tensor, N: int):
    """`MMPDE5_1d_burgers(m, X, N)` -> (X, j, build_time): the monitor is the callable `m(grid)`, X may start non-uniform."""
    ms, m2 = monitor_arrays_1d(m, N, X.device)
    return _timed_single(X, torch.as_tensor(ms), torch.as_tensor(m2))


def _solver_kwargs(solver: dict) -> dict:
    extra = set(solver) - {'route', 'cfl', 'max_steps', 'tol'}
    if extra:
        raise TypeError(f"unexpected keyword arguments {sorted(extra)}; route, cfl, max_steps and tol go to mmpde5_batch")
    return solver


def MMPDE5_2d(X: torch.Tensor, Y: torch.Tensor, N: int, params, **solver):
    """`MMPDE5_2d(X, Y, N, params)` -> (X, Y, j, build_time) on [N, N] grids (`indexing='ij'`), monitor `monitor_2d`.
    Keyword-only `route`, `cfl`, `max_steps`, `tol` go to `mmpde5_batch` (N > 32 needs `route='strided'`)."""
    _solver_kwargs(solver)
    ms, m2 = monitor_arrays_2d(lambda a, b: monitor_2d(a, b, params), N, X.device)
    xy, j, build_time = _timed_single(torch.stack([X, Y]), ms, m2, **solver)
    return xy[0], xy[1], j, build_time


def deform_mesh_mmpde1d(x_comp: torch.Tensor, n: int, opt):
    """`src/data.py:394-401`: the MMPDE5 mesh of the uniform n-node interval, in grid order -> (x_phys, j, build_time).
    As in the reference the start mesh is linspace(0, 1, n) whatever `x_comp` holds."""
    return MMPDE5_1d(torch.linspace(0, 1, n, device=x_comp.device), n, opt)


def deform_mesh_mmpde2d(x_comp: torch.Tensor, n: int, m: int, pde_params, **solver):
    """`src/data.py:404-416`: the MMPDE5 mesh of the uniform n x m grid written back in the node order of `x_comp` [n*m, 2]
    (each grid point goes to the node nearest to it after scaling to the unit square) -> (x_phys, j + 1, build_time).

    The count is the step count plus one "to account for the initial mesh".  (As shipped the reference's write-back loop
    reuses the name `j`, so it returns m whatever the iteration did; the documented intent is built.)  Square grids only:
    the reference's own mapping does not hold otherwise (`src/utils_data.py:52`).  Keyword-only `route`, `cfl`, `max_steps`,
    `tol` go to `mmpde5_batch`, as in `MMPDE5_2d`."""
    if n != m:
        raise ValueError(f"deform_mesh_mmpde2d: {n} x {m} grid; square grids only")
    gx, gy = unit_grid(n, x_comp.device)
    X, Y, j, build_time = MMPDE5_2d(gx, gy, n, pde_params, **solver)
    return write_back_to_nodes(x_comp, gx, gy, X, Y), j + 1, build_time


def unit_grid(n: int, device=None):
    """(gx, gy) of the uniform n x n grid on the unit square, `indexing='ij'`."""
    lin = torch.linspace(0, 1, n, device=device)
    return torch.meshgrid(lin, lin, indexing='ij')


def write_back_to_nodes(x_comp: torch.Tensor, gx: torch.Tensor, gy: torch.Tensor, X: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
    """The write-back of `src/data.py:404-416`: the moved grid point (X, Y)[i, j] goes to the node of `x_comp` [n*n, 2] that is
    nearest to the grid point (gx, gy)[i, j] after `x_comp` is scaled to the unit square.  Shared by `deform_mesh_mmpde2d` and
    `monge_ampere.MA2d`."""
    lo, hi = x_comp.min(0).values, x_comp.max(0).values
    scaled = ((x_comp - lo) / (hi - lo)).to(torch.float32)
    node = torch.cdist(torch.stack([gx.reshape(-1), gy.reshape(-1)], 1), scaled).argmin(1)
    x_phys = torch.zeros_like(x_comp)
    x_phys[node] = torch.stack([X.reshape(-1), Y.reshape(-1)], 1).to(x_comp.dtype)
    return x_phys


# --------------------------------------------------------------------------
# dataset targets
# --------------------------------------------------------------------------

def attach_mmpde5_targets(samples, monitor_params: Optional[dict] = None, **solver):
    """`x_phys` of every sample := its MMPDE5 mesh, all samples in ONE batched call; `ma_its` per sample as the reference's
    dataset builder stores it (`src/data.py:206-212`: the step count in 1-D, the count plus one in 2-D).

    The monitor of a sample is `monitor_1d` / `monitor_2d` of its own `pde_params` (centres and scales), with
    `monitor_params` (`mon_power`, `mon_reg`) added.  `build_time` per sample (the reference's `data.build_time`, read by
    `evaluate_model_fine` as MA_time) is the wall time of the batched call divided by the sample count.  The samples' meshes must be in grid order (`interval_mesh`,
    `square_mesh`): the start mesh is `x_comp`.  `solver`: keyword arguments of `mmpde5_batch` (`route='strided'` for 2-D meshes
    of 33..81 a side, with `cfl` / `max_steps` / `tol`)."""
    coords, monitors = [], []
    for d in samples:
        params = dict(d.pde_params, **(monitor_params or {}))
        if d.x_comp.dim() == 1:
            n = d.x_comp.shape[0]
            coords.append(d.x_comp)
            monitors.append(monitor_arrays_1d(lambda t: monitor_1d(t, params), n))
        else:
            n = int(round(d.x_comp.shape[0] ** 0.5))
            if n * n != d.x_comp.shape[0]:
                raise ValueError(f"{d.x_comp.shape[0]} nodes: not a square grid")
            coords.append(d.x_comp.t().reshape(2, n, n))
            monitors.append(monitor_arrays_2d(lambda a, b: monitor_2d(a, b, params), n))
    t0 = time.time()
    res = mmpde5_batch(coords, monitors, **solver)
    steps = res.steps.tolist()                            # waits for the device: the batched call is done
    build_time = (time.time() - t0) / max(len(samples), 1)
    warn_unconverged(res.status, 'MMPDE5 (dataset targets)')
    for d, xy, j in zip(samples, res.coords, steps):
        if xy.dim() == 1:
            d.x_phys, d.ma_its = xy.contiguous(), j
        else:
            d.x_phys, d.ma_its = xy.reshape(2, -1).t().contiguous(), j + 1
        d.build_time = build_time                         # seconds, the batched call's wall time shared out evenly
    return res
