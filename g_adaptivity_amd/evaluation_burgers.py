"""The reference's Burgers evaluation (`src/utils_eval_Burgers.py`) on the GPU: the one-step table and the rollout table.

    evaluate_model_fine_burgers(model, dataset, opt, batch_size=1) -> (df, df_time)              (:10-86)
    evaluate_model_fine_burgers_time_step(model, dataset, opt, batch_size=1, mmpde5=None) -> (df, df_time)   (:88-374)

Both compare three meshes per test sample - the uniform grid, the classical MMPDE5 mesh and the model's mesh - by the mean
square difference between the mesh's Burgers solution and the fine mesh's on the evaluation lattice.  The one-step table
does `opt['num_time_steps']` FEM steps from the initial state; the rollout does `num_eval_time_steps - 1` outer steps of
`num_time_steps` FEM steps each and moves the two adapted meshes after every outer step: the classical one by MMPDE5 with a
monitor from the fine solution's second derivative, the model's by calling the model on the evolved coefficients.  The
state is carried to the new mesh by the not-a-knot cubic spline of (old mesh, coefficients) (`spline.cubic_spline_1d`,
scipy's `UnivariateSpline(s=0)` in the reference).

Everything runs batched: `batch_size` samples advance together through every stage, every FEM stage is one `burgers_1d`
call, every spline stage one `cubic_spline_1d` call, every relaxation one `mmpde5_batch` call.  A sample's row does not
depend on its batch.  There is no CPU fallback.
"""
from __future__ import annotations

import time
import warnings
from typing import List, Optional, Sequence

import torch

from .evaluation import _as_float, _eval_loader, _eval_mode, _picked, _tables, calculate_error_reduction
from .fem1d import burgers_1d, burgers_project
from .mmpde5 import mmpde5_batch, warn_unconverged
from .spline import SPLINE_NOT_FINITE, SPLINE_NOT_INCREASING, SPLINE_OK, cubic_spline_1d

__all__ = ['evaluate_model_fine_burgers', 'evaluate_model_fine_burgers_time_step', 'burgers_project', 'BURGERS_ERROR_COLUMNS',
           'BURGERS_TIME_COLUMNS', 'BURGERS_ROLLOUT_TIME_COLUMNS', 'MMPDE5_DEFAULTS']

BURGERS_ERROR_COLUMNS = ['L2_grid', 'L2_MA', 'L2_MLmodel', 'L2_reduction_MA', 'L2_reduction_MLmodel']
BURGERS_TIME_COLUMNS = ['MA_time', 'MLmodel_time']
BURGERS_ROLLOUT_TIME_COLUMNS = ['MA_time', 'MA_mesh_time', 'MLmodel_time', 'ML_mesh_time']
MMPDE5_DEFAULTS = dict(cfl=0.05, tol=1e-6, max_steps=10000)      # MMPDE5_1d_burgers' own (classical_meshing/ma_mesh_1d.py)


# ------------------------------------------------------------------------------------------------ refusals
def _check(dataset, opt, keys: Sequence[str], what: str):
    if getattr(dataset, 'dim', len(getattr(dataset, 'mesh_dims', [0]))) != 1:
        raise NotImplementedError(f"{what}: 1-D datasets only (the reference has no 2-D Burgers)")
    if opt.get('pde_type', 'Burgers') != 'Burgers':
        raise NotImplementedError(f"{what}: pde_type={opt['pde_type']!r}; 'Burgers' only")
    for k in keys:
        if k not in opt:
            raise ValueError(f"{what}: opt[{k!r}] is missing")
    if int(opt.get('num_time_steps', 1)) < 1:
        raise ValueError(f"{what}: opt['num_time_steps'] >= 1")


def _sync(dev):
    torch.cuda.synchronize(dev)


def _flat(parts: Sequence[torch.Tensor], dev) -> torch.Tensor:
    return torch.cat([p.detach().to(dev, non_blocking=True).float().reshape(-1) for p in parts])


# ------------------------------------------------------------------------------------------------ the one-step table
def _mse_to_fine(coords: Sequence[torch.Tensor], params: Sequence[dict], opt, dev) -> torch.Tensor:
    """[M] mean square difference to the fine solution after num_time_steps steps: the loss of `gradient_meshpoints_1D`
    with grad_type 'burgers_timestep_loss_direct_mse' per mesh, ONE `burgers_1d` call."""
    counts = [int(c.numel()) for c in coords]
    _, sol, fine = burgers_1d(_flat(coords, dev), counts, list(params), opt, int(opt.get('num_time_steps', 1)))
    return ((sol - fine) ** 2).mean(1)


def evaluate_model_fine_burgers(model, dataset, opt, batch_size: int = 1):
    """The reference's one-step Burgers table (`src/utils_eval_Burgers.py:10-86`): (df, df_time), one row per evaluated
    sample, columns BURGERS_ERROR_COLUMNS and BURGERS_TIME_COLUMNS; pandas DataFrames where pandas imports, else dicts of
    numpy arrays with the same keys in the same order.

    Per sample the mean square difference, on linspace(0, 1, eval_quad_points), between the solution after
    `opt['num_time_steps']` steps on the mesh and on the fine mesh - `gradient_meshpoints_1D`'s loss for
    grad_type='burgers_timestep_loss_direct_mse' - on the uniform grid, the sample's `x_phys` and the model's mesh, and
    `calculate_error_reduction` of the last two against the first.

    Where the reference evaluates ONE shared `dataset.mesh_deformed` for every sample, this uses each sample's own `x_phys`
    (the MMPDE5 mesh of its own Gaussians for `MeshDataset(..., target='mmpde5')`): the classical column is then the
    classical mesher's result for that sample, which is what the column is compared with.

    All grid and target meshes go into one `burgers_1d` call and are stored on the sample (`eval_errors_burgers`), so later
    checkpoints pay only for the model's meshes, which go into one more call after the model loop.  Model loop, eval mode,
    `overfit_num`, the 'randg_mix' loader and the timing are `evaluate_model_fine`'s: `MLmodel_time` is the batch's model
    time divided by the batch's size, `MA_time` the sample's (amortised) `build_time` or NaN."""
    what = 'evaluate_model_fine_burgers'
    _check(dataset, opt, ('tau', 'nu', 'num_fine_mesh_points'), what)
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"{what}: batch_size >= 1")
    dev = torch.device(opt.get('device', 'cuda'))
    picked, samples = _picked(dataset, opt)
    missing = [s for s in samples if not isinstance(getattr(s, 'eval_errors_burgers', None), dict)]
    if missing:
        m = len(missing)
        e = _mse_to_fine([s.x_comp for s in missing] + [s.x_phys for s in missing], [s.pde_params for s in missing] * 2, opt, dev).cpu()
        for i, s in enumerate(missing):
            s.eval_errors_burgers = {'L2_grid': e[i], 'L2_MA': e[m + i]}
    coords, times = [], []
    with _eval_mode(model) as stamp, torch.no_grad():
        for data in _eval_loader(dataset, picked, opt, batch_size):
            nb = data.num_graphs
            counts = torch.bincount(data.batch, minlength=nb).tolist()
            data = data.to(dev)
            start = time.time()
            x = model(data)
            times += [(stamp.end_MLmodel - start) / nb] * nb
            coords += [c.clone() for c in torch.split(x.detach().reshape(-1), counts)]
    ml = _mse_to_fine(coords, [s.pde_params for s in samples], opt, dev).cpu().tolist() if samples else []
    rows = {k: [] for k in BURGERS_ERROR_COLUMNS}
    trow = {k: [] for k in BURGERS_TIME_COLUMNS}
    for k, s in enumerate(samples):
        _row(rows, _as_float(s.eval_errors_burgers['L2_grid']), _as_float(s.eval_errors_burgers['L2_MA']), ml[k])
        bt = getattr(s, 'build_time', None)
        trow['MA_time'].append(float('nan') if bt is None else _as_float(bt))
        trow['MLmodel_time'].append(times[k])
    return _tables(rows, trow, BURGERS_ERROR_COLUMNS, BURGERS_TIME_COLUMNS)


def _row(rows, grid: float, ma: float, ml: float):
    for name, v in (('L2_grid', grid), ('L2_MA', ma), ('L2_MLmodel', ml),
                    ('L2_reduction_MA', calculate_error_reduction(grid, ma)),
                    ('L2_reduction_MLmodel', calculate_error_reduction(grid, ml))):
        rows[name].append(v)


# ------------------------------------------------------------------------------------------------ the rollout's stages
# burgers_project, the initial state of every mesh of a batch in one launch, lives beside get_Burgers_initial_coeffs (fem1d.py)
def _steps(x, u, counts, opt, pts):
    """num_time_steps FEM steps from u on every mesh: (coefficients [N], solution at pts [B,P]), one launch."""
    un, sol, _ = burgers_1d(x, counts, None, opt, int(opt.get('num_time_steps', 1)), points=pts, u0=u, fine=False)
    return un, sol


def _monitor(sol_fine, pts, n: int, nf: int, opt):
    """(ms [B,n-1], m2 [B,n]) of `mmpde5_batch` from the fine solution on the lattice [B,P]: m = (mon_reg + (s''/mx)^2)^mon_power
    with s the spline of the lattice values and mx the SIGNED maximum of s'' over linspace(0, 1, num_fine_mesh_points), as
    the reference takes it (`:215-222`; a solution that is concave everywhere would divide by a negative number, squared
    away).  One spline launch for the three query sets."""
    B, P = sol_fine.shape
    dev = sol_fine.device
    q = torch.cat([torch.linspace(0, 1, nf, device=dev), torch.linspace(0, 1, 2 * n - 1, device=dev)[1:2 * n - 1:2],
                   torch.linspace(0, 1, n, device=dev)])
    d2, st = cubic_spline_1d(pts.repeat(B), sol_fine.reshape(-1), [P] * B, q, deriv=2)
    mx = d2[:, :nf].max(1, keepdim=True).values
    m = (float(opt['mon_reg']) + (d2[:, nf:] / mx) ** 2.0) ** float(opt['mon_power'])
    return m[:, :n - 1], m[:, n - 1:], st


def _remesh(x_old, u, x_new, n: int, B: int):
    """The coefficients on the new meshes: the spline of (old mesh, coefficients) at the new nodes, one launch."""
    return cubic_spline_1d(x_old, u, [n] * B, x_new, q_counts=[n] * B)


def _mesh_status(x, n: int):
    """[B] int32 on the device: what the spline will say of these meshes as abscissae (its own rule, without a launch)."""
    x = x.view(-1, n)
    finite = torch.isfinite(x).all(1)
    rising = (x[:, 1:] > x[:, :-1]).all(1)
    return torch.where(finite, torch.where(rising, SPLINE_OK, SPLINE_NOT_INCREASING), SPLINE_NOT_FINITE).to(torch.int32)


def _reference_rollout(samples: List, opt, dev, mm: dict, pts, n: int, nf: int, L: int, statuses: list):
    """The stages that do not depend on the model, for one batch of samples: the uniform grid and the fine mesh, then the
    classical mesh moved by MMPDE5.  Stores `eval_rollout_burgers` on every sample."""
    B = len(samples)
    params = [s.pde_params for s in samples]
    grid = torch.linspace(0, 1, n, device=dev).repeat(B)
    fine = torch.linspace(0, 1, nf, device=dev).repeat(B)
    ev = int(opt.get('eval_quad_points', 101))
    # grid and fine: every outer step one launch over the 2 B meshes
    x = torch.cat([grid, fine])
    u = torch.cat([burgers_project(grid, [n] * B, params, opt), burgers_project(fine, [nf] * B, params, opt, k_proj=10 * ev)])
    counts = [n] * B + [nf] * B
    sol_fine = []
    for _ in range(L):
        u, sol = _steps(x, u, counts, opt, pts)
        sol_fine.append(sol[B:])
    l2_grid = ((sol[:B] - sol[B:]) ** 2).mean(1)
    # the classical mesh
    _sync(dev)
    t0, mesh_time = time.time(), 0.0
    xm = _flat([s.x_phys for s in samples], dev)
    um = burgers_project(xm, [n] * B, params, opt)
    steps, stats = [], []
    for l in range(L):
        um, sol = _steps(xm, um, [n] * B, opt, pts)
        ms, m2, _ = _monitor(sol_fine[l], pts, n, nf, opt)
        _sync(dev)
        t1 = time.time()
        res = mmpde5_batch(list(xm.view(B, n)), [(ms[b], m2[b]) for b in range(B)], **mm)
        _sync(dev)
        mesh_time += time.time() - t1
        x_new = torch.cat(res.coords)
        steps.append(res.steps)
        stats.append(res.status)
        if l < L - 1:                                   # after the last step the mesh still moves (and is timed), the state need not follow
            um, _ = _remesh(xm, um, x_new, n, B)
        xm = x_new
    l2_ma = ((sol - sol_fine[-1]) ** 2).mean(1)
    _sync(dev)
    ma_time = time.time() - t0
    l2_grid, l2_ma = l2_grid.cpu(), l2_ma.cpu()
    steps = torch.stack(steps, 1).cpu() if steps else torch.zeros(B, 0, dtype=torch.int32)
    stats = torch.stack(stats, 1).cpu() if stats else torch.zeros(B, 0, dtype=torch.int32)
    statuses.append(stats)
    for b, s in enumerate(samples):
        s.eval_rollout_burgers = {'L2_grid': l2_grid[b], 'L2_MA': l2_ma[b], 'MA_time': ma_time / B, 'MA_mesh_time': mesh_time / B,
                                  'sol_fine': sol_fine[-1][b].clone(), 'mmpde5_steps': steps[b], 'mmpde5_status': stats[b],
                                  'x_MA': xm.view(B, n)[b].clone()}


def evaluate_model_fine_burgers_time_step(model, dataset, opt, batch_size: int = 1, mmpde5: Optional[dict] = None):
    """The reference's Burgers rollout table (`src/utils_eval_Burgers.py:88-374`): (df, df_time), one row per evaluated
    sample, columns BURGERS_ERROR_COLUMNS and BURGERS_ROLLOUT_TIME_COLUMNS (DataFrames, or dicts of arrays without pandas).

    The initial state gauss_amplitude * u_true is projected on the uniform grid, the fine mesh, the sample's `x_phys` and
    the model's first mesh.  `l` runs over range(num_eval_time_steps - 1) - one outer step fewer than the option's name
    says, as in the reference - and every outer step does `num_time_steps` FEM steps on each mesh, then moves the adapted
    meshes: the classical one by `mmpde5_batch(**mmpde5)` (default cfl=0.05, tol=1e-6, max_steps=10000) from the current
    mesh with the monitor (mon_reg + (s''/mx)^2)^mon_power, s the spline of the fine solution on the lattice and mx the
    signed maximum of s'' over the fine mesh's nodes; the model's by calling the model with `data.uu_tensor` = the
    coefficients and `data.x_phys` = the current mesh.  The coefficients move to the new mesh by the spline of (old mesh,
    coefficients).  `L2_*` is the mean square difference to the fine solution after the last FEM step.  After that step the
    classical mesh is still relaxed (the reference's MA_mesh_time counts it; `x_MA` on the sample is its result), but the
    remesh and the model call, which change no table entry, are not run.

    Kept from the reference: the signed maximum and the num_eval_time_steps - 1 outer steps.  Changed: the classical mesh
    starts from each sample's own `x_phys`, where the reference starts every sample from one shared `dataset.mesh_deformed`.

    A mesh the model tangles (nodes not strictly increasing, or not finite) cannot carry a spline - the reference would
    raise from scipy.  Here the sample gets the spline's status, its `L2_MLmodel` and reduction are NaN, the other samples
    are untouched and ONE RuntimeWarning names the count.  MMPDE5 statuses of the whole call go through `warn_unconverged`
    once.

    The grid, fine and classical rollouts do not depend on the model: their results are stored on the sample
    (`eval_rollout_burgers`: L2_grid, L2_MA, MA_time, MA_mesh_time, the final fine solution, the MMPDE5 step counts and
    statuses per outer step) and a later call with another checkpoint skips them.

    Times are wall times with the device waited for at every stamp.  `MA_time` covers the classical mesh's projection, FEM
    steps, monitors, relaxations and remeshing, `MA_mesh_time` the relaxations alone; `MLmodel_time` the model's first call,
    projection, FEM steps, model calls and remeshing, `ML_mesh_time` the model calls after the first (the reference does not
    count the first either).  All four are the batch's time divided by the batch's size: amortised when `batch_size > 1`.

    Refusals: 2-D datasets and `pde_type` other than 'Burgers' (NotImplementedError); missing `tau`, `nu`,
    `num_fine_mesh_points`, `mon_reg`, `mon_power` (ValueError naming the key).  The `plots_*` options are ignored."""
    what = 'evaluate_model_fine_burgers_time_step'
    _check(dataset, opt, ('tau', 'nu', 'num_fine_mesh_points', 'mon_reg', 'mon_power'), what)
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"{what}: batch_size >= 1")
    L = int(opt.get('num_eval_time_steps', 20)) - 1
    if L < 1:
        raise ValueError(f"{what}: opt['num_eval_time_steps'] >= 2 (it runs num_eval_time_steps - 1 outer steps)")
    mm = dict(MMPDE5_DEFAULTS, **(mmpde5 or {}))
    dev = torch.device(opt.get('device', 'cuda'))
    n, nf = int(dataset.mesh_dims[0]), int(opt['num_fine_mesh_points'])
    pts = torch.linspace(0, 1, int(opt.get('eval_quad_points', 101)), device=dev)
    picked, samples = _picked(dataset, opt)

    statuses: list = []
    with torch.no_grad():
        missing = [s for s in samples if not isinstance(getattr(s, 'eval_rollout_burgers', None), dict)]
        for i in range(0, len(missing), batch_size):
            _reference_rollout(missing[i:i + batch_size], opt, dev, mm, pts, n, nf, L, statuses)
    if statuses:
        warn_unconverged(torch.cat(statuses).reshape(-1), 'MMPDE5 (Burgers rollout)')

    l2_ml, ml_status, ml_time, ml_mesh_time = [], [], [], []
    k = 0
    with _eval_mode(model) as stamp, torch.no_grad():
        for data in _eval_loader(dataset, picked, opt, batch_size):
            B = data.num_graphs
            batch, k = samples[k:k + B], k + B
            params = [s.pde_params for s in batch]
            sol_fine = torch.stack([s.eval_rollout_burgers['sol_fine'] for s in batch]).to(dev)
            grid = torch.linspace(0, 1, n, device=dev).repeat(B)
            data = data.to(dev)
            _sync(dev)
            t0, mesh_time = time.time(), 0.0
            x = model(data).detach().reshape(-1).float().clone()
            status = _mesh_status(x, n)
            x = torch.where((status != SPLINE_OK).repeat_interleave(n), grid, x)     # a flagged sample walks on the grid; its row is NaN
            u = burgers_project(x, [n] * B, params, opt)
            for l in range(L):
                u, sol = _steps(x, u, [n] * B, opt, pts)
                if l == L - 1:
                    break
                data.uu_tensor = u.reshape(data.uu_tensor.shape) if getattr(data, 'uu_tensor', None) is not None else u
                data.x_phys = x.reshape(data.x_phys.shape)
                _sync(dev)
                t1 = time.time()
                x_new = model(data).detach().reshape(-1).float().clone()
                mesh_time += stamp.end_MLmodel - t1
                st = _mesh_status(x_new, n)
                status = torch.where(status != SPLINE_OK, status, st)
                x_new = torch.where((status != SPLINE_OK).repeat_interleave(n), grid, x_new)
                u, _ = _remesh(x, u, x_new, n, B)
                x = x_new
            l2 = ((sol - sol_fine) ** 2).mean(1)
            l2 = torch.where(status != SPLINE_OK, torch.full_like(l2, float('nan')), l2)
            _sync(dev)
            total = time.time() - t0
            l2_ml.append(l2)
            ml_status.append(status)
            ml_time += [total / B] * B
            ml_mesh_time += [mesh_time / B] * B
    l2_ml = torch.cat(l2_ml).cpu().tolist() if l2_ml else []
    ml_status = torch.cat(ml_status).cpu().tolist() if ml_status else []
    bad = sum(1 for s in ml_status if s != SPLINE_OK)
    if bad:
        warnings.warn(f"{what}: the model's mesh is not strictly increasing (or not finite) for {bad} of {len(samples)} samples; "
                      "their L2_MLmodel is NaN", RuntimeWarning, stacklevel=2)
    rows = {c: [] for c in BURGERS_ERROR_COLUMNS}
    trow = {c: [] for c in BURGERS_ROLLOUT_TIME_COLUMNS}
    for i, s in enumerate(samples):
        e = s.eval_rollout_burgers
        e['ML_status'] = ml_status[i]
        _row(rows, _as_float(e['L2_grid']), _as_float(e['L2_MA']), l2_ml[i])
        for c, v in (('MA_time', e['MA_time']), ('MA_mesh_time', e['MA_mesh_time']), ('MLmodel_time', ml_time[i]),
                     ('ML_mesh_time', ml_mesh_time[i])):
            trow[c].append(float(v))
    return _tables(rows, trow, BURGERS_ERROR_COLUMNS, BURGERS_ROLLOUT_TIME_COLUMNS)
