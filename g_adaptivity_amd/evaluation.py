"""How much does an adapted mesh reduce the FEM error?  The reference's headline evaluation, MI355X-native.

`evaluate_model_fine` (`src/utils_eval.py:106-267`) solves Poisson on three meshes per test sample - the uniform grid, the
classical (MMPDE5 / Monge-Ampere) target and the model's mesh - interpolates each solution to a fine uniform lattice, takes
trapezium L1 and L2 errors against the analytic solution and tabulates the percentage error reduction of the classical
mesher and of the model, with the model's time per sample.  This is the reference's Firedrake-free branch
(`opt['solver'] == 'torch_FEM'`, `opt['evaler'] == 'analytical'`, `:221-225, :390-405`).

    poisson_eval_errors(x, node_counts, pde_params, n_eval, cells=..., boundary=...) -> (L1 [B], L2 [B])
    eval_grid_MMPDE_MA(dataset_or_batch, opt) -> {'L1_grid', 'L2_grid', 'L1_MA', 'L2_MA'}: [S] each, stored on the samples
    evaluate_model_fine(model, dataset, opt, fine_eval=True, batch_size=1) -> (df, df_time)
    evaluate_error_np, evaluate_error_np_2d, calculate_error_reduction: the reference's host helpers, plain numpy

`poisson_eval_errors` is one call into `libgadapt_fem.so` for any number of meshes: in 2-D the load vector and banded
Cholesky launches of `fem_poisson`, then the lattice evaluation fused with the reduction of the two norms and a last launch
that adds each mesh's chunk partials (`gadapt_fem_eval_errors`, four launches); in 1-D one launch, one workgroup per mesh
(`gadapt_fem1d_poisson_eval_errors`).  The solution on the lattice is never written to memory and nothing waits for the
device.  forward='wave' (opt['fem_forward'] = 'wave' for `evaluate_model_fine` and `eval_grid_MMPDE_MA`; band 'lds') runs the
wave-parallel load vector and evaluation of `fem_poisson(forward='wave')` instead, five launches with the solution written to a
workspace (`gadapt_fem_eval_errors_wave`): the same norms, bit for bit.  A mesh's pair of norms does not depend on what else is in the batch.  The 1-D launch assembles its stiffness matrix
in fp64 (the fp32 matrix of `fem_poisson_1d` moves these norms by up to 3e-4: docs/measurements.md), the rest is that forward.

Limits: `solver='torch_FEM'` with `evaler='analytical'` only (the others need Firedrake); `fine_eval=True` only; the FEM
tail's mesh sizes (2-D: square meshes up to 26 x 26 nodes, or up to 81 x 81 with opt['fem_band'] = 'window', the windowed
band solve of `poisson_eval_errors(band='window')`; the load vector's built Simpson rule; 1-D: 1024 nodes).
"""
from __future__ import annotations

import contextlib
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native_fem as _nf
from ._native import NativeError, current_stream
from .fem import ENTRY_POINTS, _check_forward, _check_route, _solve_tail, _topology, _tri_counts, pack_gaussians, simpson_points_per_dim
from .fem1d import _Batch, _split_params, _watch_flags
from .mesh_graph import MeshData, MeshLoader, Mixed_DataLoader

__all__ = ['poisson_eval_errors', 'eval_lattice', 'eval_grid_MMPDE_MA', 'evaluate_model_fine', 'evaluate_error_np',
           'evaluate_error_np_2d', 'calculate_error_reduction', 'ERROR_COLUMNS', 'TIME_COLUMNS', 'call_stats']

ERROR_COLUMNS = ['L1_grid', 'L2_grid', 'L1_MA', 'L2_MA', 'L1_MLmodel', 'L2_MLmodel', 'L1_reduction_MA', 'L2_reduction_MA',
                 'L1_reduction_MLmodel', 'L2_reduction_MLmodel']
TIME_COLUMNS = ['MA_time', 'MLmodel_time']

# calls of poisson_eval_errors and the meshes they carried (what a repeated evaluation saves is read off here)
call_stats = {'calls': 0, 'meshes': 0}


# ------------------------------------------------------------------------------------------------ the host helpers
def evaluate_error_np(uu, u_true, x):
    """Trapezium L1 and L2 norms of uu - u_true over the points x [P] (`src/utils_eval.py:32-44`): (L1, L2)."""
    dx = np.diff(x)
    local_L2 = ((uu - u_true) ** 2)[1:] + ((uu - u_true) ** 2)[:-1]
    local_L1 = np.abs(uu - u_true)[1:] + np.abs(uu - u_true)[:-1]
    return np.sum(local_L1 * dx) / 2, np.sqrt(np.sum(local_L2 * dx) / 2)


def evaluate_error_np_2d(uu, u_true, x):
    """Trapezium L1 and L2 norms on the grid x = [X, Y] of np.meshgrid(xs, ys) (`src/utils_eval.py:46-65`): every cell gives
    dx dy / 4 of each of its four corner values: (L1, L2)."""
    dx = np.diff(x[0], axis=1)[:-1, :]
    dy = np.diff(x[1], axis=0)[:, :-1]
    error = uu.reshape(x[0].shape) - u_true.reshape(x[0].shape)
    sq, ab = error ** 2, np.abs(error)
    local_L2 = sq[:-1, 1:] + sq[1:, :-1] + sq[1:, 1:] + sq[:-1, :-1]
    local_L1 = ab[:-1, 1:] + ab[1:, :-1] + ab[1:, 1:] + ab[:-1, :-1]
    return np.sum(local_L1 * dx * dy) / 4, np.sqrt(np.sum(local_L2 * dx * dy) / 4)


def calculate_error_reduction(e_initial, e_adapted):
    """Percentage change of the error, negative when the adapted mesh is better; None when e_adapted is 0 (as the reference)."""
    if e_adapted == 0.:
        return None
    return (e_adapted - e_initial) / e_initial * 100


# ------------------------------------------------------------------------------------------------ the fused call
def eval_lattice(n_eval: int) -> torch.Tensor:
    """One axis of the fine lattice, as the reference builds it: np.linspace(0, 1, n_eval) (`utils_eval.py:119-120`), fp64."""
    return torch.from_numpy(np.linspace(0, 1, int(n_eval)))


def _require_gpu(t, what: str):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise NativeError(f"{what}: the FEM tail runs on the MI355X only (got a "
                          f"{t.device if torch.is_tensor(t) else type(t).__name__} tensor); there is no CPU fallback")


def poisson_eval_errors(x: torch.Tensor, node_counts: Sequence[int], pde_params: Sequence[dict], n_eval: int, *,
                        cells: Optional[torch.Tensor] = None, boundary: Optional[torch.Tensor] = None,
                        tri_counts: Optional[Sequence[int]] = None, opt: Optional[dict] = None, band: str = 'lds',
                        tri_slab: int = 0, forward: str = 'lane') -> Tuple[torch.Tensor, torch.Tensor]:
    """(L1 [B], L2 [B]) on the device: per mesh, the P1 Poisson solve with its own Gaussians, expanded on the lattice
    linspace(0, 1, n_eval) per dimension, and the trapezium norms of sol - u_true there.

    x [N,2]: 2-D meshes, concatenated; cells [T,3] (global node ids, mesh by mesh), boundary [N] and tri_counts as
    `fem_poisson` takes them, its topology cache reused.  x [N] or [N,1]: 1-D meshes; opt supplies load_quad_points /
    stiff_quad_points as `fem_poisson_1d` reads them.  In 2-D opt['load_quad_points'], when given, must map to the built
    Simpson rule.  GPU tensors only; no gradient.

    band (2-D only; 1-D input ignores it): 'lds' keeps each mesh's banded factor resident in LDS (square meshes up to
    26 x 26 nodes); 'window' streams it through a ring of band rows and a global workspace allocated here (fp64, about
    2 MB per 64 x 64 mesh), and takes the triangles in slabs of `tri_slab` ids (a multiple of 32; 0: the largest slab the
    LDS budget leaves): square meshes up to 81 x 81 nodes.  The windowed route factors and substitutes in fp64 and evaluates
    the load vector's forcing in fp64 (fp32 missed the evaluation's accuracy rule from 27 x 27 on), so where both routes take
    a mesh their norms agree to the fp32 rounding of those, not bitwise; the result does not depend on `tri_slab`, bit for bit.

    forward (2-D only; 1-D input does not read it): 'lane' is the four launches above.  'wave' (band='lds' only; with
    band='window' a ValueError) runs the load vector with a wave per node and the evaluation with a wave per chunk of the
    lattice (`fem_poisson(forward='wave')`) into a workspace allocated here (4 * n_eval^2 bytes a mesh: on this route the
    solution on the lattice does reach memory), then the lane route's reduction reading it: five launches
    (`gadapt_fem_eval_errors_wave`), and the same L1 and L2, bit for bit."""
    if torch.is_tensor(x) and x.dim() == 2 and x.shape[1] == 2:
        _check_forward('poisson_eval_errors', forward, band)
    _require_gpu(x, 'poisson_eval_errors')
    opt = opt or {}
    tri_slab = _check_route('poisson_eval_errors', band, tri_slab)
    n_eval = int(n_eval)
    if n_eval < 2:
        raise ValueError(f"poisson_eval_errors: {n_eval} lattice points per dimension; at least 2")
    x = x.detach().float()
    dev, B = x.device, len(node_counts)
    lib = _nf.lib()
    lat = eval_lattice(n_eval).to(device=dev, dtype=torch.float32)
    err = torch.empty(B, 2, device=dev)
    stream = current_stream(dev)
    if x.dim() == 2 and x.shape[1] == 2:
        if cells is None or boundary is None:
            raise ValueError("poisson_eval_errors: 2-D meshes need cells [T,3] and boundary [N]")
        n_built = int(lib.gadapt_fem_simpson_points())
        if 'load_quad_points' in opt and simpson_points_per_dim(opt['load_quad_points']) != n_built:
            raise NotImplementedError(f"poisson_eval_errors: load_quad_points={opt['load_quad_points']} asks for a "
                                      f"{simpson_points_per_dim(opt['load_quad_points'])}-point Simpson rule per dimension; the load "
                                      f"vector is built for {n_built} points only")
        x = x.contiguous()
        if tri_counts is None:
            tri_counts = _tri_counts(cells, node_counts)
        topo = _topology(cells, boundary, node_counts, tri_counts, dev, band)  # refuses meshes beyond the route's LDS budget
        if topo.n_nodes != x.shape[0]:
            raise ValueError(f"poisson_eval_errors: {x.shape[0]} coordinates for {topo.n_nodes} nodes")
        gptr, gpar = pack_gaussians(pde_params, dev)
        rhs, coeffs = torch.empty(topo.n_nodes, device=dev), torch.empty(topo.n_nodes, device=dev)
        partials = torch.empty(int(lib.gadapt_fem_eval_partials_floats(B)), device=dev)
        work = topo.factor_buffer(dev) if band == 'window' else None           # 'lds': the factor is not kept
        if forward == 'wave':
            sol_work = torch.empty(B * n_eval * n_eval, device=dev)            # the wave evaluation's sol, read by the reduction
            _nf.call(ENTRY_POINTS['eval_errors_wave'][band], *topo.head(gptr, gpar, x, lat, lat, n_eval),
                     *_solve_tail(topo, rhs, coeffs, work, tri_slab), sol_work.data_ptr(), partials.data_ptr(), err.data_ptr(), stream)
        else:
            _nf.call(ENTRY_POINTS['eval_errors'][band], *topo.head(gptr, gpar, x, lat, lat, n_eval),
                     *_solve_tail(topo, rhs, coeffs, work, tri_slab), partials.data_ptr(), err.data_ptr(), stream)
    elif x.dim() == 1 or (x.dim() == 2 and x.shape[1] == 1):
        x = x.reshape(-1).contiguous()
        if sum(int(n) for n in node_counts) != x.shape[0]:
            raise ValueError(f"poisson_eval_errors: {x.shape[0]} coordinates for node_counts summing to {sum(node_counts)}")
        bt = _Batch(node_counts, pde_params, dev)                              # refuses meshes beyond 1024 nodes
        if min(bt.counts) < 3:
            raise ValueError("poisson_eval_errors: every 1-D mesh needs at least 3 nodes")
        flags = torch.empty(B, dtype=torch.int32, device=dev)
        _nf.call('gadapt_fem1d_poisson_eval_errors', *bt.head(x), int(opt.get('load_quad_points', 101)),
                 int(opt.get('stiff_quad_points', 3)), n_eval, lat.data_ptr(), err.data_ptr(), flags.data_ptr(), stream)
        _watch_flags(flags)
    else:
        raise ValueError(f"poisson_eval_errors: x must be [N,2] (2-D) or [N] / [N,1] (1-D), got {tuple(x.shape)}")
    call_stats['calls'] += 1
    call_stats['meshes'] += B
    return err[:, 0], err[:, 1]


# ------------------------------------------------------------------------------------------------ the evaluation
def _check_opt(opt, fine_eval: bool = True) -> int:
    """The refusals of what is out of scope; returns eval_quad_points."""
    solver, evaler = opt.get('solver', 'torch_FEM'), opt.get('evaler', 'analytical')
    if solver == 'firedrake':
        raise NotImplementedError("evaluation: solver='firedrake' needs Firedrake for the coarse solves; only solver='torch_FEM' is built")
    if solver != 'torch_FEM':
        raise ValueError(f"evaluation: solver={solver!r}; 'torch_FEM' (or the unbuilt 'firedrake')")
    if evaler == 'fd_*':
        raise NotImplementedError("evaluation: evaler='fd_*' needs Firedrake for the fine reference solve; only evaler='analytical' is built")
    if evaler != 'analytical':
        raise ValueError(f"evaluation: evaler={evaler!r}; 'analytical' (or the unbuilt 'fd_*')")
    if not fine_eval:
        raise NotImplementedError("evaluation: fine_eval=False evaluates at the deformed nodes themselves, not on a uniform lattice, "
                                  "which the evaluation kernel's bin mask does not support; only fine_eval=True is built")
    return int(opt.get('eval_quad_points', 101))


def _samples_of(dataset_or_batch) -> List[MeshData]:
    """The per-mesh samples of a dataset, a list of samples, one sample, or a collated batch (split along its batch vector)."""
    if hasattr(dataset_or_batch, 'samples'):
        return list(dataset_or_batch.samples)
    if isinstance(dataset_or_batch, (list, tuple)):
        return list(dataset_or_batch)
    data = dataset_or_batch
    batch = getattr(data, 'batch', None)
    if batch is None:
        return [data]
    B = data.num_graphs
    counts = torch.bincount(batch.detach().cpu(), minlength=B).tolist()
    if getattr(data, 'batch_dict', None) is not None and all('pde_params' in data.batch_dict[i] for i in range(B)):
        params = [data.batch_dict[i]['pde_params'] for i in range(B)]
    else:
        params = _split_params(data.pde_params, B)
    xc, xp = torch.split(data.x_comp, counts), torch.split(data.x_phys, counts)
    out, cells = [], getattr(data, 'cells', None)
    tri = _tri_counts(cells, counts) if cells is not None else None
    off = np.concatenate([[0], np.cumsum(counts)])
    toff = np.concatenate([[0], np.cumsum(tri)]) if tri is not None else None
    for b in range(B):
        s = MeshData(x_comp=xc[b], x_phys=xp[b], pde_params=params[b])
        if cells is not None:
            s.cells = cells[int(toff[b]):int(toff[b + 1])] - int(off[b])
            s.boundary_nodes = data.boundary_nodes[int(off[b]):int(off[b + 1])]
        out.append(s)
    data.eval_errors = [None] * B
    for b, s in enumerate(out):
        s._owner = (data, b)
    return out


def _errors_of(coords: Sequence[torch.Tensor], samples: Sequence[MeshData], n_eval: int, opt, dev) -> torch.Tensor:
    """[M,2] (L1, L2) of mesh k = coords[k] on the topology and Gaussians of samples[k]: ONE poisson_eval_errors call.
    2-D meshes take the route from opt['fem_band'] and opt['fem_forward'] ('wave' with 'window' is refused before anything moves
    to the device, as by every other reader of the key); 1-D meshes read neither."""
    counts = [int(c.shape[0]) for c in coords]
    band, forward = opt.get('fem_band', 'lds'), opt.get('fem_forward', 'lane')
    if coords[0].dim() == 2 and coords[0].shape[1] == 2:
        _check_forward("evaluation (opt['fem_forward'])", forward, band)
    x = torch.cat([c.detach().to(dev, non_blocking=True).float().reshape(c.shape[0], -1) for c in coords], 0)
    params = [s.pde_params for s in samples]
    if x.shape[1] == 1:
        l1, l2 = poisson_eval_errors(x, counts, params, n_eval, opt=opt)
    else:
        off = np.concatenate([[0], np.cumsum(counts)])
        cells = torch.cat([s.cells.cpu() + int(o) for s, o in zip(samples, off[:-1])], 0)
        boundary = torch.cat([s.boundary_nodes.cpu() for s in samples], 0)
        l1, l2 = poisson_eval_errors(x, counts, params, n_eval, cells=cells, boundary=boundary,
                                     tri_counts=[int(s.cells.shape[0]) for s in samples], opt=opt, band=band,
                                     forward=forward)
    return torch.stack([l1, l2], 1)


def eval_grid_MMPDE_MA(dataset_or_batch, opt) -> Dict[str, torch.Tensor]:
    """The errors of the uniform grid (`x_comp`) and of the classical target mesh (`x_phys`) of every sample
    (`src/utils_eval.py:270-355`): {'L1_grid', 'L2_grid', 'L1_MA', 'L2_MA'}, [S] host tensors, from ONE `poisson_eval_errors`
    call over the 2 S meshes and one copy to the host.

    Each sample also gets `eval_errors`, a dict of 0-dim tensors (what `utils_eval.py:170-176` reads with `.item()`): the
    reference's pre-processed evaluation data, which `evaluate_model_fine` reuses, so that evaluating several checkpoints
    pays for the grid and target meshes once.  For a collated batch the dicts are stored as the list `batch.eval_errors`."""
    n_eval = _check_opt(opt)
    samples = _samples_of(dataset_or_batch)
    dev = torch.device(opt.get('device', 'cuda'))
    S = len(samples)
    err = _errors_of([s.x_comp for s in samples] + [s.x_phys for s in samples], samples + samples, n_eval, opt, dev).cpu()
    out = {'L1_grid': err[:S, 0], 'L2_grid': err[:S, 1], 'L1_MA': err[S:, 0], 'L2_MA': err[S:, 1]}
    for i, s in enumerate(samples):
        s.eval_errors = {k: v[i] for k, v in out.items()}
        owner = s.__dict__.pop('_owner', None)
        if owner is not None:
            owner[0].eval_errors[owner[1]] = s.eval_errors
    return out


def _as_float(v) -> float:
    return float(v.item()) if torch.is_tensor(v) else float(v)


def _picked(dataset, opt):
    """(indices, samples) to evaluate: all, or those opt['overfit_num'] lists."""
    picked = [i for i in range(len(dataset)) if not opt.get('overfit_num') or i in opt['overfit_num']]
    return picked, [dataset[i] for i in picked]


def _eval_loader(dataset, picked, opt, batch_size: int):
    """The evaluation's loader over the picked samples, in order: `Mixed_DataLoader` for data_type 'randg_mix', else `MeshLoader`."""
    sub = dataset[picked]
    if opt.get('data_type') == 'randg_mix':
        exclude = ['boundary_nodes_dict', 'mapping_dict', 'node_boundary_map', 'eval_errors', 'pde_params']
        return Mixed_DataLoader(sub, batch_size=batch_size, shuffle=False, exclude_keys=exclude, follow_batch=[])
    return MeshLoader(sub, batch_size=batch_size, shuffle=False)


@contextlib.contextmanager
def _eval_mode(model):
    """The module that stamps `end_MLmodel` (a GraphedForward stamps its model), in eval mode for the block."""
    stamp = getattr(model, 'model', model)
    was_training = bool(getattr(stamp, 'training', False))
    if hasattr(stamp, 'eval'):
        stamp.eval()
    try:
        yield stamp
    finally:
        if was_training:
            stamp.train()


def _tables(rows, trow, columns, time_columns):
    """(df, df_time): pandas DataFrames where pandas imports, else dicts of numpy arrays (None -> NaN), same keys and order."""
    try:
        import pandas as pd
    except ImportError:
        as_arr = lambda v: np.asarray([np.nan if a is None else a for a in v], dtype=np.float64)
        return {k: as_arr(v) for k, v in rows.items()}, {k: as_arr(v) for k, v in trow.items()}
    return pd.DataFrame(rows, columns=columns), pd.DataFrame(trow, columns=time_columns)


def evaluate_model_fine(model, dataset, opt, fine_eval: bool = True, batch_size: int = 1):
    """The reference's `evaluate_model_fine` (`src/utils_eval.py:106-267`) on the GPU: (df, df_time), one row per evaluated
    sample, columns ERROR_COLUMNS and TIME_COLUMNS.  pandas DataFrames when pandas imports, else dicts of numpy arrays with
    the same keys in the same order.

    Per sample: the errors of the grid and of the classical target (the sample's stored `eval_errors`, computed for the
    samples that lack them by one `eval_grid_MMPDE_MA` call), the errors of the model's mesh (all samples in ONE
    `poisson_eval_errors` call after the model loop) and the four reductions `calculate_error_reduction(e_grid, e)`.

    The model runs in eval mode without gradients through `MeshLoader`, or `Mixed_DataLoader` for
    `opt['data_type'] == 'randg_mix'`; `opt.get('fem_band', 'lds')` picks the FEM route of every `poisson_eval_errors` call
    here and in `eval_grid_MMPDE_MA` ('window': meshes beyond 26 x 26 nodes) and `opt.get('fem_forward', 'lane')` the form of its
    load vector and evaluation ('wave': the wave-parallel kernels, band 'lds' only, the same columns bit for bit); `loss_type` 'mesh_loss' and 'modular' return the coordinates, 'pde_loss' the triple
    whose second entry they are.  `opt['overfit_num']`, when set, lists the sample indices to evaluate.  With `batch_size=1`
    the model is called once per sample and `MLmodel_time` is `model.end_MLmodel - start` as in the reference (the forward
    waits for the device before it stamps); with a larger `batch_size` it is the batch's time divided by the batch's size.
    A mesh's errors do not depend on its batch.

    `MA_time`: the sample's `build_time` where it has one, else NaN.  `MeshDataset(..., target='mmpde5')` records the wall
    time of its batched MMPDE5 call (all samples in one launch sequence, device waited for) divided by the sample count: an
    amortised figure, not the time of building one mesh alone.

    Refusals (NotImplementedError): `solver='firedrake'`, `evaler='fd_*'`, `fine_eval=False`, meshes beyond the FEM tail's
    limits."""
    n_eval = _check_opt(opt, fine_eval)
    loss_type = opt.get('loss_type', 'mesh_loss')
    if loss_type not in ('mesh_loss', 'modular', 'pde_loss'):
        raise NotImplementedError(f"evaluate_model_fine: loss_type={loss_type!r}")
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("evaluate_model_fine: batch_size >= 1")
    dev = torch.device(opt.get('device', 'cuda'))
    picked, samples = _picked(dataset, opt)
    missing = [s for s in samples if not isinstance(getattr(s, 'eval_errors', None), dict)]
    if missing:
        print("Pre process eval data doesn't exists, calculating...")
        eval_grid_MMPDE_MA(missing, opt)

    loader = _eval_loader(dataset, picked, opt, batch_size)
    coords, times = [], []
    with _eval_mode(model) as stamp, torch.no_grad():
        for data in loader:
            nb = data.num_graphs
            counts = torch.bincount(data.batch, minlength=nb).tolist()
            data = data.to(dev)
            start = time.time()
            out = model(data)
            x = out[1] if loss_type == 'pde_loss' else out
            times += [(stamp.end_MLmodel - start) / nb] * nb
            coords += list(torch.split(x.detach(), counts))
    ml = _errors_of(coords, samples, n_eval, opt, dev).cpu().double().numpy() if samples else np.zeros((0, 2))

    rows = {k: [] for k in ERROR_COLUMNS}
    trow = {k: [] for k in TIME_COLUMNS}
    for k, s in enumerate(samples):
        e = {name: _as_float(v) for name, v in s.eval_errors.items()}
        e['L1_MLmodel'], e['L2_MLmodel'] = float(ml[k, 0]), float(ml[k, 1])
        for n in ('L1', 'L2'):
            e[f'{n}_reduction_MA'] = calculate_error_reduction(e[f'{n}_grid'], e[f'{n}_MA'])
            e[f'{n}_reduction_MLmodel'] = calculate_error_reduction(e[f'{n}_grid'], e[f'{n}_MLmodel'])
        for name in ERROR_COLUMNS:
            rows[name].append(e[name])
        bt = getattr(s, 'build_time', None)
        trow['MA_time'].append(float('nan') if bt is None else _as_float(bt))
        trow['MLmodel_time'].append(times[k])
    return _tables(rows, trow, ERROR_COLUMNS, TIME_COLUMNS)
