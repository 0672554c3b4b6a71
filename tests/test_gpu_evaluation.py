"""The Poisson error-reduction evaluation on the MI355X (g_adaptivity_amd/evaluation.py, gadapt_fem_eval_errors /
gadapt_fem1d_poisson_eval_errors in libgadapt_fem.so) against the test-side yardstick (tests/eval_restatement.py).

The rule for a norm of e = sol - u_true (tests/test_gpu_modular2d.py, LOSS_FLOOR): relative deviation from the fp64
yardstick <= max(2e-4, 1.5 x the fp32 yardstick's own deviation from fp64), L1 and L2 separately.  Every figure is printed
before it is asserted (run with -s to collect them)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_restatement as E  # noqa: E402
from test_gpu_modular2d import LOSS_FLOOR, _coords, _params  # noqa: E402  (the mesh and Gaussian recipes, the floor)

from g_adaptivity_amd import (GNN, MeshDataset, MixedMeshDataset, collate, eval_grid_MMPDE_MA, evaluate_model_fine, fem_poisson,  # noqa: E402
                              hot_path_opt, poisson_eval_errors)
from g_adaptivity_amd import evaluation as ev  # noqa: E402
from g_adaptivity_amd.mesh_graph import square_mesh  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
N_EVAL = 101
OPT1D = {'load_quad_points': 101, 'stiff_quad_points': 3}

_yard = {}                                                # (coords, Gaussians, dtype) -> (L1, L2): a mesh is solved once per session


def _yard2d(x, m, p, dtype):
    key = (x.numpy().tobytes(), np.concatenate(p['centers'] + p['scales']).tobytes(), dtype)
    if key not in _yard:
        _yard[key] = E.errors_2d(x, m.cells, m.boundary_nodes, p['centers'], p['scales'], N_EVAL, dtype)
    return _yard[key]


def _yard1d(x, p, dtype):
    key = (x.numpy().tobytes(), np.concatenate(p['centers'] + p['scales']).tobytes(), dtype)
    if key not in _yard:
        _yard[key] = E.errors_1d(x, p['centers'], p['scales'], OPT1D, N_EVAL, dtype)
    return _yard[key]


def _check(label, got, e64, e32):
    """The rule above for one (L1, L2) pair."""
    for name, g, r64, r32 in zip(('L1', 'L2'), got, e64, e32):
        dev, own = E.rel(g, r64), E.rel(r32, r64)
        print(f"EVAL-DEV {label} {name}: gpu {g:.9e} fp64 {r64:.9e} dev {dev:.3e} fp32-yardstick dev {own:.3e}")
        assert dev <= max(LOSS_FLOOR, 1.5 * own), (label, name, dev, own)


def _gpu2d(x, m, p):
    l1, l2 = poisson_eval_errors(x.to(DEV), [m.num_nodes], [p], N_EVAL, cells=m.cells, boundary=m.boundary_nodes)
    return float(l1.item()), float(l2.item())


# ------------------------------------------------------------------------------------------------ 1. the fused call, 2-D
@pytest.mark.one_dispatch
@pytest.mark.parametrize('kind', ['unmoved', 'jittered'])
@pytest.mark.parametrize('n', [7, 11, 15, 23])
def test_errors_2d_against_yardstick(n, kind):
    x, m = _coords(n, kind, seed=n + 1)
    p = _params(2, n)
    _check(f"2d n={n} {kind}", _gpu2d(x, m, p), _yard2d(x, m, p, torch.float64), _yard2d(x, m, p, torch.float32))


@pytest.mark.parametrize('n', [7, 11, 15, 23])
def test_errors_2d_gnn_moved_against_yardstick(n):
    x, m = _coords(n, 'gnn_moved', seed=n + 1)             # builds a message-passing graph: run under both dispatches
    p = _params(2, n)
    _check(f"2d n={n} gnn_moved", _gpu2d(x, m, p), _yard2d(x, m, p, torch.float64), _yard2d(x, m, p, torch.float32))


# ------------------------------------------------------------------------------------------------ 2. the fused call, 1-D
def _mesh1d(n, kind):
    u = torch.linspace(0, 1, n)
    if kind == 'jittered':                                 # monotone: a node moves by less than half a cell
        g = torch.Generator().manual_seed(n)
        u = u + (torch.rand(n, generator=g) * 2 - 1) * 0.3 / (n - 1)
        u[0], u[-1] = 0.0, 1.0
    return u


def _params1d(seed, k=2):
    rng = np.random.default_rng(seed)
    return {'centers': [rng.uniform(0.2, 0.8, 1).astype('f') for _ in range(k)],
            'scales': [rng.uniform(0.1, 0.4, 1).astype('f') for _ in range(k)]}


@pytest.mark.one_dispatch
@pytest.mark.parametrize('kind', ['unmoved', 'jittered'])
@pytest.mark.parametrize('n', [21, 64])
def test_errors_1d_against_yardstick(n, kind):
    x, p = _mesh1d(n, kind), _params1d(n)
    l1, l2 = poisson_eval_errors(x.to(DEV), [n], [p], N_EVAL, opt=OPT1D)
    col = poisson_eval_errors(x.to(DEV).unsqueeze(1), [n], [p], N_EVAL, opt=OPT1D)        # [N,1] is the same mesh
    assert torch.equal(col[0], l1) and torch.equal(col[1], l2)
    _check(f"1d n={n} {kind}", (l1.item(), l2.item()), _yard1d(x, p, torch.float64), _yard1d(x, p, torch.float32))


@pytest.mark.one_dispatch
def test_errors_1d_mixed_batch_bitwise():
    sizes = [21, 64, 33, 130]
    xs, ps = [_mesh1d(n, 'jittered') for n in sizes], [_params1d(n, k=1 + i) for i, n in enumerate(sizes)]
    l1, l2 = poisson_eval_errors(torch.cat(xs).to(DEV), sizes, ps, N_EVAL, opt=OPT1D)
    for b, (x, p) in enumerate(zip(xs, ps)):
        a1, a2 = poisson_eval_errors(x.to(DEV), [sizes[b]], [p], N_EVAL, opt=OPT1D)
        assert torch.equal(l1[b:b + 1], a1) and torch.equal(l2[b:b + 1], a2), b


# ------------------------------------------------------------------------------------------------ 3. one mixed batch
def _mixed_batch():
    sizes, gauss = [12, 23, 17, 14], [1, 6, 3, 2]
    xs, ms = zip(*[_coords(n, 'jittered', seed=n) for n in sizes])
    ps = [_params(k, 40 + k) for k in gauss]
    offs = np.cumsum([0] + [m.num_nodes for m in ms[:-1]])
    cells = torch.cat([m.cells + int(o) for m, o in zip(ms, offs)], 0)
    bnd = torch.cat([m.boundary_nodes for m in ms])
    return xs, ms, ps, cells, bnd


@pytest.mark.one_dispatch
def test_mixed_batch_bitwise_equal_to_single_mesh_calls():
    xs, ms, ps, cells, bnd = _mixed_batch()
    counts = [m.num_nodes for m in ms]
    x = torch.cat(xs).to(DEV)
    l1, l2 = poisson_eval_errors(x, counts, ps, N_EVAL, cells=cells, boundary=bnd)
    r1, r2 = poisson_eval_errors(x, counts, ps, N_EVAL, cells=cells, boundary=bnd)
    assert torch.equal(l1, r1) and torch.equal(l2, r2)                               # repeatable
    assert l1.shape == (4,) and l1.device == x.device and bool(torch.isfinite(l1).all() and torch.isfinite(l2).all())
    for b, (xb, m, p) in enumerate(zip(xs, ms, ps)):
        a1, a2 = poisson_eval_errors(xb.to(DEV), [m.num_nodes], [p], N_EVAL, cells=m.cells, boundary=m.boundary_nodes)
        assert torch.equal(l1[b:b + 1], a1) and torch.equal(l2[b:b + 1], a2), b


# ------------------------------------------------------------------------------------------------ 4. the existing path
@pytest.mark.one_dispatch
def test_consistent_with_fem_poisson_sol():
    """L1 / L2 in fp64 on the host from fem_poisson's sol of the same meshes: the per-point sol is the same arithmetic, only
    the fp32 summation of 10 201 weighted terms differs (about sqrt(10201) 6e-8 = 6e-6 for a fixed-tree sum): 1e-5."""
    xs, ms, ps, cells, bnd = _mixed_batch()
    unmoved = square_mesh(11)
    xs, ms, ps = list(xs) + [unmoved.x_comp], list(ms) + [unmoved], ps + [_params(2, 3)]
    cells = torch.cat([cells, unmoved.cells + cells.max() + 1], 0)
    bnd = torch.cat([bnd, unmoved.boundary_nodes])
    counts = [m.num_nodes for m in ms]
    x = torch.cat(xs).to(DEV)
    lat = ev.eval_lattice(N_EVAL).float()
    l1, l2 = poisson_eval_errors(x, counts, ps, N_EVAL, cells=cells, boundary=bnd)
    _, sol = fem_poisson(x, cells, bnd, counts, ps, [lat, lat])
    sol = sol.cpu().double().view(len(ms), N_EVAL * N_EVAL)
    ax = lat.double()
    X, Y = torch.meshgrid(ax, ax, indexing='ij')
    pts = torch.stack([X.reshape(-1), Y.reshape(-1)], 0)
    for b, p in enumerate(ps):
        w1, w2 = E.trapezium_2d(sol[b], E.R2.u_true(pts, p['centers'], p['scales']), ax)
        d1, d2 = E.rel(l1[b].item(), float(w1)), E.rel(l2[b].item(), float(w2))
        print(f"EVAL-SUM mesh {b} ({counts[b]} nodes): L1 dev {d1:.3e} L2 dev {d2:.3e}")
        assert d1 <= 1e-5 and d2 <= 1e-5, (b, d1, d2)


# ------------------------------------------------------------------------------------------------ 5. end to end
def _opt(dims, loss_type, **kw):
    return hot_path_opt(mesh_dims=dims, hidden_dim=8, num_layers=4, time_step=0.1, loss_type=loss_type, device=str(DEV),
                        load_quad_points=101, eval_quad_points=N_EVAL, **kw)


class _Recording:
    """The model, with the coordinates of every call kept (the yardstick takes the GPU model's meshes, it does not re-derive
    them)."""

    def __init__(self, model):
        self.model, self.calls = model, []

    def __call__(self, data):
        out = self.model(data)
        x = out[1] if isinstance(out, tuple) else out
        self.calls.append((x.detach().cpu(), data.num_graphs))
        return out


def _train(model, ds, steps=10):
    model.train()
    optim = torch.optim.Adam(model.parameters(), lr=1e-2)
    dd = collate(ds.samples).to(DEV)
    for _ in range(steps):
        optim.zero_grad()
        out = model(dd)
        F.mse_loss(out.view_as(dd.x_phys), dd.x_phys).backward()
        optim.step()
    return model.eval()


def _columns_against_yardstick(label, df, samples, ml_coords, dim):
    for k, s in enumerate(samples):
        for col, x in (('grid', s.x_comp), ('MA', s.x_phys), ('MLmodel', ml_coords[k])):
            if dim == 2:
                m = square_mesh(int(round(x.shape[0] ** 0.5)))
                e64, e32 = _yard2d(x, m, s.pde_params, torch.float64), _yard2d(x, m, s.pde_params, torch.float32)
            else:
                x = x.reshape(-1)
                e64, e32 = _yard1d(x, s.pde_params, torch.float64), _yard1d(x, s.pde_params, torch.float32)
            got = (float(np.asarray(df[f'L1_{col}'])[k]), float(np.asarray(df[f'L2_{col}'])[k]))
            _check(f"{label} sample {k} {col}", got, e64, e32)
        for n in ('L1', 'L2'):
            g = float(np.asarray(df[f'{n}_grid'])[k])
            for col in ('MA', 'MLmodel'):
                e = float(np.asarray(df[f'{n}_{col}'])[k])
                assert float(np.asarray(df[f'{n}_reduction_{col}'])[k]) == (e - g) / g * 100


def _end_to_end(label, ds, opt, train, dim):
    torch.manual_seed(0)
    model = GNN(ds, opt).to(DEV)
    if train:
        _train(model, ds)
    model.eval()
    S = len(ds)
    before = dict(ev.call_stats)
    stored = eval_grid_MMPDE_MA(ds, opt)
    assert ev.call_stats['calls'] == before['calls'] + 1 and ev.call_stats['meshes'] == before['meshes'] + 2 * S
    assert all(s.eval_errors['L1_grid'].dim() == 0 for s in ds.samples)
    rec1 = _Recording(model)
    df, dt = evaluate_model_fine(rec1, ds, opt)                                  # reuses the stored eval_errors:
    assert ev.call_stats['calls'] == before['calls'] + 2 and ev.call_stats['meshes'] == before['meshes'] + 3 * S   # S model meshes only
    assert [n for _, n in rec1.calls] == [1] * S                                 # batch_size=1: one call per sample
    assert list(df.keys()) == ev.ERROR_COLUMNS and list(dt.keys()) == ev.TIME_COLUMNS
    for k in ('L1_grid', 'L2_grid', 'L1_MA', 'L2_MA'):
        assert np.array_equal(np.asarray(df[k], dtype=np.float64), stored[k].double().numpy())
    t = np.asarray(dt['MLmodel_time'], dtype=float)
    print(f"EVAL-TIME {label}: MLmodel_time median {np.median(t) * 1e6:.1f} us, MA_time {np.asarray(dt['MA_time'], dtype=float)[0]}")
    assert (t > 0).all() and (t < 5.0).all()
    _columns_against_yardstick(label, df, ds.samples, [x for x, _ in rec1.calls], dim)
    rec3 = _Recording(model)
    df3, dt3 = evaluate_model_fine(rec3, ds, opt, batch_size=3)
    assert [n for _, n in rec3.calls] == [3] * (S // 3)
    for k in ev.ERROR_COLUMNS:
        assert np.array_equal(np.asarray(df3[k], dtype=np.float64), np.asarray(df[k], dtype=np.float64), equal_nan=True), k
    return df, dt


def test_evaluate_model_fine_mesh_loss_mmpde5():
    ds = MeshDataset([11, 11], 6, seed=0, target='mmpde5')
    opt = _opt([11, 11], 'mesh_loss')
    df, dt = _end_to_end('mesh_loss', ds, opt, train=True, dim=2)
    ma = np.asarray(dt['MA_time'], dtype=float)
    assert np.isfinite(ma).all() and (ma > 0).all()                              # the batched MMPDE5 call's time, shared out
    # No assertion that L2_MA < L2_grid: the fp64 yardstick on the CPU MMPDE5 restatement's meshes (tests/mmpde5_restatement.py,
    # default monitor) of these six samples gives it for five of them only - sample 0: L2 9.994e-3 on the grid, 1.0493e-2 on
    # the target (its two Gaussians are wide, the grid already resolves them); samples 1-5 fall by 7 to 32 %.


@pytest.mark.parametrize('loss_type', ['modular', 'pde_loss'])
def test_evaluate_model_fine_other_loss_types(loss_type):
    ds = MeshDataset([11, 11], 3, seed=0, target='mmpde5')
    kw = {'grad_type': 'PDE_loss_direct_mse'} if loss_type == 'modular' else {'loss_fn': 'l1'}
    _end_to_end(loss_type, ds, _opt([11, 11], loss_type, **kw), train=False, dim=2)


def test_evaluate_model_fine_1d():
    ds = MeshDataset([21], 3, seed=2, target='mmpde5')
    _end_to_end('1d', ds, _opt([21], 'mesh_loss'), train=True, dim=1)


def test_overfit_num_and_precomputed_errors():
    ds = MeshDataset([11, 11], 4, seed=5)
    opt = _opt([11, 11], 'mesh_loss', overfit_num=[1, 3])
    torch.manual_seed(0)
    model = GNN(ds, opt).to(DEV).eval()
    before = dict(ev.call_stats)
    df, dt = evaluate_model_fine(model, ds, opt)
    assert len(df['L1_grid']) == 2 and ev.call_stats['meshes'] == before['meshes'] + 2 * 2 + 2    # grid + target, then the model
    assert hasattr(ds.samples[1], 'eval_errors') and not hasattr(ds.samples[0], 'eval_errors')
    assert np.isnan(np.asarray(dt['MA_time'], dtype=float)).all()                 # target='noise' records no build time
    full, _ = evaluate_model_fine(model, ds, dict(opt, overfit_num=None))
    assert np.array_equal(np.asarray(full['L2_MLmodel'], dtype=float)[[1, 3]], np.asarray(df['L2_MLmodel'], dtype=float))


@pytest.mark.one_dispatch
def test_limits():
    m = square_mesh(30)
    with pytest.raises(NotImplementedError, match='LDS'):
        poisson_eval_errors(m.x_comp.to(DEV), [900], [_params(1, 0)], N_EVAL, cells=m.cells, boundary=m.boundary_nodes)
    m = square_mesh(7)
    with pytest.raises(NotImplementedError, match='Simpson'):
        poisson_eval_errors(m.x_comp.to(DEV), [49], [_params(1, 0)], N_EVAL, cells=m.cells, boundary=m.boundary_nodes,
                            opt={'load_quad_points': 51})
    with pytest.raises(NotImplementedError, match='1024'):
        poisson_eval_errors(torch.linspace(0, 1, 1500).to(DEV), [1500], [_params1d(0)], N_EVAL, opt=OPT1D)


# ------------------------------------------------------------------------------------------------ 6. mixed mesh sizes
def test_mixed_size_dataset_goes_through():
    ds = MixedMeshDataset([9, 11], 4, seed=2, target='mmpde5')
    opt = _opt([9, 9], 'mesh_loss', data_type='randg_mix')
    torch.manual_seed(0)
    model = GNN(ds, opt).to(DEV).eval()
    rec = _Recording(model)
    df, dt = evaluate_model_fine(rec, ds, opt)
    assert len(df['L1_grid']) == 4 and [x.shape[0] for x, _ in rec.calls] == [81, 121, 81, 121]
    assert all(np.isfinite(np.asarray(df[k], dtype=float)).all() and (np.asarray(df[k], dtype=float) > 0).all()
               for k in ev.ERROR_COLUMNS[:6])
    df2, _ = evaluate_model_fine(model, ds, opt, batch_size=2)                    # a batch mixes 9 x 9 and 11 x 11
    for k in ev.ERROR_COLUMNS:
        assert np.array_equal(np.asarray(df2[k], dtype=float), np.asarray(df[k], dtype=float), equal_nan=True), k
    k = 1
    s = ds.samples[k]
    _check("randg_mix sample 1 MLmodel", (float(np.asarray(df['L1_MLmodel'])[k]), float(np.asarray(df['L2_MLmodel'])[k])),
           _yard2d(rec.calls[k][0], square_mesh(11), s.pde_params, torch.float64),
           _yard2d(rec.calls[k][0], square_mesh(11), s.pde_params, torch.float32))
