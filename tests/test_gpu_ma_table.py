"""GPU checks of the Monge-Ampere kernels with a tabulated monitor (`ma_table_batch` over gadapt_ma_table_batch and
gadapt_ma_table_batch_strided) against the fp64 restatement of the iteration (tests/ma_table_restatement.py) on the shared cases
(tests/ma_table_cases.py; tests/test_ma_table_host.py proves what is assumed about them here), and of the path from a dataset's
`uu='fem'` through `monitor_source: 'uu'` to the evaluation.

The bars are not fitted to the kernels.  noise = max(|z - z64|, |z' - z|) of the restatement in the route's own arithmetic (fp32
on 'lane', fp64 phi with fp32 rest on 'strided'): what that arithmetic costs the case, and what a logf or an interpolation that
rounds the monitor the other way at every node and step costs it.  4 x noise is the factor of tests/test_gpu_ma.py.
docs/measurements.md has the measured table.

Measured on an MI355X: the kernels are 3.0e-8 to 7.7e-8 from the fp64 restatement after 200 to 300 updates against bars of 1.3e-7
to 2.9e-7, and stop at 440 / 440 (lane / strided; fp64 440) at 11 x 11 and at 1 058 / 1 059 (fp64 1 059) at 15 x 15 with T = 33 tables.
The dataset test uses the reference's mon_reg = 0.01 with cfl = 0.2: all four samples converge (437, 532, 563, 426 updates)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ma_cases as K  # noqa: E402
import ma_restatement as R  # noqa: E402
import ma_table_cases as TC  # noqa: E402
import ma_table_restatement as TR  # noqa: E402

from g_adaptivity_amd import (GNN, MeshDataset, MixedMeshDataset, _native_mesh, eval_grid_MMPDE_MA, evaluate_model_fine, hot_path_opt,  # noqa: E402
                              ma_batch, ma_table_batch, monitor_from_nodal, monitor_table, square_mesh)
from g_adaptivity_amd import evaluation as ev  # noqa: E402
from g_adaptivity_amd.fem import fem_poisson  # noqa: E402
from g_adaptivity_amd.monge_ampere import CAP, CONVERGED, NONCONVEX  # noqa: E402

pytestmark = [pytest.mark.gpu]

ROUTES = TC.ROUTES
# the monitor of the dataset tests: the reference's mon_power, and the reference's mon_reg = 0.01 (it converges with cfl = 0.2 on all four
# samples, so no smaller contrast was needed)
DATASET_MONITOR = {'mon_reg': 0.01, 'mon_power': 0.2}


def _same(a, b, i=0, j=0):
    return (torch.equal(a.coords[i], b.coords[j]) and torch.equal(a.steps[i], b.steps[j]) and torch.equal(a.residual[i], b.residual[j])
            and torch.equal(a.status[i], b.status[j]))


def test_the_library_has_the_table_entry_points(gpu_device):
    lib = _native_mesh.lib()
    for name in ('gadapt_ma_table_max_side', 'gadapt_ma_table_batch', 'gadapt_ma_table_batch_strided'):
        assert getattr(lib, name) is not None
    assert lib.gadapt_mesh_abi_version() == 2 and lib.gadapt_ma_table_max_side() == 1024


@pytest.mark.parametrize('name, route', TC.FIXED)
def test_fixed_step_count_against_fp64(gpu_device, name, route):
    """tol = 0: no stopping decision, exactly `updates` updates.  Every wave edge of the lane route, K = 1, 2 and 7 of the strided
    one, T = 2, N, 17 on 11 and 101, every kind of monitor."""
    c = TC.CASES[name]
    res = ma_table_batch([c.N], [c.table], tol=0.0, max_steps=c.updates, route=route)
    z64, noise = TC.noise(name, route)
    err = (res.coords[0].cpu().double() - z64).abs().max().item()
    print(f"table {route} {name} N={c.N} T={c.T} K={TC.slots(c.N) if route == 'strided' else 1} updates={c.updates}: kernel error {err:.3e}, "
          f"noise {noise:.3e}, bar {4 * noise:.3e}")
    assert res.steps.tolist() == [c.updates] and res.status.tolist() == [CAP]
    assert res.coords[0].shape == (2, c.N, c.N) and res.coords[0].dtype == torch.float32 and res.coords[0].device.type == 'cuda'
    assert err <= 4 * noise


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('name', TC.CONVERGING)
def test_converged_runs_against_fp64(gpu_device, name, route):
    """T = 33.  Stopping step within the restatement's own sensitivity to rounding plus 2; coordinates within 4 x noise plus what
    the updates between the two stopping steps can move a node, at most cfl h tol each: the bar of tests/test_gpu_ma_m2n.py."""
    c, arith = TC.case(name), TC.ARITH_OF_ROUTE[route]
    res = ma_table_batch([c.N], [c.table], route=route)
    (z64, j64, *_), (_, j, *_), (_, jp, *_) = TC.converged(name, 'fp64'), TC.converged(name, arith), TC.converged(name, arith, True)
    _, noise = TC.noise(name, route, j64)                                            # at the fp64 stopping step, tol = 0
    xy, j_gpu = res.coords[0].cpu(), int(res.steps[0])
    err = (xy.double() - z64).abs().max().item()
    bar = 4 * noise + abs(j_gpu - j64) * TC.CFL / (c.N - 1) * TC.TOL
    before, after = R.uniform_spread(c.N, c.params), R.cell_spread(xy, c.params)
    print(f"table {route} {name} N={c.N} T={c.T}: stopping steps gpu / {arith} / {arith}' / fp64 {j_gpu} / {j} / {jp} / {j64}; kernel "
          f"error {err:.3e}, noise {noise:.3e}, bar {bar:.3e}; cell spread {before:.4f} -> {after:.4f}")
    assert res.status.tolist() == [CONVERGED] and res.residual.item() <= TC.TOL
    assert abs(j_gpu - j64) <= max(abs(j - j64), abs(jp - j64)) + 2
    assert err <= bar
    gx, gy = R.grid(c.N, torch.float32)
    assert torch.equal(xy[0][0], gx[0]) and torch.equal(xy[0][-1], gx[-1])           # 0 and 1 bit for bit
    assert torch.equal(xy[1][:, 0], gy[:, 0]) and torch.equal(xy[1][:, -1], gy[:, -1])
    assert R.triangles_keep_orientation(xy, square_mesh(c.N).cells)
    assert after < before


@pytest.mark.parametrize('route', ROUTES)
def test_alone_in_a_mixed_batch_and_again_bit_identical(gpu_device, route):
    """Mixed N and mixed T in one launch.  (A mesh of N <= 32 need not give the same bits on both routes.)"""
    names = [n for n, r in TC.FIXED if r == route]
    sizes, tables = [TC.CASES[n].N for n in names], [TC.CASES[n].table for n in names]
    assert len({(n, t.shape[0]) for n, t in zip(sizes, tables)}) > 4
    for kw in (dict(tol=0.0, max_steps=60), dict(max_steps=150)):                    # a fixed count; each to its own stopping step
        mixed, again = ma_table_batch(sizes, tables, route=route, **kw), ma_table_batch(sizes, tables, route=route, **kw)
        for b, name in enumerate(names):
            alone = ma_table_batch([sizes[b]], [tables[b]], route=route, **kw)
            assert _same(alone, mixed, 0, b) and _same(mixed, again, b, b), name
            assert (alone.coords[0].cpu() - torch.stack(R.grid(sizes[b], torch.float32))).abs().max().item() > 1e-4, name
        if 'tol' in kw:
            assert mixed.status.tolist() == [CAP] * len(names) and mixed.steps.tolist() == [60] * len(names)
    assert set(mixed.status.tolist()) <= {CONVERGED, CAP} and max(mixed.steps.tolist()) == 150


@pytest.mark.parametrize('route', ROUTES)
def test_symmetric_table_gives_a_symmetric_mesh(gpu_device, route):
    """One centred Gaussian with equal scales on a symmetric lattice: the table is symmetric under (x, y) -> (y, x) and x -> 1 - x,
    the kernels' operation order is not, so both hold within the noise bar of this case's own restatement at its fp64 stopping step."""
    c = TC.case('sym11')
    assert torch.equal(c.table.float(), c.table.float().t())
    res = ma_table_batch([c.N], [c.table], route=route)
    x, y = res.coords[0].cpu().double()
    _, noise = TC.noise('sym11', route, TC.converged('sym11', 'fp64')[1])
    print(f"table {route} sym11: |x - y^T| {(x - y.t()).abs().max().item():.3e}, |x - mirror| {(x - (1 - x.flip(0))).abs().max().item():.3e}, "
          f"bar {4 * noise:.3e}")
    assert res.status.tolist() == [CONVERGED]
    assert (x - y.t()).abs().max().item() <= 4 * noise
    assert (x - (1 - x.flip(0))).abs().max().item() <= 4 * noise


@pytest.mark.parametrize('route', ROUTES)
def test_status_paths(gpu_device, route):
    c = TC.case('ds11')
    grid = torch.stack(R.grid(c.N, torch.float32))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        res = ma_table_batch([c.N], [c.table], route=route)
        assert res.status.tolist() == [CONVERGED] and 0 < res.steps.item() < 20000 and res.residual.item() <= TC.TOL
        res = ma_table_batch([c.N], [c.table], max_steps=5, route=route)
        assert res.status.tolist() == [CAP] and res.steps.tolist() == [5] and res.residual.item() > TC.TOL
        res = ma_table_batch([c.N], [c.table], tol=0.0, max_steps=37, route=route)    # tol = 0 runs exactly max_steps
        assert res.status.tolist() == [CAP] and res.steps.tolist() == [37]
        res = ma_table_batch([11, 8, 32], [TC.constant(5), TC.constant(2, 0.3), TC.constant(101, 7.0)], route=route)
        assert res.steps.tolist() == [0, 0, 0] and res.status.tolist() == [CONVERGED] * 3
        for xy, n in zip(res.coords, (11, 8, 32)):
            assert torch.equal(xy.cpu(), torch.stack(R.grid(n, torch.float32)))
        # an ordinary bad input: one entry of the table is not a positive number.  r is not finite there: a status word
        for bad in (0.0, -1.0, float('nan')):
            t = c.table.clone()
            t[16, 16] = bad
            res = ma_table_batch([c.N, c.N], [t, c.table], route=route)
            want = TR.ma(c.N, t, arith=TC.ARITH_OF_ROUTE[route], cfl=TC.CFL, tol=TC.TOL)
            assert want[3] == TR.NONCONVEX and want[1] == 0                           # node (5, 5) sits on table point (16, 16)
            assert res.status.tolist() == [NONCONVEX, CONVERGED] and res.steps.tolist()[0] == 0
            xy = res.coords[0].cpu()
            assert bool(torch.isfinite(xy).all()) and torch.equal(xy, grid)           # flagged, and the last evaluated phi is 0
            assert not bool(torch.isfinite(res.residual[0]))
        assert not w                                                                  # the batch call itself is silent


def test_the_table_of_the_analytic_monitor_follows_the_analytic_kernel(gpu_device):
    """ds11, 200 updates, T = 129: the two kernels differ by no more than the fp64 restatements of the two differ, plus both
    noise bars."""
    c = K.CASES['ds11']
    table = monitor_table(c.params, 129)
    got_t = ma_table_batch([c.N], [table], tol=0.0, max_steps=200).coords[0].cpu().double()
    got_a = ma_batch([c.N], [c.params], tol=0.0, max_steps=200).coords[0].cpu().double()
    runs = {a: TR.ma(c.N, table, arith=a, cfl=TC.CFL, tol=0.0, max_steps=200, perturb=p)[0].double()
            for a, p in (('fp64', None), ('fp32', None))}
    z32p = TR.ma(c.N, table, arith='fp32', cfl=TC.CFL, tol=0.0, max_steps=200, perturb=TC.PERTURB_SEED)[0].double()
    noise_t = max((runs['fp32'] - runs['fp64']).abs().max().item(), (z32p - runs['fp32']).abs().max().item())
    z64a, noise_a = K.noise('ds11', 200)
    gap = (runs['fp64'] - z64a).abs().max().item()
    d = (got_t - got_a).abs().max().item()
    print(f"table T=129 against the analytic kernel, ds11, 200 updates: {d:.3e}; fp64 restatements differ by {gap:.3e}, noise bars "
          f"{4 * noise_t:.3e} + {4 * noise_a:.3e}")
    assert d <= gap + 4 * noise_t + 4 * noise_a
    assert d > 0                                                                      # and they are two monitors


# ---------------------------------------------------------------------------------------------- uu='fem', monitor_source='uu'

def _dataset(**kw):
    return MeshDataset([11, 11], 4, seed=0, target='monge_ampere', uu='fem',
                       target_params=dict(DATASET_MONITOR, monitor_source='uu', solver={'cfl': 0.2, 'tol': 1e-4, 'max_steps': 20000}), **kw)


def test_dataset_with_fem_uu_and_a_solution_driven_monitor(gpu_device):
    """mon_reg = 0.01, the reference's value, with cfl = 0.2: nothing was lowered."""
    ds = _dataset()
    exact = MeshDataset([11, 11], 4, seed=0)
    analytic = MeshDataset([11, 11], 4, seed=0, target='monge_ampere', target_params=dict(DATASET_MONITOR))
    res = ds.target_result
    print(f"uu-driven dataset: steps {res.steps.tolist()}, status {res.status.tolist()}")
    assert res.status.tolist() == [CONVERGED] * 4
    cells = ds.base.cells
    x = torch.cat([s.x_comp for s in ds.samples]).to(gpu_device)
    coeffs, _ = fem_poisson(x, torch.cat([cells + 121 * k for k in range(4)]), torch.cat([s.boundary_nodes for s in ds.samples]),
                            [121] * 4, [s.pde_params for s in ds.samples], (torch.linspace(0, 1, 17), torch.linspace(0, 1, 17)))
    coeffs = coeffs.reshape(4, 121).cpu()
    for k, (s, e, a) in enumerate(zip(ds.samples, exact.samples, analytic.samples)):
        assert s.x_phys.shape == (121, 2) and s.x_phys.dtype == torch.float32 and s.ma_its == res.steps[k].item() + 1 > 1
        assert R.triangles_keep_orientation(s.x_phys.t().reshape(2, 11, 11), cells)
        assert torch.equal(s.uu_tensor, coeffs[k])                                    # the direct solve, bit for bit
        assert torch.equal(e.uu_tensor, e.u_true_tensor) and torch.equal(s.u_true_tensor, e.u_true_tensor)
        gap = (s.uu_tensor - e.uu_tensor).abs().max().item()
        assert gap > 1e-5                                                             # a P1 solve on 11 x 11, not the stand-in
        bn = s.boundary_nodes
        assert (s.uu_tensor[bn] - e.uu_tensor[bn]).abs().max().item() <= 1e-5         # Dirichlet values are u's, formed in fp32
        assert torch.equal(s.x_comp, e.x_comp) and torch.equal(s.f_tensor, e.f_tensor)   # the draws are the same
        # the mesh is the table path's, whatever shares the launch
        table = monitor_from_nodal(s.uu_tensor.view(11, 11).double(), **DATASET_MONITOR)
        alone = ma_table_batch([11], [table])
        assert torch.equal(alone.coords[0].cpu().reshape(2, -1).t(), s.x_phys)
        p = dict(s.pde_params, **DATASET_MONITOR)
        before, after, ana = R.uniform_spread(11, p), R.cell_spread(s.x_phys.t().reshape(2, 11, 11), p), \
            R.cell_spread(a.x_phys.t().reshape(2, 11, 11), p)
        print(f"sample {k}: |uu_fem - u| {gap:.3e}; cell spread grid {before:.4f}, uu-driven {after:.4f} (ratio {after / before:.2f}), "
              f"analytic {ana:.4f} (ratio {ana / before:.2f})")
        assert (s.x_phys - a.x_phys).abs().max().item() > 1e-4                        # two monitors, two meshes
    mixed = MixedMeshDataset([9, 11], 4, seed=2, target='monge_ampere', uu='fem',
                             target_params=dict(DATASET_MONITOR, monitor_source='uu', solver={'route': 'strided'}))
    assert [s.x_phys.shape[0] for s in mixed.samples] == [81, 121, 81, 121] and all(s.ma_its > 1 for s in mixed.samples)
    assert mixed.target_result.status.tolist() == [CONVERGED] * 4
    assert all(not torch.equal(s.uu_tensor, s.u_true_tensor) for s in mixed.samples)


def test_the_evaluation_takes_the_solution_driven_dataset(gpu_device):
    ds = _dataset()
    analytic = MeshDataset([11, 11], 4, seed=0, target='monge_ampere', target_params=dict(DATASET_MONITOR))
    opt = hot_path_opt(mesh_dims=[11, 11], hidden_dim=8, num_layers=4, time_step=0.1, loss_type='mesh_loss', device=str(gpu_device),
                       load_quad_points=101, eval_quad_points=101)
    stored, stored_a = eval_grid_MMPDE_MA(ds, opt), eval_grid_MMPDE_MA(analytic, opt)
    for k in ('L1_grid', 'L2_grid', 'L1_MA', 'L2_MA'):
        v = stored[k]
        print(f"uu-driven evaluation: {k} {v.tolist()}; analytic monitor {stored_a[k].tolist()}")
        assert v.shape == (4,) and bool(torch.isfinite(v).all()) and bool((v > 0).all()), k
    assert torch.equal(stored['L2_grid'], stored_a['L2_grid'])
    assert all(isinstance(s.eval_errors, dict) and s.eval_errors['L2_MA'] == stored['L2_MA'][i] for i, s in enumerate(ds.samples))
    torch.manual_seed(0)
    model = GNN(ds, opt).to(gpu_device).eval()
    df, dt = evaluate_model_fine(model, ds, opt)
    assert list(df.keys()) == ev.ERROR_COLUMNS and list(dt.keys()) == ev.TIME_COLUMNS
    for k in ev.ERROR_COLUMNS[:6]:
        v = np.asarray(df[k], dtype=float)
        assert v.shape == (4,) and np.isfinite(v).all() and (v > 0).all(), k
    assert np.isfinite(np.asarray(dt['MA_time'], dtype=float)).all()


def test_fem_uu_in_one_dimension_and_beyond_26_a_side(gpu_device):
    """`uu='fem'` on the other two forwards: `fem_poisson_1d`, and the windowed band solve that sides above 26 need."""
    from g_adaptivity_amd.fem1d import fem_poisson_1d
    ds, exact = MeshDataset([21], 3, seed=1, uu='fem'), MeshDataset([21], 3, seed=1)
    x = torch.cat([s.x_comp for s in ds.samples]).to(gpu_device)
    coeffs, _ = fem_poisson_1d(x, [21] * 3, [s.pde_params for s in ds.samples], {})
    coeffs = coeffs.reshape(3, 21).cpu()
    for k, (s, e) in enumerate(zip(ds.samples, exact.samples)):
        assert s.uu_tensor.shape == e.uu_tensor.shape and s.uu_tensor.dtype == e.uu_tensor.dtype
        assert torch.equal(s.uu_tensor, coeffs[k]) and torch.equal(s.x_phys, e.x_phys) and torch.equal(s.u_true_tensor, e.u_true_tensor)
        assert 1e-6 < (s.uu_tensor - e.uu_tensor).abs().max().item() < 0.5
    with pytest.raises((NotImplementedError, ValueError)):
        MeshDataset([33, 33], 2, seed=1, uu='fem')                                   # the LDS band stops at 26 a side
    big, plain = MeshDataset([33, 33], 2, seed=1, uu='fem', uu_params={'fem_band': 'window'}), MeshDataset([33, 33], 2, seed=1)
    for s, e in zip(big.samples, plain.samples):
        gap = (s.uu_tensor - e.uu_tensor).abs().max().item()
        print(f"33 x 33, windowed P1 solve: |uu_fem - u| {gap:.3e}")
        assert s.uu_tensor.shape == (33 * 33,) and 1e-6 < gap < 0.1
