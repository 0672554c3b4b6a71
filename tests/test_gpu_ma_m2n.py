"""GPU checks of the Monge-Ampere kernels with the M2N 'fast' monitor (`ma_batch` with `mesh_type = 'M2N'` over gadapt_ma_m2n_batch
and gadapt_ma_m2n_batch_strided) against the fp64 restatement of the iteration (tests/ma_m2n_restatement.py) on the shared cases
(tests/ma_m2n_cases.py; tests/test_ma_m2n_host.py proves what is assumed about them here).

The bars are not fitted to the kernels.  noise = max(|z - z64|, |z' - z|) of the restatement in the route's own arithmetic (fp32
on 'lane', fp64 phi with fp32 rest on 'strided'): what that arithmetic costs the case, and what an expf / logf / sqrtf or a
quotient that rounds the monitor the other way at every node and step costs it.  4 x noise is the factor of tests/test_gpu_ma.py.
docs/measurements.md has the measured table.

Measured on an MI355X: the kernels are 3.0e-8 to 1.5e-7 from the fp64 restatement after 100 to 500 updates against bars of 1.2e-7
to 6.0e-7, and stop at 781 / 780 (lane / strided; fp64 780) at 11 x 11 and at 1 986 / 1 972 (fp64 1 972) at 15 x 15, the steps of
the restatement in each route's own arithmetic."""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ma_m2n_cases as K  # noqa: E402
import ma_m2n_restatement as M  # noqa: E402

from g_adaptivity_amd import MA2d, MeshDataset, MixedMeshDataset, _native_mesh, deform_mesh_ma2d, ma_batch, square_mesh  # noqa: E402
from g_adaptivity_amd.monge_ampere import CAP, CONVERGED, NONCONVEX  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]

ROUTES = ('lane', 'strided')
FIXED = [(n, r) for n in K.FIXED for r in ROUTES] + [(n, 'strided') for n in K.FIXED_STRIDED]


def _same(a, b, i=0, j=0):
    return (torch.equal(a.coords[i], b.coords[j]) and torch.equal(a.steps[i], b.steps[j]) and torch.equal(a.residual[i], b.residual[j])
            and torch.equal(a.status[i], b.status[j]))


def test_the_library_has_the_m2n_entry_points(gpu_device):
    lib = _native_mesh.lib()
    for name in ('gadapt_ma_m2n_batch', 'gadapt_ma_m2n_batch_strided', 'gadapt_ma_m2n_lds_bytes', 'gadapt_ma_m2n_strided_lds_bytes'):
        assert getattr(lib, name) is not None
    assert lib.gadapt_mesh_abi_version() == 2


@pytest.mark.parametrize('name, route', FIXED)
def test_fixed_step_count_against_fp64(gpu_device, name, route):
    """tol = 0: no stopping decision, exactly `updates` updates.  Every wave edge of the lane route, K = 1, 2, 4 and 7 of the
    strided one, both parameter pairs."""
    c = K.CASES[name]
    res = ma_batch([c.N], [c.params], tol=0.0, max_steps=c.updates, route=route)
    z64, noise = K.noise(name, route)
    err = (res.coords[0].cpu().double() - z64).abs().max().item()
    print(f"m2n {route} {name} N={c.N} K={K.slots(c.N) if route == 'strided' else 1} updates={c.updates}: kernel error {err:.3e}, "
          f"noise {noise:.3e}, bar {4 * noise:.3e}")
    assert res.steps.tolist() == [c.updates] and res.status.tolist() == [CAP]
    assert res.coords[0].shape == (2, c.N, c.N) and res.coords[0].dtype == torch.float32 and res.coords[0].device.type == 'cuda'
    assert err <= 4 * noise


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('name', K.CONVERGING)
def test_converged_runs_against_fp64(gpu_device, name, route):
    """Stopping step within the restatement's own sensitivity to rounding plus 2; coordinates within 4 x noise plus what the
    updates between the two stopping steps can move a node, at most cfl h tol each: the bar of tests/test_gpu_ma.py."""
    c, arith = K.CASES[name], K.ARITH_OF_ROUTE[route]
    res = ma_batch([c.N], [c.params], route=route)
    (z64, j64, *_), (_, j, *_), (_, jp, *_) = K.converged(name, 'fp64'), K.converged(name, arith), K.converged(name, arith, True)
    _, noise = K.noise(name, route, j64)                                             # at the fp64 stopping step, tol = 0
    xy, j_gpu = res.coords[0].cpu(), int(res.steps[0])
    err = (xy.double() - z64).abs().max().item()
    bar = 4 * noise + abs(j_gpu - j64) * K.CFL / (c.N - 1) * K.TOL
    before, after = M.uniform_spread(c.N, c.params), M.cell_spread(xy, c.params)
    print(f"m2n {route} {name} N={c.N}: stopping steps gpu / {arith} / {arith}' / fp64 {j_gpu} / {j} / {jp} / {j64}; kernel error "
          f"{err:.3e}, noise {noise:.3e}, bar {bar:.3e}; cell spread {before:.4f} -> {after:.4f}")
    assert res.status.tolist() == [CONVERGED] and res.residual.item() <= K.TOL
    assert abs(j_gpu - j64) <= max(abs(j - j64), abs(jp - j64)) + 2
    assert err <= bar
    gx, gy = M.grid(c.N, torch.float32)
    assert torch.equal(xy[0][0], gx[0]) and torch.equal(xy[0][-1], gx[-1])           # 0 and 1 bit for bit
    assert torch.equal(xy[1][:, 0], gy[:, 0]) and torch.equal(xy[1][:, -1], gy[:, -1])
    for i, k in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
        assert xy[0][i, k] == gx[i, k] and xy[1][i, k] == gy[i, k]                   # corners do not move
    assert M.triangles_keep_orientation(xy, square_mesh(c.N).cells)
    assert after <= 0.5 * before


@pytest.mark.parametrize('route', ROUTES)
def test_alone_in_a_mixed_batch_and_again_bit_identical(gpu_device, route):
    names = ['n3_g1', 'n9_g1', 'n11_g2', 'n11_g8', 'n32_g2'] + (['n33_g2', 'n81_g2'] if route == 'strided' else [])
    sizes, params = [K.CASES[n].N for n in names], [K.CASES[n].params for n in names]
    for kw in (dict(tol=0.0, max_steps=60), dict(max_steps=300)):                    # a fixed count; each to its own stopping step
        mixed, again = ma_batch(sizes, params, route=route, **kw), ma_batch(sizes, params, route=route, **kw)
        for b, name in enumerate(names):
            alone = ma_batch([sizes[b]], [params[b]], route=route, **kw)
            assert _same(alone, mixed, 0, b) and _same(mixed, again, b, b), name
            assert (alone.coords[0].cpu() - torch.stack(M.grid(sizes[b], torch.float32))).abs().max().item() > 1e-4, name
        if 'tol' in kw:
            assert mixed.status.tolist() == [CAP] * len(names) and mixed.steps.tolist() == [60] * len(names)
    # the restatement stops at 95 at 3 x 3 and has residuals of 0.13 to 1.2 left after 300 updates at the other sizes
    assert mixed.status.tolist() == [CONVERGED] + [CAP] * (len(names) - 1)
    assert mixed.steps.tolist()[1:] == [300] * (len(names) - 1) and 0 < mixed.steps[0].item() < 300


@pytest.mark.parametrize('route', ROUTES)
def test_symmetric_monitor_gives_a_symmetric_mesh(gpu_device, route):
    """One centred Gaussian with equal scales: u_xy^2 and so F are symmetric under (x, y) -> (y, x) and x -> 1 - x, the kernels'
    operation order is not, so both hold within the noise bar of this case's own restatement at its fp64 stopping step."""
    c = K.CASES['sym11']
    res = ma_batch([c.N], [c.params], route=route)
    x, y = res.coords[0].cpu().double()
    _, noise = K.noise('sym11', route, K.converged('sym11', 'fp64')[1])
    print(f"m2n {route} sym11: |x - y^T| {(x - y.t()).abs().max().item():.3e}, |x - mirror| {(x - (1 - x.flip(0))).abs().max().item():.3e}, "
          f"bar {4 * noise:.3e}")
    assert res.status.tolist() == [CONVERGED]
    assert (x - y.t()).abs().max().item() <= 4 * noise
    assert (x - (1 - x.flip(0))).abs().max().item() <= 4 * noise


@pytest.mark.parametrize('route', ROUTES)
def test_no_gaussians_is_the_grid(gpu_device, route):
    """Fmax = 0: the monitor is mon_reg, a decision every lane takes from the Fmax it read from LDS."""
    flat = dict(K.RUN, centers=[], scales=[])
    res = ma_batch([11, 8, 32], [flat, dict(K.LOW, centers=[], scales=[]), flat], route=route)
    assert res.steps.tolist() == [0, 0, 0] and res.status.tolist() == [CONVERGED] * 3
    for xy, n in zip(res.coords, (11, 8, 32)):
        assert torch.equal(xy.cpu(), torch.stack(M.grid(n, torch.float32)))


@pytest.mark.parametrize('route', ROUTES)
def test_status_paths(gpu_device, route):
    c = K.CASES['ds11']
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        res = ma_batch([c.N], [c.params], max_steps=5, route=route)
        assert not w                                                                  # the batch call itself is silent
        assert res.status.tolist() == [CAP] and res.steps.tolist() == [5] and res.residual.item() > K.TOL
    c = K.CASES['nonconvex15']
    with warnings.catch_warnings(record=True) as w:                                   # a status word of a finite loop, not a fault
        warnings.simplefilter('always')
        res = ma_batch([c.N], [c.params], cfl=K.CFL, route=route)
        assert res.status.tolist() == [NONCONVEX] and res.steps.tolist() == [1] and not w
        lower = ma_batch([c.N], [c.params], cfl=0.05, max_steps=5, route=route)       # NONCONVEX means "lower cfl"
        assert lower.status.tolist() == [CAP] and lower.steps.tolist() == [5]


def test_ma2d_with_the_m2n_monitor_is_ma_batch(gpu_device):
    c = K.CASES['ds11']
    mesh = square_mesh(c.N)
    res = ma_batch([c.N], [c.params])
    x_phys, j, build_time = MA2d(mesh.x_comp, c.N, c.params)
    assert j == res.steps.item() > 0 and build_time > 0 and torch.equal(x_phys, res.coords[0].cpu().reshape(2, -1).t())
    x_phys, its, _ = deform_mesh_ma2d(mesh.x_comp, c.N, c.N, c.params)
    assert its == j + 1 and torch.equal(x_phys, res.coords[0].cpu().reshape(2, -1).t())
    # the monitor is read: the same Gaussians under 'ma' with the same mon_reg give another mesh
    as_ma = ma_batch([c.N], [{k: v for k, v in c.params.items() if k not in K.M2N}])
    assert (as_ma.coords[0] - res.coords[0]).abs().max().item() > 1e-3
    c = K.CASES['nonconvex15']
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        x_phys, j, _ = MA2d(square_mesh(c.N).x_comp, c.N, c.params)
        assert j == 0 and torch.equal(x_phys, torch.zeros(c.N * c.N, 2)) and any('lost convexity' in str(i.message) for i in w)


def test_dataset_targets(gpu_device):
    ma = MeshDataset([11, 11], 4, seed=3, target='monge_ampere', target_params={'mon_reg': 0.1, 'mon_power': 0.2})
    ds = MeshDataset([11, 11], 4, seed=3, target='monge_ampere', target_params=dict(K.RUN, solver={'route': 'lane'}))
    res = ds.target_result
    assert res.status.tolist() == [CONVERGED] * 4
    for a, b, j in zip(ma.samples, ds.samples, res.steps.tolist()):
        assert torch.equal(a.x_comp, b.x_comp) and torch.equal(a.f_tensor, b.f_tensor)   # the draws are the same
        assert b.x_phys.shape == (121, 2) and b.x_phys.dtype == torch.float32 and b.ma_its == j + 1 and j > 0
        assert (a.x_phys - b.x_phys).abs().max().item() > 1e-3                           # the monitors are not
    alone = ma_batch([11], [dict(ds.samples[2].pde_params, **K.RUN)])
    assert torch.equal(alone.coords[0].cpu().reshape(2, -1).t(), ds.samples[2].x_phys)   # whatever shares the launch
    mixed = MixedMeshDataset([9, 11], 4, seed=2, target='monge_ampere', target_params=dict(K.RUN, solver={'route': 'strided'}))
    assert [s.x_phys.shape[0] for s in mixed.samples] == [81, 121, 81, 121] and all(s.ma_its > 1 for s in mixed.samples)
    assert mixed.target_result.status.tolist() == [CONVERGED] * 4
    alone = ma_batch([11], [dict(mixed.samples[1].pde_params, **K.RUN)], route='strided')
    assert torch.equal(alone.coords[0].cpu().reshape(2, -1).t(), mixed.samples[1].x_phys)
