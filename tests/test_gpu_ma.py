"""GPU checks of the batched Monge-Ampere kernel (g_adaptivity_amd.monge_ampere over libgadapt_mesh.so) against the fp64
restatement of its iteration (tests/ma_restatement.py) on the shared cases (tests/ma_cases.py; tests/test_ma_host.py proves what
is assumed about them here).

The bars are not fitted to the kernel.  noise = max(|z32 - z64|, |z32' - z32|) of the restatement: what fp32 costs the case, and
what an expf / logf / powf that rounds the monitor the other way at every node and step costs it.  4 x noise is the factor of
tests/test_gpu_mmpde5.py.

Measured on an MI355X (docs/measurements.md has the tables): the kernel is 2.2e-8 to 6.8e-8 from the fp64 restatement after 200
or 500 updates against bars of 6.3e-8 to 3.6e-7, and stops at the fp64 step at 11 x 11 (442) and 15 x 15 (1 121)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ma_cases as K  # noqa: E402
import ma_restatement as R  # noqa: E402

from g_adaptivity_amd import (GNN, MA2d, MeshDataset, MixedMeshDataset, deform_mesh_ma2d, evaluate_model_fine, hot_path_opt,  # noqa: E402
                              ma_batch, square_mesh)
from g_adaptivity_amd import evaluation as ev  # noqa: E402
from g_adaptivity_amd.monge_ampere import CAP, CONVERGED, NONCONVEX  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]


@pytest.mark.parametrize('name', K.FIXED)
def test_fixed_step_count_against_fp64(gpu_device, name):
    """tol = 0: no stopping decision, exactly `updates` updates."""
    c = K.CASES[name]
    res = ma_batch([c.N], [c.params], tol=0.0, max_steps=c.updates)
    z64, noise = K.noise(name)
    err = (res.coords[0].cpu().double() - z64).abs().max().item()
    print(f"ma {name} N={c.N} K={c.updates}: kernel error {err:.3e}, noise {noise:.3e}, bar {4 * noise:.3e}")
    assert res.steps.tolist() == [c.updates] and res.status.tolist() == [CAP]
    assert res.coords[0].shape == (2, c.N, c.N) and res.coords[0].device.type == 'cuda' and res.steps.device.type == 'cuda'
    assert err <= 4 * noise


@pytest.mark.parametrize('name', K.CONVERGING)
def test_converged_runs_against_fp64(gpu_device, name):
    """Stopping step within the restatement's own sensitivity to rounding plus 2 (the residual falls by about 2 % a step at
    11 x 11 and the fp32 floor there is 3 % of tol); coordinates within 4 x noise plus what the updates between the two stopping
    steps can move a node: at most cfl h tol each."""
    c = K.CASES[name]
    res = ma_batch([c.N], [c.params])
    (z64, j64, *_), (_, j32, *_), (_, j32p, *_) = K.converged(name, 'fp64'), K.converged(name, 'fp32'), K.converged(name, 'fp32', True)
    _, noise = K.noise(name, j64)                                                    # at the fp64 stopping step, tol = 0
    xy, j_gpu = res.coords[0].cpu(), int(res.steps[0])
    err = (xy.double() - z64).abs().max().item()
    bar = 4 * noise + abs(j_gpu - j64) * K.CFL / (c.N - 1) * K.TOL
    before, after = R.uniform_spread(c.N, c.params), R.cell_spread(xy, c.params)
    print(f"ma {name} N={c.N}: stopping steps gpu / fp32 / fp32' / fp64 {j_gpu} / {j32} / {j32p} / {j64}; kernel error {err:.3e}, "
          f"noise {noise:.3e}, bar {bar:.3e}; cell spread {before:.4f} -> {after:.4f}")
    assert res.status.tolist() == [CONVERGED] and res.residual.item() <= K.TOL
    assert abs(j_gpu - j64) <= max(abs(j32 - j64), abs(j32p - j64)) + 2
    assert err <= bar
    gx, gy = R.grid(c.N, torch.float32)
    assert torch.equal(xy[0][0], gx[0]) and torch.equal(xy[0][-1], gx[-1])           # 0 and 1 bit for bit
    assert torch.equal(xy[1][:, 0], gy[:, 0]) and torch.equal(xy[1][:, -1], gy[:, -1])
    for i, j in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
        assert xy[0][i, j] == gx[i, j] and xy[1][i, j] == gy[i, j]                   # corners do not move
    assert R.triangles_keep_orientation(xy, square_mesh(c.N).cells)
    assert after <= 0.5 * before


def test_alone_in_a_mixed_batch_and_again_bit_identical(gpu_device):
    names = ['n3_g1', 'n9_g1', 'n11_g2', 'n11_g8', 'n32_g2']                         # N = 3, 9, 11, 32; 1, 2 and 8 Gaussians
    sizes, params = [K.CASES[n].N for n in names], [K.CASES[n].params for n in names]
    for kw in (dict(tol=0.0, max_steps=60), dict(max_steps=400)):                    # a fixed count; each to its own stopping step
        mixed, again = ma_batch(sizes, params, **kw), ma_batch(sizes, params, **kw)
        for b, name in enumerate(names):
            alone = ma_batch([sizes[b]], [params[b]], **kw)
            assert torch.equal(alone.coords[0], mixed.coords[b]) and torch.equal(mixed.coords[b], again.coords[b]), name
            assert alone.steps.item() == mixed.steps[b].item() == again.steps[b].item(), name
            assert alone.residual.item() == mixed.residual[b].item() == again.residual[b].item(), name
            assert alone.status.item() == mixed.status[b].item(), name
            assert (alone.coords[0].cpu() - torch.stack(R.grid(sizes[b], torch.float32))).abs().max().item() > 1e-4, name
    assert mixed.status.tolist() == [CONVERGED, CONVERGED, CAP, CAP, CAP]             # 24 and 312 updates; 774, 540, 4 178 wanted
    assert mixed.steps.tolist()[2:] == [400, 400, 400] and mixed.steps[0].item() < mixed.steps[1].item() < 400


def test_symmetric_monitor_gives_a_symmetric_mesh(gpu_device):
    """One centred Gaussian with equal scales: the problem is symmetric under (x, y) -> (y, x) and x -> 1 - x, the kernel's
    operation order is not, so both hold within the noise bar of this case's own restatement at its fp64 stopping step."""
    c = K.CASES['sym11']
    res = ma_batch([c.N], [c.params])
    x, y = res.coords[0].cpu().double()
    _, noise = K.noise('sym11', K.converged('sym11', 'fp64')[1])
    print(f"ma sym11: |x - y^T| {(x - y.t()).abs().max().item():.3e}, |x - mirror| {(x - (1 - x.flip(0))).abs().max().item():.3e}, "
          f"bar {4 * noise:.3e}")
    assert res.status.tolist() == [CONVERGED]
    assert (x - y.t()).abs().max().item() <= 4 * noise
    assert (x - (1 - x.flip(0))).abs().max().item() <= 4 * noise


def test_constant_monitor_is_the_grid(gpu_device):
    res = ma_batch([11, 8], [{'centers': [], 'scales': []}, {'centers': [], 'scales': [], 'mon_reg': 0.01, 'mon_power': 0.2}])
    assert res.steps.tolist() == [0, 0] and res.status.tolist() == [CONVERGED, CONVERGED]
    for xy, n in zip(res.coords, (11, 8)):
        assert torch.equal(xy.cpu(), torch.stack(R.grid(n, torch.float32)))


def test_status_paths(gpu_device):
    c = K.CASES['narrow11']
    mesh = square_mesh(c.N)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        res = ma_batch([c.N], [c.params], max_steps=5)
        assert not w                                                                  # the batch call itself is silent
        assert res.status.tolist() == [CAP] and res.steps.tolist() == [5] and res.residual.item() > K.TOL
        x_phys, j, _ = MA2d(mesh.x_comp, c.N, c.params, max_steps=5)
        assert j == 5 and any('not yet converged' in str(i.message) for i in w)
        assert torch.equal(x_phys, res.coords[0].cpu().reshape(2, -1).t())
    with warnings.catch_warnings(record=True) as w:                                   # a status word of a finite loop, not a fault
        warnings.simplefilter('always')
        res = ma_batch([c.N], [c.params], cfl=1.0)
        assert res.status.tolist() == [NONCONVEX] and res.steps.tolist() == [1] and not w
        x_phys, j, build_time = MA2d(mesh.x_comp, c.N, c.params, cfl=1.0)
        assert j == 0 and build_time > 0 and torch.equal(x_phys, torch.zeros(c.N * c.N, 2))
        assert any('lost convexity' in str(i.message) for i in w)
        x_phys, its, _ = deform_mesh_ma2d(mesh.x_comp, c.N, c.N, c.params, cfl=1.0)
        assert its == 1 and not x_phys.any()


def test_dataset_targets(gpu_device):
    noise = MeshDataset([11, 11], 4, seed=3)
    ds = MeshDataset([11, 11], 4, seed=3, target='monge_ampere', target_params=K.REG)
    res = ds.target_result
    assert res.status.tolist() == [CONVERGED] * 4
    for a, b, j in zip(noise.samples, ds.samples, res.steps.tolist()):
        assert torch.equal(a.x_comp, b.x_comp) and torch.equal(a.f_tensor, b.f_tensor)   # the draws are the same
        assert b.x_phys.shape == (121, 2) and b.x_phys.dtype == torch.float32 and b.x_phys.device.type == 'cpu'
        assert b.ma_its == j + 1 and j > 0 and b.build_time > 0
        bn = b.boundary_nodes
        assert (b.x_phys[bn] == b.x_comp[bn]).any(1).all()                               # the normal coordinate stays
        assert (b.x_phys - b.x_comp).abs().max().item() > 1e-3                           # the mesh is adapted
    alone = ma_batch([11], [dict(ds.samples[2].pde_params, **K.REG)])
    assert torch.equal(alone.coords[0].cpu().reshape(2, -1).t(), ds.samples[2].x_phys)   # whatever shares the launch
    mixed = MixedMeshDataset([9, 11], 4, seed=2, target='monge_ampere')                  # one launch, the default monitor
    assert [s.x_phys.shape[0] for s in mixed.samples] == [81, 121, 81, 121] and all(s.ma_its > 1 for s in mixed.samples)
    assert mixed.target_result.steps.shape == (4,) and mixed.target_result.status.tolist() == [CONVERGED] * 4


def test_deform_mesh_ma2d_writes_back_in_the_order_given(gpu_device):
    c = K.CASES['ds11']
    mesh = square_mesh(c.N)
    straight, j, build_time = MA2d(mesh.x_comp, c.N, c.params)
    res = ma_batch([c.N], [c.params])
    assert j == res.steps.item() and build_time > 0 and torch.equal(straight, res.coords[0].cpu().reshape(2, -1).t())
    perm = torch.randperm(c.N * c.N, generator=torch.Generator().manual_seed(3))
    x_phys, its, _ = deform_mesh_ma2d(mesh.x_comp[perm], c.N, c.N, c.params)
    assert its == j + 1 and x_phys.shape == (c.N * c.N, 2)
    back = torch.empty_like(x_phys)
    back[perm] = x_phys
    assert torch.equal(back, straight)
    on_gpu, _, _ = MA2d(mesh.x_comp.to(gpu_device), c.N, c.params)
    assert on_gpu.device.type == 'cuda' and torch.equal(on_gpu.cpu(), straight)


def test_evaluate_model_fine_on_monge_ampere_targets(gpu_device):
    ds = MeshDataset([11, 11], 3, seed=0, target='monge_ampere', target_params=K.REG)
    opt = hot_path_opt(mesh_dims=[11, 11], hidden_dim=8, num_layers=4, time_step=0.1, loss_type='mesh_loss', device=str(gpu_device),
                       load_quad_points=101, eval_quad_points=101)
    torch.manual_seed(0)
    model = GNN(ds, opt).to(gpu_device).eval()
    df, dt = evaluate_model_fine(model, ds, opt)
    for k in ev.ERROR_COLUMNS:
        if 'MA' in k:
            assert np.isfinite(np.asarray(df[k], dtype=float)).all(), k
    ma_time = np.asarray(dt['MA_time'], dtype=float)
    assert np.isfinite(ma_time).all() and (ma_time > 0).all()
    print(f"ma evaluate_model_fine: L2_grid {np.asarray(df['L2_grid'], dtype=float)}, L2_MA {np.asarray(df['L2_MA'], dtype=float)}")


def test_limits(gpu_device):
    p = K.CASES['ds11'].params
    with pytest.raises(ValueError, match='32'):
        ma_batch([33], [p])
    with pytest.raises(ValueError, match='at most 8'):
        ma_batch([11], [K.drawn(1, 9)])
    with pytest.raises(ValueError, match='2-D only'):
        MeshDataset([21], 2, target='monge_ampere')
