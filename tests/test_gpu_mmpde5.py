"""GPU checks of the batched MMPDE5 kernel (g_adaptivity_amd.mmpde5 over libgadapt_mesh.so) against the CPU restatement
(tests/mmpde5_restatement.py) and the golden data recorded from the reference (tools/make_mmpde5_golden.py).

Measured on an MI355X (docs/measurements.md has the table): in 1-D the kernel equals the fp32 restatement bit for bit at
K = 200 and 1 000 steps and stops at the golden step; in 2-D it is within 1.0x of the fp32 restatement's own error and stops
18 steps from the golden count at 11 x 11 and 15 x 15 (bars 137 and 336)."""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mmpde5_restatement as R  # noqa: E402
from test_mmpde5_host import CASES, EDGE_1D, EDGE_2D, EDGE_STEPS, edge_case, edge_restated, load  # noqa: E402

from g_adaptivity_amd import (MMPDE5_1d, MMPDE5_1d_burgers, MMPDE5_2d, DeviceMeshLoader, MeshDataset, MixedMeshDataset,  # noqa: E402
                              deform_mesh_mmpde1d, deform_mesh_mmpde2d, mmpde5_batch, square_mesh)
from g_adaptivity_amd.mmpde5 import CAP, CONVERGED  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]


@pytest.mark.parametrize('steps', [200, 1000])
@pytest.mark.parametrize('name', CASES)
def test_fixed_step_count_against_fp64(gpu_device, name, steps):
    """tol = 0: no stopping decision.  The bar is 4x the error of the fp32 restatement against the fp64 one at the same step
    count (another operation order at the same precision is another draw of the same rounding noise)."""
    _, z0, _, ms, m2, _ = load(name)
    res = mmpde5_batch([z0], [(ms, m2)], tol=0.0, max_steps=steps)
    z64, _, _ = R.mmpde5(z0, ms, m2, dtype=torch.float64, tol=0, max_steps=steps)
    z32, _, _ = R.mmpde5(z0, ms, m2, tol=0, max_steps=steps)
    err = (res.coords[0].double() - z64).abs().max().item()
    bar = 4 * (z32.double() - z64).abs().max().item()
    print(f"{name} K={steps}: kernel error {err:.3e}, bar {bar:.3e}")
    assert res.steps.tolist() == [steps] and res.status.tolist() == [CAP]
    assert res.coords[0].device == z0.device and res.coords[0].shape == z0.shape
    assert err <= bar


@pytest.mark.parametrize('name', CASES)
def test_converged_runs_against_the_reference(gpu_device, name):
    """Steps within the measured sensitivity of the stopping step to rounding (|j_fp32 - j_fp64| of the restatement),
    coordinates within 4x of max |golden - fp64 restatement|."""
    g, z0, z, ms, m2, _ = load(name)
    res = mmpde5_batch([z0.to(gpu_device)], [(ms, m2)])
    _, j32, _ = R.mmpde5(z0, ms, m2)
    z64, j64, _ = R.mmpde5(z0, ms, m2, dtype=torch.float64)
    j_gpu, err = int(res.steps[0]), (res.coords[0].cpu() - z).abs().max().item()
    bar = 4 * (z.double() - z64).abs().max().item()
    print(f"{name}: j gpu {j_gpu}, golden {int(g['j'])}, fp32 / fp64 restatement {j32} / {j64}; |gpu - golden| {err:.3e}, bar {bar:.3e}")
    assert res.coords[0].device.type == 'cuda' and res.steps.device.type == 'cuda'       # same device out
    assert res.status.tolist() == [CONVERGED] and res.measure.item() <= 1e-6
    assert abs(j_gpu - int(g['j'])) <= abs(j32 - j64)
    assert err <= bar


def test_alone_and_in_a_mixed_batch_bit_identical(gpu_device):
    loaded = {n: load(n) for n in ('1d_n21_reg0p1', '2d_n11', '2d_n15', 'burgers_n17')}
    lin = torch.linspace(0, 1, 32)
    big = torch.stack(torch.meshgrid(lin, lin, indexing='ij'))                             # 32 x 32: 16 waves, and the largest block
    big_mon = (1 + torch.rand(31, 31, generator=torch.Generator().manual_seed(0)), torch.ones(32, 32) * 1.5)
    long1d = torch.linspace(0, 1, 1024)
    long_mon = (1 + torch.rand(1023, generator=torch.Generator().manual_seed(1)), torch.ones(1024))
    coords = [v[1] for v in loaded.values()] + [big, long1d]
    mons = [(v[3], v[4]) for v in loaded.values()] + [big_mon, long_mon]
    kw = dict(max_steps=50)                                                               # every mesh reaches this cap
    mixed = mmpde5_batch(coords, mons, **kw)
    again = mmpde5_batch(coords, mons, **kw)
    assert mixed.steps.tolist() == [50] * 6 and mixed.status.tolist() == [CAP] * 6
    for b, (xy, mon) in enumerate(zip(coords, mons)):
        alone = mmpde5_batch([xy], [mon], **kw)
        assert torch.equal(alone.coords[0], mixed.coords[b]) and torch.equal(mixed.coords[b], again.coords[b])
        assert alone.steps.item() == 50 and alone.measure.item() == mixed.measure[b].item()
        assert not torch.equal(alone.coords[0], xy)
    # converged meshes and one that reaches the cap in one launch: each stops at its own step
    g, z0, z, ms, m2, _ = loaded['2d_n11']
    g1, x0, _, ms1, m21, _ = loaded['1d_n21_reg0p1']
    solo = mmpde5_batch([z0], [(ms, m2)])
    both = mmpde5_batch([x0, z0, z0], [(ms1, m21), (ms, m2), (ms, m2)], max_steps=2000)   # the 1-D mesh needs 2 719
    assert both.status.tolist() == [CAP, CONVERGED, CONVERGED] and both.steps[0].item() == 2000
    assert both.steps[1].item() == solo.steps.item() and torch.equal(both.coords[1], solo.coords[0])
    assert torch.equal(both.coords[1], both.coords[2])


EDGES = [(1, n) for n in EDGE_1D] + [(2, n) for n in EDGE_2D]


def _measure_bar(m32, m64):
    """4x the fp32 restatement's own measure error; 4 ulp of the measure should that error be exactly zero (it is not at any
    size of EDGES: the smallest, 8e-7 of the measure, is at 9 x 9)."""
    own = abs(m32 - m64)
    return 4 * own if own > 0 else 4 * float(torch.nextafter(torch.tensor(m64, dtype=torch.float32), torch.tensor(float('inf'))) - m64)


@pytest.mark.parametrize('dim,N', EDGES)
def test_wave_and_workgroup_edges_against_fp64(gpu_device, dim, N):
    """50 steps with tol = 0 at the sizes where the wave count changes and where the last wave is nearly empty: coordinates
    under the bar of test_fixed_step_count_against_fp64, and the last step's measure (the only value that goes through the
    cross-wave sum) under the same 4x bar against the fp64 restatement's measure."""
    z0, mon = edge_case(dim, N)
    res = mmpde5_batch([z0.to(gpu_device)], [mon], tol=0.0, max_steps=EDGE_STEPS)
    (z64, m64), (z32, m32) = edge_restated(dim, N, torch.float64), edge_restated(dim, N, torch.float32)
    err = (res.coords[0].cpu().double() - z64).abs().max().item()
    bar = 4 * (z32.double() - z64).abs().max().item()
    merr, mbar = abs(res.measure.item() - m64), _measure_bar(m32, m64)
    print(f"mmpde5 {dim}d N={N}: coords err {err:.3e} bar {bar:.3e}; measure {res.measure.item():.9e} fp64 {m64:.9e} "
          f"err {merr:.3e} bar {mbar:.3e}")
    assert res.steps.tolist() == [EDGE_STEPS] and res.status.tolist() == [CAP]
    assert res.coords[0].shape == z0.shape
    assert err <= bar
    assert merr <= mbar


def test_wave_and_workgroup_edges_in_one_launch_equal_solo_runs(gpu_device):
    cases = [edge_case(dim, N) for dim, N in EDGES]
    coords, mons = [c[0].to(gpu_device) for c in cases], [c[1] for c in cases]
    mixed = mmpde5_batch(coords, mons, tol=0.0, max_steps=EDGE_STEPS)
    assert mixed.steps.tolist() == [EDGE_STEPS] * len(EDGES) and mixed.status.tolist() == [CAP] * len(EDGES)
    for b, (xy, mon) in enumerate(zip(coords, mons)):
        alone = mmpde5_batch([xy], [mon], tol=0.0, max_steps=EDGE_STEPS)
        assert torch.equal(alone.coords[0], mixed.coords[b]), EDGES[b]
        assert alone.measure.item() == mixed.measure[b].item() and alone.steps.item() == EDGE_STEPS, EDGES[b]


def test_reference_signatures(gpu_device):
    g, x0, x, _, _, params = load('1d_n21_reg0p1')
    X, j, build_time = MMPDE5_1d(x0, 21, params)
    assert X.shape == (21,) and X.device.type == 'cpu' and isinstance(j, int) and build_time > 0
    assert abs(j - int(g['j'])) <= 58 and (X - x).abs().max().item() <= 4e-5
    Xg, jg, _ = MMPDE5_1d(x0.to(gpu_device), 21, params)
    assert Xg.device.type == 'cuda' and jg == j and torch.equal(Xg.cpu(), X)
    xd, jd, _ = deform_mesh_mmpde1d(torch.rand(21), 21, params)
    assert jd == j and torch.equal(xd, X)

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tools'))
    from make_mmpde5_golden import burgers_monitor, burgers_start          # the callable and start mesh of that fixture
    gb, _, xb, _, _, _ = load('burgers_n17')
    Xb, jb, _ = MMPDE5_1d_burgers(burgers_monitor, burgers_start(17), 17)
    assert jb == int(gb['j']) and (Xb - xb).abs().max().item() <= 1e-6

    g2, z0, z, _, _, p2 = load('2d_n11')
    X2, Y2, j2, bt = MMPDE5_2d(z0[0], z0[1], 11, p2)
    assert X2.shape == (11, 11) and Y2.shape == (11, 11) and abs(j2 - int(g2['j'])) <= 137 and bt > 0
    assert max((X2 - z[0]).abs().max().item(), (Y2 - z[1]).abs().max().item()) <= 2e-5
    mesh = square_mesh(11)
    perm = torch.randperm(121, generator=torch.Generator().manual_seed(3))
    x_phys, its, _ = deform_mesh_mmpde2d(mesh.x_comp[perm], 11, 11, p2)                   # any node order
    assert its == j2 + 1 and x_phys.shape == (121, 2)
    back = torch.empty_like(x_phys)
    back[perm] = x_phys
    assert torch.equal(back, torch.stack([X2.reshape(-1), Y2.reshape(-1)], 1))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        mmpde5_batch([z0], [(torch.tensor(g2['ms']), torch.tensor(g2['m2']))], max_steps=5)
        assert not w                                                                      # the batch call itself is silent
        MeshDataset([11, 11], 2, seed=0, target='mmpde5', target_params={'solver': {'max_steps': 5}})
        assert any('not yet converged' in str(i.message) for i in w)


@pytest.mark.parametrize('dims', [[11, 11], [21]])
def test_dataset_targets_feed_the_loader(gpu_device, dims):
    noise = MeshDataset(dims, 6, seed=4)
    ds = MeshDataset(dims, 6, seed=4, target='mmpde5', target_params={'mon_power': 0.2, 'mon_reg': 0.1})
    for a, b in zip(noise.samples, ds.samples):
        assert torch.equal(a.x_comp, b.x_comp) and torch.equal(a.f_tensor, b.f_tensor)    # the draws are the same
        assert b.x_phys.shape == a.x_phys.shape and b.x_phys.dtype == torch.float32 and b.ma_its > 1
        bn = b.boundary_nodes
        assert torch.equal(b.x_phys[bn], b.x_comp[bn])                                    # boundary nodes stay
        assert (b.x_phys - b.x_comp).abs().max().item() > 1e-3                            # the interior is adapted
    one = MeshDataset(dims, 1, seed=4, target='mmpde5', target_params={'mon_power': 0.2, 'mon_reg': 0.1})
    assert torch.equal(one.samples[0].x_phys, ds.samples[0].x_phys)                        # whatever shares the launch
    batch = next(iter(DeviceMeshLoader(ds, batch_size=3, device=gpu_device)))
    assert torch.equal(batch.x_phys.cpu(), torch.cat([s.x_phys for s in ds.samples[:3]]))
    mixed = MixedMeshDataset([9, 11], 4, seed=2, target='mmpde5')
    assert [s.x_phys.shape[0] for s in mixed.samples] == [81, 121, 81, 121] and all(s.ma_its > 1 for s in mixed.samples)


def test_one_training_step_on_mmpde5_targets(gpu_device):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'examples'))
    import train_mesh_loss
    from g_adaptivity_amd import hot_path_opt
    opt = hot_path_opt(mesh_dims=[11, 11], hidden_dim=8, num_layers=2, batch_size=4, epochs=2, device='cuda:0', loss_fn='mse',
                       lr=1e-3, show_mesh_evol_plots='False', device_loader=True, native_loss=True, graphed=True)
    ds = MeshDataset([11, 11], 8, seed=0, target='mmpde5')
    _, losses, _ = train_mesh_loss.main(opt, ds, log=lambda *_: None)
    assert len(losses) == 2 and all(0 < v < float('inf') for v in losses)
