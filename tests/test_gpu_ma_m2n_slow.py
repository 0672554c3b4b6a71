"""GPU checks of the Monge-Ampere kernel with the M2N 'slow' monitor (`ma_batch(..., m2n_solve='p1')` over gadapt_ma_m2n_slow_batch:
a P1 Poisson solve on the moving mesh, banded Cholesky in LDS, inside every update) against the fp64 restatement of the iteration
(tests/ma_m2n_slow_restatement.py) on the shared cases (tests/ma_m2n_slow_cases.py; tests/test_ma_m2n_slow_host.py proves what is
assumed about them here, among it that 4 x noise is at most a tenth of the distance to the 'fast' monitor's mesh).

The bars are not fitted to the kernel.  noise = max(|z32 - z64|, |z32' - z32|) of the restatement in fp32, plain and with the
monitor perturbed by an ulp per node and evaluation; 4 x noise is the factor of tests/test_gpu_ma_m2n.py.  The monitor at 0
updates has 4 x |m32 - m64| of the restatement.  docs/measurements.md has the measured table.

Measured on an MI355X: the kernel is 5.7e-8 to 3.6e-5 from the fp64 restatement after 60 to 200 updates, 0.7 to 1.3 x the noise of
each case (bars of 4 x), its monitor at 0 updates 4.1e-8 to 1.9e-4 from fp64 against bars of 4.3e-7 to 7.5e-4, and it stops at 708
(fp64 710) at 11 x 11 and at 1 982 (fp64 1 977) at 15 x 15, inside the spread of the fp32 restatements."""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ma_m2n_slow_cases as K  # noqa: E402
import ma_m2n_slow_restatement as S  # noqa: E402

from g_adaptivity_amd import (MA2d, MASlowResult, MeshDataset, _native_mesh, deform_mesh_ma2d, ma_batch, monitor_m2n_slow,  # noqa: E402
                              square_mesh)
from g_adaptivity_amd.monge_ampere import CAP, CONVERGED, NONCONVEX  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]

P1 = {'m2n_solve': 'p1'}


def _same(a, b, i=0, j=0):
    return (torch.equal(a.coords[i], b.coords[j]) and torch.equal(a.steps[i], b.steps[j]) and torch.equal(a.residual[i], b.residual[j])
            and torch.equal(a.status[i], b.status[j]))


def test_the_library_has_the_slow_entry_point(gpu_device):
    lib = _native_mesh.lib()
    for name in ('gadapt_ma_m2n_slow_batch', 'gadapt_ma_m2n_slow_lds_bytes', 'gadapt_ma_m2n_slow_max_side'):
        assert getattr(lib, name) is not None
    assert lib.gadapt_mesh_abi_version() == 2 and lib.gadapt_ma_m2n_slow_max_side() == K.MAX_SIDE >= 23


@pytest.mark.parametrize('name', K.FIXED)
def test_monitor_at_zero_updates_against_fp64(gpu_device, name):
    """max_steps = 0, tol = 0: `monitor_out` is the monitor of the uniform grid, the solve alone.  Against `monitor_m2n_slow` in
    fp64; the bar is 4 x the distance of the fp32 restatement's monitor from the fp64 restatement's."""
    c = K.CASES[name]
    res = ma_batch([c.N], [c.params], tol=0.0, max_steps=0, **P1)
    gx, gy = S.grid(c.N, torch.float64)
    want = monitor_m2n_slow(gx, gy, c.params)
    m64, mnoise = K.monitor_noise(name)
    err = (res.monitor[0].cpu().double() - want).abs().max().item()
    print(f"slow monitor {name} N={c.N}: kernel error {err:.3e}, fp32 restatement from fp64 {mnoise:.3e}, bar {4 * mnoise:.3e}; "
          f"monitor_m2n_slow from the restatement {(want - m64).abs().max().item():.3e}")
    assert isinstance(res, MASlowResult) and res.steps.tolist() == [0] and res.status.tolist() == [CAP]
    assert res.monitor[0].shape == (c.N, c.N) and res.monitor[0].dtype == torch.float32
    assert torch.equal(res.coords[0].cpu(), torch.stack(S.grid(c.N, torch.float32)))
    assert err <= 4 * mnoise


@pytest.mark.parametrize('name', K.FIXED)
def test_fixed_step_count_against_fp64(gpu_device, name):
    """tol = 0: no stopping decision, exactly `updates` updates, every wave edge from one interior node to the LDS limit."""
    c = K.CASES[name]
    res = ma_batch([c.N], [c.params], tol=0.0, max_steps=c.updates, **P1)
    z64, noise = K.noise(name)
    err = (res.coords[0].cpu().double() - z64).abs().max().item()
    print(f"slow {name} N={c.N} updates={c.updates}: kernel error {err:.3e}, noise {noise:.3e}, bar {4 * noise:.3e}, "
          f"gap to 'fast' {K.gap_to_fast(name):.3e}")
    assert res.steps.tolist() == [c.updates] and res.status.tolist() == [CAP]
    assert res.coords[0].shape == (2, c.N, c.N) and res.coords[0].dtype == torch.float32 and res.coords[0].device.type == 'cuda'
    assert err <= 4 * noise


@pytest.mark.parametrize('name', K.CONVERGING)
def test_converged_runs_against_fp64(gpu_device, name):
    """Stopping step within the restatement's own sensitivity to rounding plus 2; coordinates within 4 x noise plus what the
    updates between the two stopping steps can move a node, at most cfl h tol each: the bar of tests/test_gpu_ma_m2n.py."""
    c = K.CASES[name]
    res = ma_batch([c.N], [c.params], **P1)
    (z64, j64, *_), (_, j, *_), (_, jp, *_) = K.converged(name, 'fp64'), K.converged(name, 'fp32'), K.converged(name, 'fp32', True)
    _, noise = K.noise(name, j64)                                                    # at the fp64 stopping step, tol = 0
    xy, j_gpu = res.coords[0].cpu(), int(res.steps[0])
    err = (xy.double() - z64).abs().max().item()
    bar = 4 * noise + abs(j_gpu - j64) * K.CFL / (c.N - 1) * K.TOL
    print(f"slow {name} N={c.N}: stopping steps gpu / fp32 / fp32' / fp64 {j_gpu} / {j} / {jp} / {j64}; kernel error {err:.3e}, "
          f"noise {noise:.3e}, bar {bar:.3e}")
    assert res.status.tolist() == [CONVERGED] and res.residual.item() <= K.TOL
    assert abs(j_gpu - j64) <= max(abs(j - j64), abs(jp - j64)) + 2
    assert err <= bar
    gx, gy = S.grid(c.N, torch.float32)
    assert torch.equal(xy[0][0], gx[0]) and torch.equal(xy[0][-1], gx[-1])           # 0 and 1 bit for bit
    assert torch.equal(xy[1][:, 0], gy[:, 0]) and torch.equal(xy[1][:, -1], gy[:, -1])
    assert S.triangles_keep_orientation(xy, square_mesh(c.N).cells)


def test_alone_in_a_mixed_batch_and_again_bit_identical(gpu_device):
    """[3, 9, 11, 16, max]: the 3 x 3 mesh shares a launch of 576 lanes with the largest mesh, so eight of its nine waves hold no
    node and still have to reach every barrier of its one-column solve: the barrier-uniformity case."""
    names = ['n3_g1', 'n9_g1', 'n11_g2', 'n16_g2', 'nmax_g2']
    sizes, params = [K.CASES[n].N for n in names], [K.CASES[n].params for n in names]
    for kw in (dict(tol=0.0, max_steps=40), dict(max_steps=120)):                    # a fixed count; each to its own stopping step
        mixed, again = ma_batch(sizes, params, **kw, **P1), ma_batch(sizes, params, **kw, **P1)
        for b, name in enumerate(names):
            alone = ma_batch([sizes[b]], [params[b]], **kw, **P1)
            assert _same(alone, mixed, 0, b) and _same(mixed, again, b, b), name
            assert torch.equal(alone.monitor[0], mixed.monitor[b]) and torch.equal(mixed.monitor[b], again.monitor[b]), name
            assert (alone.coords[0].cpu() - torch.stack(S.grid(sizes[b], torch.float32))).abs().max().item() > 1e-4, name
        if 'tol' in kw:
            assert mixed.status.tolist() == [CAP] * len(names) and mixed.steps.tolist() == [40] * len(names)
    assert set(mixed.status.tolist()) <= {CONVERGED, CAP} and all(0 < s <= 120 for s in mixed.steps.tolist())


@pytest.mark.parametrize('name', ['n3_g1', 'n9_g1', 'n11_g8', 'n23_g2'])
def test_alpha_zero_gives_the_bits_of_the_fast_kernel(gpu_device, name):
    """M2N_alpha = 0: alpha * (E / Emax) is 0 (E / Emax is finite, at most 1), reg + 0 is exact, and everything else is the source
    of ma_m2n_kernel compiled with the same flags: the bits of gadapt_ma_m2n_batch with the same mon_reg and beta."""
    c = K.CASES[name]
    slow = ma_batch([c.N], [dict(c.params, M2N_alpha=0.0)], max_steps=150, **P1)
    fast = ma_batch([c.N], [K.fast_params(c.params)], max_steps=150)
    assert _same(slow, fast) and slow.steps.item() > 0
    with_e = ma_batch([c.N], [c.params], max_steps=150, **P1)
    assert (with_e.coords[0] - fast.coords[0]).abs().max().item() > 1e-3              # and alpha = 1 is read


def test_no_gaussians_is_the_grid(gpu_device):
    """u = f = 0: the solve gives 0, Emax = Fmax = 0, the monitor is mon_reg: decisions every lane takes from LDS values."""
    flat = dict(K.RUN, centers=[], scales=[])
    res = ma_batch([11, 8, K.MAX_SIDE], [flat, dict(K.LOW, centers=[], scales=[]), flat], **P1)
    assert res.steps.tolist() == [0, 0, 0] and res.status.tolist() == [CONVERGED] * 3
    for xy, m, n, reg in zip(res.coords, res.monitor, (11, 8, K.MAX_SIDE), (0.1, 0.01, 0.1)):
        assert torch.equal(xy.cpu(), torch.stack(S.grid(n, torch.float32)))
        assert torch.equal(m.cpu(), torch.full((n, n), reg, dtype=torch.float32))


def test_status_paths(gpu_device):
    c = K.CASES['ds11']
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        res = ma_batch([c.N], [c.params], max_steps=5, **P1)
        assert not w                                                                  # the batch call itself is silent
        assert res.status.tolist() == [CAP] and res.steps.tolist() == [5] and res.residual.item() > K.TOL
    c = K.CASES['nonconvex15']                                                        # found with the fp64 restatement
    with warnings.catch_warnings(record=True) as w:                                   # a status word of a finite loop, not a fault
        warnings.simplefilter('always')
        res = ma_batch([c.N], [c.params], cfl=K.NONCONVEX_CFL, **P1)
        assert res.status.tolist() == [NONCONVEX] and res.steps.tolist() == [1] and not w
        lower = ma_batch([c.N], [c.params], cfl=0.05, max_steps=5, **P1)              # NONCONVEX means "lower cfl"
        assert lower.status.tolist() == [CAP] and lower.steps.tolist() == [5]


def test_symmetric_monitor_gives_a_symmetric_mesh(gpu_device):
    """One centred Gaussian with equal scales.  The triangulation maps to itself under (i, j) -> (j, i) and under the point
    reflection (not under a mirror in one direction), the kernel's operation order under neither: x = y^T within the noise bar
    of this case's own restatement at its fp64 stopping step, the point reflection within that plus what the fp64 restatement
    itself keeps of it (the grid's fp32 coordinates are not exactly symmetric about 1/2)."""
    c = K.CASES['sym11']
    res = ma_batch([c.N], [c.params], **P1)
    x, y = res.coords[0].cpu().double()
    z64, j64 = K.converged('sym11', 'fp64')[:2]
    _, noise = K.noise('sym11', j64)
    own = (z64[0] - (1 - z64[0].flip(0).flip(1))).abs().max().item()
    t, p = (x - y.t()).abs().max().item(), (x - (1 - x.flip(0).flip(1))).abs().max().item()
    print(f"slow sym11: |x - y^T| {t:.3e}, |x - point reflection| {p:.3e} (fp64 restatement {own:.3e}), bar {4 * noise:.3e}")
    assert res.status.tolist() == [CONVERGED]
    assert t <= 4 * noise and p <= 4 * noise + own


def test_ma2d_and_dataset_targets_are_ma_batch(gpu_device):
    c = K.CASES['ds11']
    mesh = square_mesh(c.N)
    res = ma_batch([c.N], [c.params], **P1)
    x_phys, j, build_time = MA2d(mesh.x_comp, c.N, c.params, **P1)
    assert j == res.steps.item() > 0 and build_time > 0 and torch.equal(x_phys, res.coords[0].cpu().reshape(2, -1).t())
    x_phys, its, _ = deform_mesh_ma2d(mesh.x_comp, c.N, c.N, c.params, **P1)
    assert its == j + 1 and torch.equal(x_phys, res.coords[0].cpu().reshape(2, -1).t())
    fast = MeshDataset([11, 11], 3, seed=3, target='monge_ampere', target_params=K.fast_params(K.RUN))
    ds = MeshDataset([11, 11], 3, seed=3, target='monge_ampere', target_params=dict(K.RUN, solver=P1))
    out = ds.target_result
    assert isinstance(out, MASlowResult) and out.status.tolist() == [CONVERGED] * 3
    for a, b, steps in zip(fast.samples, ds.samples, out.steps.tolist()):
        assert torch.equal(a.x_comp, b.x_comp) and b.x_phys.shape == (121, 2) and b.ma_its == steps + 1 and steps > 0
        assert (a.x_phys - b.x_phys).abs().max().item() > 1e-3                           # the monitors are not the same
    alone = ma_batch([11], [dict(ds.samples[2].pde_params, **K.RUN)], **P1)
    assert torch.equal(alone.coords[0].cpu().reshape(2, -1).t(), ds.samples[2].x_phys)   # whatever shares the launch
