"""GPU checks of the strided Monge-Ampere route (`ma_batch(..., route='strided')` over gadapt_ma_batch_strided: fp64 potential,
K = ceil(N^2 / 1024) nodes per lane, up to 81 x 81) against the fp64 restatement of the iteration (tests/ma_restatement.py) on
the shared cases (tests/ma_strided_cases.py; tests/test_ma_strided_host.py proves what is assumed about them here).

The bars are not fitted to the kernel.  noise = max(|z_mixed - z64|, |z_mixed' - z_mixed|) of the restatements: what the route's
mixed arithmetic costs the case, and what an expf / logf / powf that rounds the monitor the other way at every node and step
costs it (5.96e-8 in every case, a bar of 2.38e-7).  4 x noise is the factor of tests/test_gpu_ma.py.  docs/measurements.md has
the measured table."""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ma_cases as K  # noqa: E402
import ma_restatement as R  # noqa: E402
import ma_strided_cases as SK  # noqa: E402

from g_adaptivity_amd import MeshDataset, ma_batch, square_mesh  # noqa: E402
from g_adaptivity_amd.monge_ampere import CAP, CONVERGED, NONCONVEX  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]

STRIDED = dict(route='strided')


@pytest.mark.parametrize('name', SK.FIXED)
def test_fixed_step_count_against_fp64(gpu_device, name):
    """tol = 0: no stopping decision, exactly 300 updates; one case per slot count K and per edge of it."""
    c = SK.CASES[name]
    res = ma_batch([c.N], [c.params], tol=0.0, max_steps=c.updates, **STRIDED)
    z64, noise = SK.noise(name)
    err = (res.coords[0].cpu().double() - z64).abs().max().item()
    print(f"ma strided {name} N={c.N} K={SK.slots(c.N)}: kernel error {err:.3e}, noise {noise:.3e}, bar {4 * noise:.3e}")
    assert res.status.tolist() == [CAP] and res.steps.tolist() == [c.updates]
    assert res.coords[0].shape == (2, c.N, c.N) and res.coords[0].dtype == torch.float32 and res.coords[0].device.type == 'cuda'
    assert err <= 4 * noise


def _check_converged(name, res):
    """The assertions of a converged run against the case's yardstick (computed here for ds33, stored for ds64)."""
    c, y = SK.case(name), SK.yardstick(name)
    xy, j_gpu = res.coords[0].cpu(), int(res.steps[0])
    err = (xy.double() - y.z64).abs().max().item()
    bar = 4 * y.noise + abs(j_gpu - y.j64) * SK.CFL / (c.N - 1) * SK.TOL       # what the updates between the two stops can move a node
    before, after = R.uniform_spread(c.N, c.params), R.cell_spread(xy, c.params)
    print(f"ma strided {name} N={c.N}: stopping steps gpu / mixed / mixed' / fp64 {j_gpu} / {y.jm} / {y.jmp} / {y.j64}; kernel error "
          f"{err:.3e}, noise {y.noise:.3e}, bar {bar:.3e}; residual {res.residual.item():.3e}; cell spread {before:.4f} -> {after:.4f}")
    assert res.status.tolist() == [CONVERGED] and res.residual.item() <= SK.TOL
    assert abs(j_gpu - y.j64) <= max(abs(y.jm - y.j64), abs(y.jmp - y.j64)) + 2
    assert err <= bar
    gx, gy = R.grid(c.N, torch.float32)
    assert torch.equal(xy[0][0], gx[0]) and torch.equal(xy[0][-1], gx[-1])      # the normal coordinate bit for bit
    assert torch.equal(xy[1][:, 0], gy[:, 0]) and torch.equal(xy[1][:, -1], gy[:, -1])
    for i, j in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
        assert xy[0][i, j] == gx[i, j] and xy[1][i, j] == gy[i, j]              # corners do not move
    assert R.triangles_keep_orientation(xy, square_mesh(c.N).cells)
    assert after <= 0.5 * before
    return j_gpu


def test_ds33_converged_against_fp64(gpu_device):
    c = SK.case('ds33')
    j_gpu = _check_converged('ds33', ma_batch([c.N], [c.params], **STRIDED))
    # capped one update before the kernel's own stopping step, the residual is still above tol
    short = ma_batch([c.N], [c.params], max_steps=j_gpu - 1, **STRIDED)
    assert short.status.tolist() == [CAP] and short.steps.tolist() == [j_gpu - 1] and short.residual.item() > SK.TOL


def test_ds64_converged_against_the_stored_fp64_run(gpu_device):
    """The default cap at 64 x 64: this sample stops at 17 512 in fp64, below the default 20 000, so the default call is the same
    run bit for bit; the drawn case n64_g2 wants 25 497 updates in fp64 (25 495 in the mixed restatement, whose residual after
    20 000 is 7.0e-4), so there the default call returns CAP at 20 000."""
    c = SK.case('ds64')
    res = ma_batch([c.N], [c.params], max_steps=40000, **STRIDED)
    _check_converged('ds64', res)
    dflt = ma_batch([c.N], [c.params], **STRIDED)
    assert torch.equal(dflt.coords[0], res.coords[0]) and torch.equal(dflt.steps, res.steps) and dflt.status.tolist() == [CONVERGED]
    c = SK.CASES['n64_g2']
    dflt = ma_batch([c.N], [c.params], **STRIDED)                               # 64 x 64 can want more than the default cap
    assert dflt.status.tolist() == [CAP] and dflt.steps.tolist() == [20000] and dflt.residual.item() > SK.TOL


def test_alone_in_a_mixed_batch_and_again_bit_identical(gpu_device):
    names = ['n8_g2', 'n33_g2', 'n46_g2', 'n64_g2', 'n81_g2']                    # K = 1, 2, 3, 4, 7 in one launch
    sizes, params = [SK.CASES[n].N for n in names], [SK.CASES[n].params for n in names]
    for kw in (dict(tol=0.0, max_steps=60), dict(max_steps=400)):               # a fixed count; each to its own stopping step
        mixed, again = ma_batch(sizes, params, **kw, **STRIDED), ma_batch(sizes, params, **kw, **STRIDED)
        for b, name in enumerate(names):
            alone = ma_batch([sizes[b]], [params[b]], **kw, **STRIDED)
            assert torch.equal(alone.coords[0], mixed.coords[b]) and torch.equal(mixed.coords[b], again.coords[b]), name
            assert torch.equal(alone.steps[0], mixed.steps[b]) and torch.equal(mixed.steps[b], again.steps[b]), name
            assert torch.equal(alone.residual[0], mixed.residual[b]) and torch.equal(mixed.residual[b], again.residual[b]), name
            assert torch.equal(alone.status[0], mixed.status[b]) and torch.equal(mixed.status[b], again.status[b]), name
            assert (alone.coords[0].cpu() - torch.stack(R.grid(sizes[b], torch.float32))).abs().max().item() > 1e-4, name
        if 'tol' in kw:
            assert mixed.status.tolist() == [CAP] * 5 and mixed.steps.tolist() == [60] * 5
    # the mixed restatement stops at 366 at 8 x 8 and has residuals of 0.25 to 0.96 left after 400 updates at the other sizes
    assert mixed.status.tolist() == [CONVERGED, CAP, CAP, CAP, CAP]
    assert mixed.steps.tolist()[1:] == [400] * 4 and 0 < mixed.steps[0].item() < 400


@pytest.mark.parametrize('name', SK.ROUTE)
def test_route_contract_up_to_32(gpu_device, name):
    """Up to 32 a side both routes run: the strided one is within its own bar of fp64 (it does not share bits with the lane route:
    phi is fp64 on one and fp32 on the other), and the default is the lane route, untouched by the keyword."""
    c = SK.CASES[name]
    kw = dict(tol=0.0, max_steps=c.updates)
    strided = ma_batch([c.N], [c.params], **kw, **STRIDED)
    z64, noise = SK.noise(name)
    err = (strided.coords[0].cpu().double() - z64).abs().max().item()
    print(f"ma strided {name} N={c.N} K={c.updates}: kernel error {err:.3e}, noise {noise:.3e}, bar {4 * noise:.3e}")
    assert strided.status.tolist() == [CAP] and strided.steps.tolist() == [c.updates] and err <= 4 * noise
    plain, lane = ma_batch([c.N], [c.params], **kw), ma_batch([c.N], [c.params], route='lane', **kw)
    assert torch.equal(plain.coords[0], lane.coords[0]) and torch.equal(plain.residual, lane.residual)
    assert torch.equal(plain.steps, lane.steps) and torch.equal(plain.status, lane.status)
    _, lane_noise = K.noise({'route11': 'n11_g2', 'route32': 'n32_g2'}[name])
    assert (plain.coords[0].cpu().double() - z64).abs().max().item() <= 4 * lane_noise     # the lane route's own bar, as before


def test_lost_convexity_and_constant_monitor(gpu_device):
    c = K.CASES['narrow11']
    with warnings.catch_warnings(record=True) as w:                             # a status word of a finite loop, not a fault
        warnings.simplefilter('always')
        res = ma_batch([c.N], [c.params], cfl=1.0, **STRIDED)
        assert res.status.tolist() == [NONCONVEX] and res.steps.tolist() == [1] and not w
    flat = {'centers': [], 'scales': [], **SK.REG}
    res = ma_batch([33, 8], [flat, {'centers': [], 'scales': []}], **STRIDED)
    assert res.steps.tolist() == [0, 0] and res.status.tolist() == [CONVERGED, CONVERGED]
    for xy, n in zip(res.coords, (33, 8)):
        assert torch.equal(xy.cpu(), torch.stack(R.grid(n, torch.float32)))


def test_dataset_targets_at_64(gpu_device):
    solver = {'route': 'strided', 'max_steps': 40000}
    ds = MeshDataset([64, 64], 2, seed=0, target='monge_ampere', target_params={**SK.REG, 'solver': solver})
    res = ds.target_result
    assert res.status.tolist() == [CONVERGED, CONVERGED]
    for s, j in zip(ds.samples, res.steps.tolist()):
        assert s.x_phys.shape == (4096, 2) and s.x_phys.dtype == torch.float32 and s.ma_its == j + 1 and j > 10000
        assert (s.x_phys - s.x_comp).abs().max().item() > 1e-3                  # the mesh is adapted
    alone = ma_batch([64], [dict(ds.samples[0].pde_params, **SK.REG)], **solver)
    assert torch.equal(alone.coords[0].cpu().reshape(2, -1).t(), ds.samples[0].x_phys)   # whatever shares the launch
    assert alone.steps.item() == res.steps[0].item()


def test_limits_without_the_keyword_are_unchanged(gpu_device):
    with pytest.raises(ValueError, match='32'):
        MeshDataset([33, 33], 2, target='monge_ampere')
    with pytest.raises(ValueError, match='32'):
        ma_batch([33], [SK.CASES['n33_g2'].params])
    with pytest.raises(ValueError, match='81'):
        ma_batch([82], [SK.CASES['n33_g2'].params], **STRIDED)
