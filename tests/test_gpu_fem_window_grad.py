"""The differentiable windowed FEM route on the MI355X (band='window' of fem_poisson and modular_loss_2d, opt['fem_band'] =
'window' of torch_FEM_2D, GNN.forward with pde_loss and gradient_meshpoints_2D: gadapt_fem_forward_window,
gadapt_fem_modular_forward_window, gadapt_fem_backward_window, fem_csrc/fem_window_grad_kernels.hip).

Rules (the project's own, no new tolerance), each against the fp64 restatement with the fp32 restatement's own deviation from
it as the yardstick:
    loss                 rel <= max(LOSS_FLOOR, 1.5 x fp32 deviation)      (tests/test_gpu_modular2d.py)
    gradient             rel <= max(1e-4, 1.5 x fp32 deviation), _rel of tests/test_gpu_modular2d.py
    coefficients, sol    rel <= max(1e-5, 1.5 x fp32 deviation)            (tests/test_gpu_pde_loss.py)
Windowed calls among themselves - slabs, batches, repeats, a second backward - are compared bitwise.

Where both routes fit (7, 11, 23 a side) the restatements run live, once per mesh, shared by the tests.  At 27, 34 and 64 a side
one call of the restatement takes 12 to 26 s and minutes of CPU, so its loss, gradient and coefficients are stored in
tests/golden/fem_window_grad/n{27,34,64}.npz (make_fem_window_grad_golden.py beside them; 64 x 64 for 'mse' only, which
took five minutes); the tests rebuild the same inputs from the shared recipes and check their checksum against the fixture's.
Every figure is printed before it is asserted (-s); docs/measurements.md has them."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fem_restatement as R  # noqa: E402
import modular2d_restatement as M  # noqa: E402
from test_gpu_evaluation_window import GOLDEN as EVAL_GOLDEN, _check as _check_norms  # noqa: E402  (the evaluation's rule and yardstick)
from test_gpu_modular2d import LOSS_FLOOR, _coords, _params, _rel  # noqa: E402  (the mesh and Gaussian recipes, the floor)

from g_adaptivity_amd import (GNN, MeshDataset, collate, fem_poisson, gradient_meshpoints_2D, hot_path_opt, l1_loss,  # noqa: E402
                              poisson_eval_errors, torch_FEM_2D)
from g_adaptivity_amd import evaluation as ev  # noqa: E402
from g_adaptivity_amd.fem import modular_loss_2d  # noqa: E402
from g_adaptivity_amd.mesh_graph import MeshData, MeshTopology  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
N_LAT = 101
LAT = torch.linspace(0, 1, N_LAT)
QUAD = list(torch.meshgrid(LAT, LAT, indexing='ij'))
FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fem_window_grad')
KINDS = {'mse': ('mse', N_LAT), 'L2': ('simpson', R.SIMPSON_N)}     # restatement kind -> (reduction, n_lat) of modular_loss_2d


def _case(n, kind):
    x, m = _coords(n, kind, seed=n + 1)
    return x, m, _params(2, n)


def _u_true_lattice(p, dtype=torch.float32):
    return R.u_true(M.grid(N_LAT, dtype), p['centers'], p['scales'])


@functools.lru_cache(maxsize=None)
def _live_reference(n, kind):
    """modular2d_restatement.direct_loss for both reductions on one solve (its own operations, the load vector and the dense
    solve shared), in fp64 and fp32: coefficients, sol on the 101 x 101 lattice, both losses and their gradients."""
    x, m, p = _case(n, kind)
    out = {}
    for dt in (torch.float64, torch.float32):
        xx = x.to(dt).clone().requires_grad_(True)
        A, rhs, cells = M._system(xx, m.cells, m.boundary_nodes, p['centers'], p['scales'], R.SIMPSON_N)
        c = torch.linalg.solve(A, rhs.unsqueeze(1)).squeeze(1)
        pts = M.grid(N_LAT, dt)
        sol = M.expand(c, pts, xx, cells)
        mse = torch.nn.functional.mse_loss(sol, R.u_true(pts, p['centers'], p['scales']))
        l2 = M.l2_error(c, xx, cells, p['centers'], p['scales'], R.SIMPSON_N)
        (g_mse,) = torch.autograd.grad(mse, xx, retain_graph=True)
        (g_l2,) = torch.autograd.grad(l2, xx)
        out[dt] = dict(coeffs=c.detach().double(), sol=sol.detach().double(), loss_mse=mse.detach().double(), grad_mse=g_mse.double(),
                       loss_L2=l2.detach().double(), grad_L2=g_l2.double())
    return out[torch.float64], out[torch.float32]


@functools.lru_cache(maxsize=None)
def _fixture(n):
    x, m, p = _case(n, 'jittered')
    z = np.load(os.path.join(FIXTURES, f'n{n}.npz'))
    assert int(z['n']) == n and int(z['n_lat_mse']) == N_LAT and int(z['n_lat_l2']) == R.SIMPSON_N
    assert float(z['coords_sum']) == x.double().sum().item()       # the fixture's mesh
    r64, r32 = {}, {}
    for tag, r in (('64', r64), ('32', r32)):
        r['coeffs'] = torch.from_numpy(z['coeffs' + tag].astype(np.float64))
        for k in KINDS:
            if f'loss{tag}_{k}' in z:
                r['loss_' + k] = torch.tensor(float(z[f'loss{tag}_{k}']), dtype=torch.float64)
                r['grad_' + k] = torch.from_numpy(z[f'grad{tag}_{k}'].astype(np.float64))
    return x, m, p, r64, r32


def _assert_rule(label, what, got, r64, r32, floor):
    dev, own = _rel(got.detach().cpu().double().reshape(r64.shape), r64), _rel(r32, r64)
    print(f"FEM-WINDOW-GRAD {label} {what}: dev {dev:.3e} fp32-restatement dev {own:.3e} bound {max(floor, 1.5 * own):.3e}")
    assert np.isfinite(dev) and dev <= max(floor, 1.5 * own), (label, what, dev, own)


def _poisson(x, m, p, **kw):
    xg = x.to(DEV).requires_grad_(True)
    coeffs, sol = fem_poisson(xg, m.cells, m.boundary_nodes, [m.num_nodes], [p], QUAD, band='window', **kw)
    return xg, coeffs, sol


def _poisson_mse(x, m, p, **kw):
    """fem_poisson(band='window') with the mse loss written in torch: (coeffs, sol, loss, gradient)."""
    xg, coeffs, sol = _poisson(x, m, p, **kw)
    loss = ((sol - _u_true_lattice(p).to(DEV)) ** 2).mean()
    loss.backward()
    return coeffs.detach(), sol.detach(), loss.detach(), xg.grad


def _modular(x, m, p, kind, **kw):
    reduction, n_lat = KINDS[kind]
    return modular_loss_2d(x.to(DEV), m.cells, m.boundary_nodes, [m.num_nodes], [p], n_lat, reduction, band='window', **kw)


# ------------------------------------------------------------------------------------------------ 1. where both routes fit
@pytest.mark.one_dispatch
@pytest.mark.parametrize('kind', ['unmoved', 'jittered'])
@pytest.mark.parametrize('n', [7, 11, 23])
def test_fem_poisson_window_against_restatements(n, kind):
    x, m, p = _case(n, kind)
    r64, r32 = _live_reference(n, kind)
    label = f"n={n} {kind} fem_poisson"
    coeffs, sol, loss, g = _poisson_mse(x, m, p)
    _assert_rule(label, 'coeffs', coeffs, r64['coeffs'], r32['coeffs'], 1e-5)
    _assert_rule(label, 'sol', sol, r64['sol'], r32['sol'], 1e-5)
    _assert_rule(label, 'mse loss', loss, r64['loss_mse'], r32['loss_mse'], LOSS_FLOOR)
    _assert_rule(label, 'mse gradient', g, r64['grad_mse'], r32['grad_mse'], 1e-4)
    again = _poisson_mse(x, m, p)
    for a, b in zip((coeffs, sol, loss, g), again):
        assert torch.equal(a, b)                                   # repeatable


@pytest.mark.one_dispatch
@pytest.mark.parametrize('k', ['mse', 'L2'])
@pytest.mark.parametrize('kind', ['unmoved', 'jittered'])
@pytest.mark.parametrize('n', [7, 11, 23])
def test_modular_loss_window_against_restatements(n, kind, k):
    x, m, p = _case(n, kind)
    r64, r32 = _live_reference(n, kind)
    label = f"n={n} {kind} modular {k}"
    loss, g = _modular(x, m, p, k)
    assert loss.shape == (1,) and g.shape == (n * n, 2)
    _assert_rule(label, 'loss', loss[0], r64['loss_' + k], r32['loss_' + k], LOSS_FLOOR)
    _assert_rule(label, 'gradient', g, r64['grad_' + k], r32['grad_' + k], 1e-4)
    loss2, g2 = _modular(x, m, p, k)
    assert torch.equal(loss, loss2) and torch.equal(g, g2)         # repeatable


# ------------------------------------------------------------------------------------------------ 2. slab edges
@pytest.mark.one_dispatch
@pytest.mark.parametrize('n,tri_slab', [(9, 64), (11, 64), (11, 32)])
def test_slab_edges_bitwise(n, tri_slab):
    """9 x 9: 128 triangles = two full slabs of 64; 11 x 11: 200 = three slabs of 64 and one of 8, or six of 32 and one of 8
    (shorter than a word)."""
    x, m, p = _case(n, 'jittered')
    assert m.cells.shape[0] == 2 * (n - 1) ** 2
    one, slabbed = _poisson_mse(x, m, p), _poisson_mse(x, m, p, tri_slab=tri_slab)
    for name, a, b in zip(('coeffs', 'sol', 'loss', 'x_grads'), one, slabbed):
        assert torch.equal(a, b), name
    for k in KINDS:
        (l1, g1), (l2, g2) = _modular(x, m, p, k), _modular(x, m, p, k, tri_slab=tri_slab)
        assert torch.equal(l1, l2) and torch.equal(g1, g2), k


# ------------------------------------------------------------------------------------------------ 3. beyond the resident band
@pytest.mark.one_dispatch
@pytest.mark.parametrize('n', [27, 34])
def test_first_sizes_beyond_the_resident_band(n):
    """27 x 27: 625 unknowns, band 25, the first size whose factor does not stay resident; 34 x 34: 2178 triangles, two slabs
    by default.  The default route refuses both."""
    x, m, p, r64, r32 = _fixture(n)
    got = {}
    for k in KINDS:
        loss, g = got[k] = _modular(x, m, p, k)
        label = f"n={n} jittered modular {k}"
        print(f"FEM-WINDOW-GRAD {label}: loss {loss.item():.9e} fp64 {r64['loss_' + k].item():.9e}")
        _assert_rule(label, 'loss', loss[0], r64['loss_' + k], r32['loss_' + k], LOSS_FLOOR)
        _assert_rule(label, 'gradient', g, r64['grad_' + k], r32['grad_' + k], 1e-4)
    label = f"n={n} jittered fem_poisson"
    coeffs, sol, loss, g = _poisson_mse(x, m, p)
    assert bool(torch.isfinite(sol).all())
    _assert_rule(label, 'coeffs', coeffs, r64['coeffs'], r32['coeffs'], 1e-5)
    _assert_rule(label, 'mse loss', loss, r64['loss_mse'], r32['loss_mse'], LOSS_FLOOR)
    _assert_rule(label, 'mse gradient', g, r64['grad_mse'], r32['grad_mse'], 1e-4)
    with pytest.raises(NotImplementedError, match='LDS'):
        fem_poisson(x.to(DEV), m.cells, m.boundary_nodes, [m.num_nodes], [p], QUAD)
    with pytest.raises(NotImplementedError, match='LDS'):
        modular_loss_2d(x.to(DEV), m.cells, m.boundary_nodes, [m.num_nodes], [p], N_LAT, 'mse')
    for a, b in zip((coeffs, sol, loss, g), _poisson_mse(x, m, p, tri_slab=512)):    # more slabs, the same sums
        assert torch.equal(a, b)
    for k in KINDS:
        l2, g2 = _modular(x, m, p, k, tri_slab=512)
        assert torch.equal(l2, got[k][0]) and torch.equal(g2, got[k][1]), k


# ------------------------------------------------------------------------------------------------ 4. backward twice
@pytest.mark.one_dispatch
def test_backward_twice_on_one_forward():
    """The adjoint solve rewrites the mesh's y slot of the kept workspace and only reads the factor: no trace is left."""
    x, m, p = _case(27, 'jittered')
    xg, coeffs, sol = _poisson(x, m, p)
    loss = ((sol - _u_true_lattice(p).to(DEV)) ** 2).mean() + coeffs.sum() * 1e-6
    loss.backward(retain_graph=True)
    first = xg.grad.clone()
    xg.grad = None
    loss.backward(retain_graph=True)
    assert bool(torch.isfinite(first).all()) and first.abs().max().item() > 0
    assert torch.equal(xg.grad, first)


# ------------------------------------------------------------------------------------------------ 5. batches
@pytest.mark.one_dispatch
def test_mixed_batch_bitwise_equal_to_single_mesh_calls():
    """11 and 34 a side in one call: the small mesh runs with the ring slack of the large one's launch."""
    cases = [_case(11, 'jittered'), _case(34, 'jittered')]
    xs, ms, ps = zip(*cases)
    counts = [m.num_nodes for m in ms]
    cells = torch.cat([ms[0].cells, ms[1].cells + counts[0]], 0)
    bnd = torch.cat([m.boundary_nodes for m in ms])
    xb = torch.cat(xs).to(DEV)
    coeffs, sol = fem_poisson(xb, cells, bnd, counts, list(ps), QUAD, band='window')
    batch = {k: modular_loss_2d(xb, cells, bnd, counts, list(ps), KINDS[k][1], KINDS[k][0], band='window') for k in KINDS}
    off = 0
    for b, (x, m, p) in enumerate(cases):
        _, c1, s1 = _poisson(x, m, p)
        assert torch.equal(coeffs[off:off + counts[b]], c1.detach()), b
        assert torch.equal(sol[b * N_LAT * N_LAT:(b + 1) * N_LAT * N_LAT], s1.detach()), b
        for k in KINDS:
            l1, g1 = _modular(x, m, p, k)
            assert torch.equal(batch[k][0][b:b + 1], l1), (b, k)
            assert torch.equal(batch[k][1][off:off + counts[b]], g1), (b, k)
        off += counts[b]


# ------------------------------------------------------------------------------------------------ 6. boundary rows
def _u_true_nodes(x, p):
    """u_true at the nodes x [N,2] in fp32 on the device, operation by operation as the load vector's boundary rows."""
    out = torch.zeros(x.shape[0], device=x.device)
    for c, s in zip(p['centers'], p['scales']):
        c0, c1, s0, s1 = (torch.tensor(float(v), dtype=torch.float32, device=x.device) for v in (c[0], c[1], s[0], s[1]))
        d0, d1 = x[:, 0] - c0, x[:, 1] - c1
        out = out + torch.exp(-(d0 * d0) / (s0 * s0) - (d1 * d1) / (s1 * s1))
    return out


@pytest.mark.one_dispatch
def test_boundary_rows():
    # the default route's boundary coefficients are u_true at the node, bitwise, and so written in torch
    x, m, p = _case(11, 'jittered')
    c_lds, _ = fem_poisson(x.to(DEV), m.cells, m.boundary_nodes, [m.num_nodes], [p], QUAD)
    bnd = m.boundary_nodes.to(DEV)
    assert torch.equal(c_lds.view(-1)[bnd], _u_true_nodes(x.to(DEV), p)[bnd])
    _, c_win, _ = _poisson(x, m, p)
    assert torch.equal(c_win.detach().view(-1)[bnd], c_lds.view(-1)[bnd])
    # 27 x 27: the same on the windowed route; mu = 0 there, the gradient finite everywhere
    x, m, p = _case(27, 'jittered')
    coeffs, _, _, g = _poisson_mse(x, m, p)
    bnd = m.boundary_nodes.to(DEV)
    assert torch.equal(coeffs.view(-1)[bnd], _u_true_nodes(x.to(DEV), p)[bnd])
    assert bool(torch.isfinite(g).all())
    for k in KINDS:
        loss, gx = _modular(x, m, p, k)
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(gx).all()), k


# ------------------------------------------------------------------------------------------------ 7. the metric workload's size
@pytest.mark.one_dispatch
def test_metric_workload_size_64():
    """One forward and backward at 64 x 64 on the mesh and Gaussians of tests/golden/eval_window/yardstick.npz.  The
    trapezium norms of fem_poisson's sol (fp64 sums in torch of the fp32 e = sol - u_true) against poisson_eval_errors on the
    same mesh - the same coefficients and the same chain of additions per point, only the fp32 reduction differs - and against
    the stored fp64 yardstick under the evaluation's rule; loss and gradient against the 64 x 64 fixture ('mse')."""
    n = 64
    x, m, p, r64, r32 = _fixture(n)
    z = np.load(EVAL_GOLDEN)
    assert float(z[f'coords_sum_n{n}']) == x.double().sum().item() and int(z['n_eval']) == N_LAT
    loss, g = _modular(x, m, p, 'mse')
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(g).all())
    label = "n=64 jittered modular mse"
    print(f"FEM-WINDOW-GRAD {label}: loss {loss.item():.9e} fp64 {r64['loss_mse'].item():.9e}")
    _assert_rule(label, 'loss', loss[0], r64['loss_mse'], r32['loss_mse'], LOSS_FLOOR)
    _assert_rule(label, 'gradient', g, r64['grad_mse'], r32['grad_mse'], 1e-4)
    # the evaluation's lattice (np.linspace in fp64, rounded to fp32), so that both calls see the same points
    lat = ev.eval_lattice(N_LAT).float()
    xg = x.to(DEV).requires_grad_(True)
    coeffs, sol = fem_poisson(xg, m.cells, m.boundary_nodes, [m.num_nodes], [p], [lat, lat], band='window')
    assert bool(torch.isfinite(coeffs).all()) and bool(torch.isfinite(sol).all())
    _assert_rule("n=64 jittered fem_poisson", 'coeffs', coeffs, r64['coeffs'], r32['coeffs'], 1e-5)
    pts = torch.stack([t.reshape(-1) for t in torch.meshgrid(lat, lat, indexing='ij')], 1).to(DEV)
    e = (sol.detach() - _u_true_nodes(pts, p)).double().view(N_LAT, N_LAT)
    w1 = torch.ones(N_LAT, dtype=torch.float64, device=DEV)
    w1[0] = w1[-1] = 0.5
    w = w1[:, None] * w1[None, :]
    h = (lat[-1].double() - lat[0].double()).item() / (N_LAT - 1)
    l1, l2 = (h * h * (w * e.abs()).sum()).item(), torch.sqrt(h * h * (w * e * e).sum()).item()
    e1, e2 = poisson_eval_errors(x.to(DEV), [m.num_nodes], [p], N_LAT, cells=m.cells, boundary=m.boundary_nodes, band='window')
    for name, a, b in (('L1', l1, e1.item()), ('L2', l2, e2.item())):
        dev = abs(a - b) / abs(b)
        print(f"FEM-WINDOW-GRAD n=64 {name}: from sol {a:.9e} poisson_eval_errors {b:.9e} dev {dev:.3e}")
        assert dev <= LOSS_FLOOR, (name, dev)
    _check_norms("n=64 jittered, norms of fem_poisson's sol", [l1, l2], z[f'e64_n{n}'].tolist(), z[f'e32_n{n}'].tolist())
    sol.square().mean().backward()
    assert bool(torch.isfinite(xg.grad).all())


# ------------------------------------------------------------------------------------------------ 8. the callers
def test_gnn_pde_loss_window():
    n = 27
    ds = MeshDataset([n, n], 2, seed=7, pde_loss_fields=True)
    opt = hot_path_opt(mesh_dims=[n, n], hidden_dim=8, num_layers=4, time_step=0.1, loss_type='pde_loss', loss_fn='l1',
                       device=str(DEV))
    assert opt['fem_band'] == 'lds'
    torch.manual_seed(0)
    dd = collate(ds.samples).to(DEV)
    with pytest.raises(NotImplementedError, match='LDS'):
        GNN(ds, {k: v for k, v in opt.items() if k != 'fem_band'}).to(DEV)(dd)
    torch.manual_seed(0)
    model = GNN(ds, dict(opt, fem_band='window')).to(DEV).train()
    coeffs, x_phys, sol = model(dd)
    assert coeffs.shape == (2 * n * n, 1) and sol.shape == (2 * N_LAT * N_LAT,)
    c2, s2 = fem_poisson(x_phys.detach(), dd.cells, dd.boundary_nodes, [n * n, n * n], list(dd.pde_params), model.quad_points,
                         band='window')
    assert torch.equal(coeffs.detach(), c2) and torch.equal(sol.detach(), s2)
    l1_loss(sol.view(-1, 1), dd.u_true_fine_tensor.view(-1, 1)).backward()
    grads = [prm.grad for prm in model.parameters() if prm.grad is not None]
    assert grads and all(bool(torch.isfinite(gr).all()) for gr in grads)
    assert any(gr.abs().max().item() > 0 for gr in grads)


@pytest.mark.one_dispatch
def test_modular_and_torch_fem_callers():
    n = 27
    cases = [_case(n, 'jittered'), _case(n, 'unmoved')]
    xs, ms, _ = zip(*cases)
    ps = [_params(2, 3), _params(1, 4)]
    counts = [n * n, n * n]
    cells = torch.cat([ms[0].cells, ms[1].cells + counts[0]], 0)
    bnd = torch.cat([mm.boundary_nodes for mm in ms])
    batch = torch.repeat_interleave(torch.arange(2), torch.tensor(counts))
    data = MeshData(cells=cells, boundary_nodes=bnd, pde_params=ps, batch=batch, _num_graphs=2)
    x = torch.cat(xs).to(DEV)
    for gt, (reduction, n_lat) in (('PDE_loss_direct_mse', KINDS['mse']), ('PDE_loss_direct_L2', KINDS['L2'])):
        opt = dict(grad_type=gt, mesh_dims=[n, n], eval_quad_points=101, load_quad_points=101)
        with pytest.raises(NotImplementedError, match='LDS'):
            gradient_meshpoints_2D(opt, data, x)
        mean, g = gradient_meshpoints_2D(dict(opt, fem_band='window'), data, x)
        loss, g2 = modular_loss_2d(x, cells, bnd, counts, ps, n_lat, reduction, band='window')
        assert mean.dim() == 0 and torch.equal(mean, loss.mean()) and torch.equal(g, g2), gt
    x1, m1, p1 = cases[0]
    mesh = MeshTopology(m1.cells.numpy())
    args = (mesh, x1.to(DEV), QUAD, n, [torch.from_numpy(c) for c in p1['centers']], [torch.from_numpy(s) for s in p1['scales']])
    with pytest.raises(NotImplementedError, match='LDS'):
        torch_FEM_2D({'device': DEV}, *args)
    coeffs, pts, sol = torch_FEM_2D({'device': DEV, 'fem_band': 'window'}, *args)
    assert coeffs.shape == (n * n, 1) and sol.shape == (N_LAT, N_LAT) and bool(torch.isfinite(sol).all())
    _, c2, s2 = _poisson(x1, m1, p1)
    assert torch.equal(coeffs, c2.detach()) and torch.equal(sol.reshape(-1), s2.detach())


# ------------------------------------------------------------------------------------------------ 9. refusals
@pytest.mark.one_dispatch
def test_refusals_before_any_launch():
    x, m, p = _case(9, 'unmoved')
    xd = x.to(DEV)
    for tri_slab in (-32, 48, 1):
        with pytest.raises(ValueError, match='tri_slab'):
            fem_poisson(xd, m.cells, m.boundary_nodes, [m.num_nodes], [p], QUAD, band='window', tri_slab=tri_slab)
        with pytest.raises(ValueError, match='tri_slab'):
            modular_loss_2d(xd, m.cells, m.boundary_nodes, [m.num_nodes], [p], N_LAT, 'mse', band='window', tri_slab=tri_slab)
    with pytest.raises(ValueError, match='band'):
        fem_poisson(xd, m.cells, m.boundary_nodes, [m.num_nodes], [p], QUAD, band='ring')
    with pytest.raises(ValueError, match='band'):
        modular_loss_2d(xd, m.cells, m.boundary_nodes, [m.num_nodes], [p], N_LAT, 'mse', band='ring')
    data = MeshData(cells=m.cells, boundary_nodes=m.boundary_nodes, pde_params=[p])
    with pytest.raises(ValueError, match='band'):
        gradient_meshpoints_2D(dict(grad_type='PDE_loss_direct_mse', mesh_dims=[9, 9], fem_band='ring'), data, xd)
    x, m, p = _case(82, 'unmoved')
    with pytest.raises(NotImplementedError, match='81 x 81'):
        fem_poisson(x.to(DEV), m.cells, m.boundary_nodes, [m.num_nodes], [p], QUAD, band='window')
    with pytest.raises(NotImplementedError, match='81 x 81'):
        modular_loss_2d(x.to(DEV), m.cells, m.boundary_nodes, [m.num_nodes], [p], N_LAT, 'mse', band='window')
