"""The 2-D FEM tail on the MI355X on evaluation lattices other than 101 x 101 (fem_csrc/fem_kernels.hip,
fem_window_kernels.hip, fem_window_grad_kernels.hip through fem_poisson, modular_loss_2d, poisson_eval_errors and the GNN's
pde_loss tail).  The cases, the lattices and the reference are tests/fem_lattices.py's; tests/test_fem_lattices_host.py holds
what they must satisfy without a GPU.

    u2, C (nlat = 2)       Q = 4 points for the 8 chunks of the evaluation: empty chunks, every triangle's lattice window is
                           the whole lattice
    u3, u4                 fewer points than lanes; the Simpson row rule at its smallest
    u16, u17, u33          u17 and u33 put every lattice point on a border of the 16 x 16 bin grid
    u255, u256, u257       the second trip of fem_loss_kernel's one-lane-per-row loop; more rows than lanes
    A                      a lattice larger than the mesh: triangles clamp into inner bins, points outside give sol = 0.0
    B                      a sub-window with lat[0] != 0 and another extent per axis: triangles wholly outside the lattice
                           clamp into edge bins, scx != scy, lattice_range with a nonzero lo and empty windows
    u359, band='window'    the running sums of the slabbed evaluation leave one mask word: a forced 32-triangle slab (J5: one
                           slab, J7: 32 + 32 + 8); a 64-triangle slab and u360 are refused before anything is launched

Rules (the project's own through _assert_rule of tests/test_gpu_fem_window_grad.py, no new tolerance), each against the fp64
restatement with the fp32 restatement's own deviation from it as the yardstick:
    loss                          rel <= max(LOSS_FLOOR, 1.5 x fp32 deviation)
    coefficients, sol             rel <= max(1e-5, 1.5 x fp32 deviation)
    gradient, all nodes           rel <= max(1e-4, 1.5 x fp32 deviation)
    gradient, interior nodes      the same rule on the interior rows alone; the host test caps the fp32 deviation there at
                                  6.6e-5, so this bar is 1e-4 (tests/fem_lattices.py says why the all-node one is loose)
    error norms                   tests/test_gpu_evaluation.py::_check; on u2 the yardstick is exactly 0 and both norms get
                                  8 x 2^-23 x max |u_true(corners)|: a few fp32 roundings of one value, L1 = L2^2 = the mean
                                  corner error there
Batches, slabs and repeats are compared bitwise.  Every figure is printed before it is asserted (-s; grep FEM-LATTICES);
docs/measurements.md has them."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_restatement as E  # noqa: E402
import fem_lattices as L  # noqa: E402
import fem_restatement as R  # noqa: E402
from test_gpu_evaluation import _check as _check_norms  # noqa: E402  (the evaluation's rule)
from test_gpu_fem_window_grad import _assert_rule  # noqa: E402  (the rule)
from test_gpu_modular2d import LOSS_FLOOR  # noqa: E402

from g_adaptivity_amd import GNN, MeshDataset, collate, fem_poisson, gradient_meshpoints_2D, hot_path_opt, poisson_eval_errors  # noqa: E402
from g_adaptivity_amd._native import NativeError  # noqa: E402
from g_adaptivity_amd.fem import modular_loss_2d  # noqa: E402
from g_adaptivity_amd.mesh_graph import MeshData  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BANDS = ('lds', 'window')
IDS = [f"{m}-{lat}" for m, lat in L.CASES]
NO_ROOM, SLAB_MASK = 'running sums leave no room', "tri_slab's bin mask exceeds"


def _quad(lat):
    """The lattice as GNN.quad_points has it: [X, Y] of meshgrid 'ij'."""
    return list(torch.meshgrid(*L.axes(lat), indexing='ij'))


def _poisson_grad(mesh, lat, band, **kw):
    """fem_poisson on the case and the gradient of sol . w_sol + coeffs . w_c: (coeffs [N], sol [Q], gradient [N,2])."""
    x, m = L.mesh(mesh)
    w_sol, w_c = L.weights(mesh, lat)
    xg = x.to(DEV).requires_grad_(True)
    coeffs, sol = fem_poisson(xg, m.cells, m.boundary_nodes, [m.num_nodes], [L.params(mesh, lat)], _quad(lat), band=band, **kw)
    ((sol * w_sol.to(DEV)).sum() + (coeffs.view(-1) * w_c.to(DEV)).sum()).backward()
    return coeffs.detach().view(-1), sol.detach(), xg.grad


def _modular(mesh, lat, reduction, band, **kw):
    x, m = L.mesh(mesh)
    return modular_loss_2d(x.to(DEV), m.cells, m.boundary_nodes, [m.num_nodes], [L.params(mesh, lat)], L.unit_k(lat), reduction, band=band,
                           **kw)


def _rule(label, what, got, r64, r32, floor):
    _assert_rule("FEM-LATTICES " + label, what, got, r64, r32, floor)


def _gradient_rules(label, mesh, g, r64, r32):
    """The all-node rule, then the same on the interior nodes (the host test's cap makes that bar 1e-4)."""
    interior = ~L.mesh(mesh)[1].boundary_nodes
    g = g.detach().cpu().double()
    assert g.shape == r64.shape and bool(torch.isfinite(g).all())
    _rule(label, 'gradient, all nodes', g, r64, r32, 1e-4)
    _rule(label, 'gradient, interior nodes', g[interior], r64[interior], r32[interior], 1e-4)


def _poisson_against_fp64(mesh, lat, band, **kw):
    r64, r32 = L.reference(mesh, lat)
    label = f"{mesh} {lat} band={band} fem_poisson"
    coeffs, sol, g = _poisson_grad(mesh, lat, band, **kw)
    assert sol.shape == r64['sol'].shape
    _rule(label, 'coeffs', coeffs, r64['coeffs'], r32['coeffs'], 1e-5)
    _rule(label, 'sol', sol, r64['sol'], r32['sol'], 1e-5)
    if lat != 'u2':                                        # u2: sol alone, the four corner coefficients (fem_lattices.py)
        _gradient_rules(label, mesh, g, r64['grad_w'], r32['grad_w'])
    return coeffs, sol, g


def _modular_against_fp64(mesh, lat, reduction, band, **kw):
    r64, r32 = L.reference(mesh, lat)
    label = f"{mesh} {lat} band={band} modular {reduction}"
    loss, g = _modular(mesh, lat, reduction, band, **kw)
    assert loss.shape == (1,)
    print(f"FEM-LATTICES {label}: loss {loss.item():.9e} fp64 {r64['loss_' + reduction].item():.9e}")
    _rule(label, 'loss', loss[0], r64['loss_' + reduction], r32['loss_' + reduction], LOSS_FLOOR)
    _gradient_rules(label, mesh, g, r64['grad_' + reduction], r32['grad_' + reduction])
    return loss, g


# ------------------------------------------------------------------------------------------------ 1. against fp64
@pytest.mark.one_dispatch
@pytest.mark.parametrize('band', BANDS)
@pytest.mark.parametrize('mesh,lat', L.CASES, ids=IDS)
def test_fem_poisson_against_fp64(mesh, lat, band):
    _, sol, _ = _poisson_against_fp64(mesh, lat, band)
    if lat == 'A':                                         # exactly 0.0 wherever the reference puts the point outside the mesh
        pts = L.points(*L.axes(lat), torch.float64)
        outside = ((pts < 0) | (pts > 1)).any(0)
        assert int(outside.sum()) > 0 and bool((L.reference(mesh, lat)[0]['sol'][outside] == 0).all())
        assert bool((sol.cpu()[outside] == 0.0).all())


LOSS_CASES = [(m, lat, red) for m, lat in L.CASES for red in ('mse', 'simpson')
              if L.has_loss(lat) and (red == 'mse' or L.has_simpson(lat))]


@pytest.mark.one_dispatch
@pytest.mark.parametrize('band', BANDS)
@pytest.mark.parametrize('mesh,lat,reduction', LOSS_CASES, ids=[f"{m}-{lat}-{red}" for m, lat, red in LOSS_CASES])
def test_modular_loss_against_fp64(mesh, lat, reduction, band):
    """u255, u256 and u257 give fem_loss_kernel's row loop its second trip."""
    _modular_against_fp64(mesh, lat, reduction, band)


@functools.lru_cache(maxsize=None)
def _eval_reference(mesh, k):
    x, m = L.mesh(mesh)
    p = L.params(mesh, f'u{k}')
    args = (x, m.cells, m.boundary_nodes, p['centers'], p['scales'], k)
    return E.errors_2d(*args, torch.float64), E.errors_2d(*args, torch.float32)


def _eval_errors(mesh, k, band, **kw):
    x, m = L.mesh(mesh)
    l1, l2 = poisson_eval_errors(x.to(DEV), [m.num_nodes], [L.params(mesh, f'u{k}')], k, cells=m.cells, boundary=m.boundary_nodes, band=band,
                                 **kw)
    return [l1.item(), l2.item()]


EVAL_CASES = [('J5', k, 'lds') for k in (3, 16, 17, 255, 256, 257)] + [('J7', 3, 'lds'), ('J7', 17, 'lds')] + \
             [(m, L.K_LIMIT, 'window') for m in L.MESHES]


@pytest.mark.one_dispatch
@pytest.mark.parametrize('mesh,k,band', EVAL_CASES, ids=[f"{m}-u{k}-{b}" for m, k, b in EVAL_CASES])
def test_poisson_eval_errors_against_yardstick(mesh, k, band):
    e64, e32 = _eval_reference(mesh, k)
    got = _eval_errors(mesh, k, band)
    assert np.isfinite(got).all()
    _check_norms(f"FEM-LATTICES {mesh} u{k} band={band}", got, e64, e32)


@pytest.mark.one_dispatch
@pytest.mark.parametrize('band', BANDS)
def test_poisson_eval_errors_on_the_corner_lattice(band):
    """u2: the yardstick is exactly 0 (sol at a corner is that node's coefficient, u_true there)."""
    e64, e32 = _eval_reference('J5', 2)
    assert e64 == (0.0, 0.0) and e32 == (0.0, 0.0)
    p = L.params('J5', 'u2')
    bar = 8 * 2.0 ** -23 * R.u_true(L.points(*L.axes('u2'), torch.float64), p['centers'], p['scales']).abs().max().item()
    got = _eval_errors('J5', 2, band)
    print(f"FEM-LATTICES J5 u2 band={band} error norms: L1 {got[0]:.3e} L2 {got[1]:.3e} bar {bar:.3e}")
    assert np.isfinite(got).all() and 0.0 <= got[0] <= bar and 0.0 <= got[1] <= bar, (got, bar)


# ------------------------------------------------------------------------------------------------ 2. the window limit
@pytest.mark.one_dispatch
@pytest.mark.parametrize('mesh', list(L.MESHES))
def test_window_limit(mesh):
    """u359 on band='window': 64 444 B of running sums and one mask word of 1024 B in the 64 KB budget."""
    k = L.K_LIMIT
    lat = f'u{k}'
    x, m = L.mesh(mesh)
    p = L.params(mesh, lat)
    first = _poisson_against_fp64(mesh, lat, 'window')
    loss, g = _modular_against_fp64(mesh, lat, 'mse', 'window')
    if m.cells.shape[0] > 32:                              # J7: the default plan's slab is the 32 an explicit one asks for
        for a, b in zip(first, _poisson_grad(mesh, lat, 'window', tri_slab=32)):
            assert torch.equal(a, b)
        loss32, g32 = _modular(mesh, lat, 'mse', 'window', tri_slab=32)
        assert torch.equal(loss32, loss) and torch.equal(g32, g)
    # refused before anything is launched: a slab of two mask words at u359, and u360 with any slab
    xd = x.to(DEV)
    args = (xd, m.cells, m.boundary_nodes, [m.num_nodes], [p])
    with pytest.raises(NativeError, match=SLAB_MASK):
        fem_poisson(*args, _quad(lat), band='window', tri_slab=64)
    with pytest.raises(NativeError, match=SLAB_MASK):
        modular_loss_2d(*args, k, 'mse', band='window', tri_slab=64)
    with pytest.raises(NativeError, match=SLAB_MASK):
        poisson_eval_errors(xd, [m.num_nodes], [p], k, cells=m.cells, boundary=m.boundary_nodes, band='window', tri_slab=64)
    for slab in (0, 32):
        with pytest.raises(NativeError, match=NO_ROOM):
            fem_poisson(*args, _quad(f'u{k + 1}'), band='window', tri_slab=slab)
        with pytest.raises(NativeError, match=NO_ROOM):
            modular_loss_2d(*args, k + 1, 'mse', band='window', tri_slab=slab)
        with pytest.raises(NativeError, match=NO_ROOM):
            poisson_eval_errors(xd, [m.num_nodes], [p], k + 1, cells=m.cells, boundary=m.boundary_nodes, band='window', tri_slab=slab)
    # a valid call after the refusals: the earlier bits
    for a, b in zip(first, _poisson_grad(mesh, lat, 'window')):
        assert torch.equal(a, b)
    loss2, g2 = _modular(mesh, lat, 'mse', 'window')
    assert torch.equal(loss2, loss) and torch.equal(g2, g)


# ------------------------------------------------------------------------------------------------ 3. bitwise
@pytest.mark.one_dispatch
@pytest.mark.parametrize('band', BANDS)
@pytest.mark.parametrize('lat', ['B', 'u3'])
def test_batch_bitwise_equal_to_single_mesh_calls(lat, band):
    """J5 + J7 in one call: every mesh as in its own call, and each call as its repeat."""
    names = list(L.MESHES)
    xs, ms = zip(*[L.mesh(nm) for nm in names])
    ps = [L.params(nm, lat) for nm in names]
    counts = [m.num_nodes for m in ms]
    offs = np.cumsum([0] + counts[:-1]).tolist()
    cells = torch.cat([m.cells + o for m, o in zip(ms, offs)], 0)
    bnd = torch.cat([m.boundary_nodes for m in ms])
    ws = [L.weights(nm, lat) for nm in names]
    w_sol, w_c = torch.cat([w[0] for w in ws]).to(DEV), torch.cat([w[1] for w in ws]).to(DEV)
    Q = L.axes(lat)[0].numel() ** 2

    def batch_call():
        xg = torch.cat(xs).to(DEV).requires_grad_(True)
        coeffs, sol = fem_poisson(xg, cells, bnd, counts, ps, _quad(lat), band=band)
        ((sol * w_sol).sum() + (coeffs.view(-1) * w_c).sum()).backward()
        out = [coeffs.detach().view(-1), sol.detach(), xg.grad]
        if L.has_loss(lat):
            for red in ('mse', 'simpson'):
                out += list(modular_loss_2d(xg.detach(), cells, bnd, counts, ps, L.unit_k(lat), red, band=band))
        return out

    batch = batch_call()
    for a, b in zip(batch, batch_call()):
        assert torch.equal(a, b)
    for i, (nm, off) in enumerate(zip(names, offs)):
        single = _poisson_grad(nm, lat, band)
        for a, b in zip(single, _poisson_grad(nm, lat, band)):
            assert torch.equal(a, b), (nm, 'repeat')
        assert torch.equal(batch[0][off:off + counts[i]], single[0]), (nm, 'coeffs')
        assert torch.equal(batch[1][i * Q:(i + 1) * Q], single[1]), (nm, 'sol')
        assert torch.equal(batch[2][off:off + counts[i]], single[2]), (nm, 'gradient')
        assert bool(torch.isfinite(single[2]).all()) and single[2].abs().max().item() > 0
        if L.has_loss(lat):
            for j, red in enumerate(('mse', 'simpson')):
                loss, g = _modular(nm, lat, red, band)
                loss_r, g_r = _modular(nm, lat, red, band)
                assert torch.equal(loss, loss_r) and torch.equal(g, g_r), (nm, red, 'repeat')
                assert torch.equal(batch[3 + 2 * j][i:i + 1], loss), (nm, red, 'loss')
                assert torch.equal(batch[4 + 2 * j][off:off + counts[i]], g), (nm, red, 'gradient')


# ------------------------------------------------------------------------------------------------ 4. callers
def test_gnn_pde_loss_tail_on_a_17_point_lattice():
    """eval_quad_points = 17 reaches the kernels through GNN.quad_points: the model's sol is fem_poisson's on that lattice."""
    n, k, B = 7, 17, 2
    ds = MeshDataset([n, n], B, seed=7, pde_loss_fields=True, eval_quad_points=k)
    opt = hot_path_opt(mesh_dims=[n, n], hidden_dim=8, num_layers=4, time_step=0.1, loss_type='pde_loss', loss_fn='l1',
                       eval_quad_points=k, device=str(DEV))
    torch.manual_seed(0)
    model = GNN(ds, opt).to(DEV)
    assert model.quad_points[0].shape == (k, k) and torch.equal(model.quad_points[0][:, 0], torch.linspace(0, 1, k))
    dd = collate(ds.samples).to(DEV)
    coeffs, x_phys, sol = model(dd)
    assert coeffs.shape == (B * n * n, 1) and sol.shape == (B * k * k,) and bool(torch.isfinite(sol).all())
    c2, s2 = fem_poisson(x_phys.detach(), dd.cells, dd.boundary_nodes, [n * n] * B, dd.pde_params, model.quad_points)
    assert torch.equal(sol.detach(), s2) and torch.equal(coeffs.detach(), c2)
    assert dd.u_true_fine_tensor.numel() == sol.numel()


@pytest.mark.one_dispatch
def test_gradient_meshpoints_2d_refuses_a_5_point_load_vector():
    """PDE_loss_direct_mse reads eval_quad_points for the load vector too: 33 -> 5 Simpson points, and 9 are built."""
    x, m = L.mesh('J5')
    data = MeshData(cells=m.cells, boundary_nodes=m.boundary_nodes, pde_params=[L.params('J5', 'u33')])
    opt = dict(grad_type='PDE_loss_direct_mse', mesh_dims=[5, 5], eval_quad_points=33, load_quad_points=101)
    with pytest.raises(NotImplementedError, match=r'built for 9 points per dimension only \(got 5\)'):
        gradient_meshpoints_2D(opt, data, x.to(DEV))
