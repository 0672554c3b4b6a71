"""The mesh descent on the MI355X (g_adaptivity_amd/descent.py, baselines.py; fem_csrc/descent_kernels.hip): bit-identical to
the loop it replaces, within the project's rule of the fp64 restatement (tests/descent_restatement.py, recorded in
tests/golden/descent/descent.npz), the degenerate calls, the tangling watch, and the baseline models through evaluate_model_fine.

The rule: rel(gpu, fp64) <= max(floor, 1.5 rel(fp32, fp64)), relative max-norm, both restatement runs from the same code;
floor 1e-5 for coordinates, coefficients, sol and losses (the floors of test_gpu_fem1d_sizes.py).  Every case prints its
figures before it asserts."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import descent_restatement as D  # noqa: E402

from g_adaptivity_amd import (Fixed_Mesh_2D, MeshDataset, backFEM_2D, collate, evaluate_model_fine, hot_path_opt, mesh_descent_1d,  # noqa: E402
                              mesh_descent_2d, poisson_eval_errors)
from g_adaptivity_amd.fem import fem_poisson, modular_loss_2d  # noqa: E402
from g_adaptivity_amd.fem1d import gradient_meshpoints_1D  # noqa: E402
from g_adaptivity_amd.mesh_graph import MeshData, square_mesh  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]
DEV = torch.device('cuda:0')
FLOOR = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'descent', 'descent.npz')
_golden = {}


def golden():
    if not _golden:
        _golden.update(np.load(GOLDEN))
    return _golden


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu().reshape(-1), torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _check(label, gpu, f32, f64, floor=FLOOR):
    noise, err = _rel(f32, f64), _rel(gpu, f64)
    print(f"descent {label}: err {err:.3e} noise {noise:.3e}")
    assert bool(torch.isfinite(torch.as_tensor(gpu)).all()), label
    assert err <= max(floor, 1.5 * noise), (label, err, noise)


def _batch_2d(cases):
    """cases: [(x0, mesh, params)] -> (x0 [N,2] on the device, cells, boundary, counts, params)."""
    offs = np.cumsum([0] + [m.num_nodes for _, m, _ in cases[:-1]])
    cells = torch.cat([m.cells + int(o) for (_, m, _), o in zip(cases, offs)], 0)
    bnd = torch.cat([m.boundary_nodes for _, m, _ in cases])
    return torch.cat([x for x, _, _ in cases]).to(DEV), cells, bnd, [m.num_nodes for _, m, _ in cases], [p for _, _, p in cases]


def _det_tol(n):
    """fp32 rounding of a triangle determinant x0 (y1 - y2) + x1 (y2 - y0) + x2 (y0 - y1) on an n x n mesh of the unit square:
    coordinates up to 1, differences up to two cells, six roundings of up to 2^-23 relative on terms of that size."""
    return 6 * 2.0 ** -23 * 2.0 / (n - 1)


# ------------------------------------------------------------------------------------------------------ 2-D
def test_is_the_loop_2d():
    """One call on 5 x 5, 16 x 16, 17 x 17 and 26 x 26 nodes (25, 256, 289, 676 nodes; 32, 450, 512, 1250 triangles: below, at
    and just over a workgroup, and the LDS edge of the factor), one or two Gaussians each: bit-identical to three rounds of
    modular_loss_2d and the torch update."""
    sizes, gauss, epochs, lr = (5, 16, 17, 26), (1, 2, 2, 1), 3, 0.05
    cases = [D.jittered_square(n, 30 + n) + (D.params_2d(k, 60 + n),) for n, k in zip(sizes, gauss)]
    x0, cells, bnd, counts, ps = _batch_2d(cases)
    assert [m.cells.shape[0] for _, m, _ in cases] == [32, 450, 512, 1250] and counts == [25, 256, 289, 676]
    keep = x0.clone()
    res = mesh_descent_2d(x0, cells, bnd, counts, ps, epochs, lr, keep_meshes=True)
    assert torch.equal(x0, keep)                                              # the caller's tensor is not the one that moves
    interior = ~bnd.to(DEV)
    x, losses, meshes = x0.clone(), [], []
    lat = torch.linspace(0, 1, 9)
    for _ in range(epochs):
        coeffs, _ = fem_poisson(x, cells, bnd, counts, ps, (lat, lat))
        loss, gx = modular_loss_2d(x, cells, bnd, counts, ps, 9, 'simpson')
        x = x.clone()
        x[interior] = x[interior] - lr * gx[interior]
        losses.append(loss)
        meshes.append(x)
    assert torch.equal(res.x, x)
    assert torch.equal(res.loss_hist, torch.stack(losses)) and res.loss_hist.shape == (epochs, 4)
    assert torch.equal(res.mesh_hist, torch.stack(meshes))
    assert torch.equal(res.coeffs, coeffs[:, 0])                              # the last epoch's solve: before the last step
    assert torch.equal(res.x[~interior], x0[~interior]) and not torch.equal(res.x[interior], x0[interior])
    assert res.first_tangled.tolist() == [-1] * 4 and bool((res.min_area > 0).all())
    for b, (xb, m, _) in enumerate(cases):                                    # the watch's figure is the mesh's smallest determinant
        o = sum(counts[:b])
        want = D.min_signed_area(res.x[o:o + counts[b]].cpu().double(), m.cells, xb).item()
        assert abs(res.min_area[b].item() - want) <= _det_tol(sizes[b]), (b, res.min_area[b].item(), want)
    # without the history, and one mesh alone: the same bits
    assert torch.equal(mesh_descent_2d(x0, cells, bnd, counts, ps, epochs, lr).x, res.x)
    xb, m, p = cases[2]
    alone = mesh_descent_2d(xb.to(DEV), m.cells, m.boundary_nodes, [m.num_nodes], [p], epochs, lr)
    o = counts[0] + counts[1]
    assert torch.equal(alone.x, res.x[o:o + counts[2]]) and torch.equal(alone.loss_hist[:, 0], res.loss_hist[:, 2])


@pytest.mark.parametrize('n', D.PARITY_2D['sizes'])
def test_parity_2d(n):
    """5 epochs at the reference's lr = 0.2 against the fp64 restatement, whose run does not tangle (the generator of the
    recorded runs refuses one that does)."""
    g = golden()
    x0, m, p = D.parity_case_2d(n)
    assert np.array_equal(g[f'p2d_{n}_x0'], x0.numpy()), "tests/golden/descent/descent.npz is not of this case: rerun its generator"
    res = mesh_descent_2d(x0.to(DEV), m.cells, m.boundary_nodes, [n * n], [p], D.PARITY_2D['epochs'], D.PARITY_2D['lr'])
    assert res.first_tangled.tolist() == [-1]
    for name, got in (('x', res.x), ('coeffs', res.coeffs), ('loss', res.loss_hist[:, 0])):
        _check(f"2-D {n} x {n} {name}", got.cpu(), g[f'p2d_{n}_{name}32'], g[f'p2d_{n}_{name}64'])


def test_degenerate_calls_2d():
    cases = [D.jittered_square(7, 3) + (D.params_2d(2, 4),), D.jittered_square(9, 5) + (D.params_2d(1, 6),)]
    x0, cells, bnd, counts, ps = _batch_2d(cases)
    r0 = mesh_descent_2d(x0, cells, bnd, counts, ps, 0, 0.1, keep_meshes=True)
    assert torch.equal(r0.x, x0) and r0.x.data_ptr() != x0.data_ptr()
    assert r0.loss_hist.shape == (0, 2) and r0.mesh_hist.shape == (0, 130, 2) and r0.coeffs is None
    assert r0.first_tangled.tolist() == [-1, -1]
    r = mesh_descent_2d(x0, cells, bnd, counts, ps, 3, 0.0)
    assert torch.equal(r.x, x0)
    assert torch.equal(r.loss_hist[0], r.loss_hist[1]) and torch.equal(r.loss_hist[1], r.loss_hist[2])   # determinism
    assert bool(torch.isfinite(r.loss_hist).all()) and r.first_tangled.tolist() == [-1, -1]


def test_tangling_watch_2d():
    """x_ref the uniform 5 x 5 mesh; x0 that mesh with one interior node moved across its right neighbour; lr = 0: the first
    step's watch reports it, and the untouched mesh in the same batch reports nothing."""
    m = square_mesh(5)
    x_ref = torch.cat([m.x_comp, m.x_comp])
    bad = m.x_comp.clone()
    v = 2 * 5 + 2                                                            # node (2, 2) at (0.5, 0.5); its right neighbour is at x = 0.75
    assert not bool(m.boundary_nodes[v]) and torch.equal(m.x_comp[v + 5], torch.tensor([0.75, 0.5]))
    bad[v, 0] = 0.8
    cases = [(bad, m, D.params_2d(1, 1)), (m.x_comp.clone(), m, D.params_2d(1, 2))]
    x0, cells, bnd, counts, ps = _batch_2d(cases)
    r = mesh_descent_2d(x0, cells, bnd, counts, ps, 1, 0.0, x_ref=x_ref.to(DEV))
    assert r.first_tangled.tolist() == [0, -1]
    assert r.min_area[0].item() < 0 < r.min_area[1].item()
    assert abs(r.min_area[0].item() - D.min_signed_area(bad.double(), m.cells, m.x_comp).item()) <= _det_tol(5)
    # the default reference is x0 itself: the same start counts as untangled
    assert mesh_descent_2d(x0, cells, bnd, counts, ps, 1, 0.0).first_tangled.tolist() == [-1, -1]


# ------------------------------------------------------------------------------------------------------ 1-D
def test_1d_internal_mixed_sizes():
    """5, 21, 64, 65 and 1024 nodes in one call, 3 epochs, lr = 0.001: against the fp64 restatement under the rule, and against
    the loop over gradient_meshpoints_1D(PDE_loss_direct_L2) with the torch update to 1e-6 relative (that loop sums its loss
    in another order, so it is not bit-identical)."""
    g, c = golden(), D.CASE_1D
    xs, params = D.case_1d()
    sizes, B = list(c['sizes']), len(c['sizes'])
    for x, n in zip(xs, sizes):
        assert np.array_equal(g[f'p1d_{n}_x0'], x.numpy()), "tests/golden/descent/descent.npz is not of this case: rerun its generator"
    x0 = torch.cat(xs).to(DEV)
    res = mesh_descent_1d(x0, sizes, params, c['opt'], c['epochs'], c['lr'], keep_meshes=True)
    assert res.first_tangled.tolist() == [-1] * B and bool((res.min_area > 0).all())
    assert res.sol.shape == (B, 21) and res.loss_hist.shape == (c['epochs'], B) and res.mesh_hist.shape == (c['epochs'], sum(sizes))
    assert torch.equal(res.mesh_hist[-1], res.x)
    off = 0
    for b, n in enumerate(sizes):
        sl = slice(off, off + n)
        assert res.x[off].item() == 0.0 and res.x[off + n - 1].item() == 1.0
        for name, got in (('x', res.x[sl]), ('coeffs', res.coeffs[sl]), ('loss', res.loss_hist[:, b]), ('sol', res.sol[b])):
            _check(f"1-D n={n} {name}", got.cpu(), g[f'p1d_{n}_{name}32'], g[f'p1d_{n}_{name}64'])
        off += n
    # the loop this call replaces
    opt = dict(c['opt'], grad_type='PDE_loss_direct_L2')
    data = MeshData(pde_params=params, _num_graphs=B, batch=torch.repeat_interleave(torch.arange(B), torch.tensor(sizes)))
    inner = torch.ones(sum(sizes), dtype=torch.bool)
    ends = np.cumsum([0] + sizes)
    inner[ends[:-1]] = False
    inner[ends[1:] - 1] = False
    inner = inner.to(DEV)
    x, means = x0.clone(), []
    for _ in range(c['epochs']):
        mean, gx = gradient_meshpoints_1D(opt, data, x)
        x = x.clone()
        x[inner] = x[inner] - c['lr'] * gx[inner]
        means.append(mean)
    ex, el = _rel(res.x, x), _rel(res.loss_hist.mean(1), torch.stack(means))
    print(f"descent 1-D against the gradient_meshpoints_1D loop: x {ex:.3e} mean loss {el:.3e}")
    assert ex <= 1e-6 and el <= 1e-6


def test_1d_all_rescales_and_clips():
    g, c, a = golden(), D.CASE_1D, D.CASE_1D_ALL
    _, params = D.case_1d()
    res = mesh_descent_1d(torch.linspace(0, 1, a['n']).to(DEV), [a['n']], [params[1]], c['opt'], a['epochs'], a['lr'], mesh_params='all',
                          keep_meshes=True)
    for mesh in res.mesh_hist:
        assert mesh[0].item() == 0.0 and mesh[-1].item() == 1.0
    assert res.first_tangled.tolist() == [-1]
    _check("1-D all x", res.x.cpu(), g['all1d_x32'], g['all1d_x64'])
    _check("1-D all loss", res.loss_hist[:, 0].cpu(), g['all1d_loss32'], g['all1d_loss64'])


def test_1d_degenerate_calls_and_watch():
    c = D.CASE_1D
    _, params = D.case_1d()
    x0 = torch.cat([torch.linspace(0, 1, 21), torch.linspace(0, 1, 5)]).to(DEV)
    r0 = mesh_descent_1d(x0, [21, 5], params[:2], c['opt'], 0, 0.1)
    assert torch.equal(r0.x, x0) and r0.loss_hist.shape == (0, 2) and r0.first_tangled.tolist() == [-1, -1] and r0.sol is None
    r = mesh_descent_1d(x0, [21, 5], params[:2], c['opt'], 3, 0.0)
    assert torch.equal(r.x, x0) and torch.equal(r.loss_hist[0], r.loss_hist[2]) and r.first_tangled.tolist() == [-1, -1]
    # two swapped neighbours: the watch reports epoch 0 for that mesh alone
    folded = torch.linspace(0, 1, 21)
    folded[7], folded[8] = folded[8].item(), folded[7].item()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                                     # the forward's "negative diffs" warning
        r = mesh_descent_1d(torch.cat([folded, torch.linspace(0, 1, 5)]).to(DEV), [21, 5], params[:2], c['opt'], 1, 0.0)
        assert r.first_tangled.tolist() == [0, -1] and r.min_area[0].item() < 0 < r.min_area[1].item()


# ------------------------------------------------------------------------------------------------------ models
def _opt(model, n, **kw):
    return hot_path_opt(model=model, mesh_dims=[n, n], device=str(DEV), **kw)


def test_backfem_2d_returns_the_triple():
    ds = MeshDataset([7, 7], 3, seed=5)
    data = collate(ds.samples).to(DEV)
    model = backFEM_2D(_opt('backFEM_2D', 7, epochs=3))
    assert model.lr == 0.2
    model.epoch = 0                                                           # the pipeline's stray attribute writes
    coeffs, coords, sol = model(data)
    want = mesh_descent_2d(data.x_comp, data.cells, data.boundary_nodes, [49] * 3, data.pde_params, 3, 0.2)
    assert torch.equal(coords, want.x) and torch.equal(coeffs, want.coeffs.unsqueeze(1)) and sol is None
    assert model.end_MLmodel is not None and model.loss_list.shape == (3, 3) and model.mesh_list.shape == (3, 147, 2)
    assert torch.equal(model.loss_list, want.loss_hist) and not torch.equal(coords, data.x_comp)


def test_fixed_mesh_2d_pde_loss_is_the_transposed_solve():
    ds = MeshDataset([7, 7], 2, seed=6)
    data = collate(ds.samples).to(DEV)
    model = Fixed_Mesh_2D(_opt('fixed_mesh_2D', 7, loss_type='pde_loss', eval_quad_points=21))
    coeffs, coords, sol = model(data)
    q = torch.linspace(0, 1, 21)
    c_want, s_want = fem_poisson(data.x_comp, data.cells, data.boundary_nodes, [49, 49], data.pde_params, (q, q))
    assert coords is data.x_comp and torch.equal(coeffs, c_want) and model.end_MLmodel is not None
    assert torch.equal(sol, s_want.view(2, 21, 21).transpose(1, 2).reshape(-1))
    assert not torch.equal(sol, s_want)                                       # the Gaussians are not symmetric in x and y


def test_evaluate_model_fine_with_backfem_2d():
    ds = MeshDataset([7, 7], 4, seed=7)
    opt = _opt('backFEM_2D', 7, epochs=3, eval_quad_points=51)
    df, df_time = evaluate_model_fine(backFEM_2D(opt), ds, opt, batch_size=2)
    err = {k: np.asarray(df[k], dtype=np.float64) for k in ('L1_grid', 'L2_grid', 'L1_MA', 'L2_MA', 'L1_MLmodel', 'L2_MLmodel',
                                                           'L1_reduction_MLmodel', 'L2_reduction_MLmodel')}
    for k, v in err.items():
        assert v.shape == (4,) and np.isfinite(v).all(), k
    t = np.asarray(df_time['MLmodel_time'], dtype=np.float64)
    assert t.shape == (4,) and np.isfinite(t).all() and (t > 0).all()
    data = collate(ds.samples).to(DEV)
    x = mesh_descent_2d(data.x_comp, data.cells, data.boundary_nodes, [49] * 4, data.pde_params, 3, opt['lr']).x
    l1, l2 = poisson_eval_errors(x, [49] * 4, data.pde_params, 51, cells=data.cells, boundary=data.boundary_nodes)
    assert np.array_equal(err['L1_MLmodel'], l1.cpu().double().numpy()) and np.array_equal(err['L2_MLmodel'], l2.cpu().double().numpy())
    # the fixed mesh is the grid column itself
    fopt = _opt('fixed_mesh_2D', 7, eval_quad_points=51, solver='torch_FEM')
    dff, _ = evaluate_model_fine(Fixed_Mesh_2D(fopt), ds, fopt, batch_size=4)
    assert np.array_equal(np.asarray(dff['L1_MLmodel'], dtype=np.float64), err['L1_grid'])
