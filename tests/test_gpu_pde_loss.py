"""loss_type='pde_loss' on the MI355X: the FEM tail (g_adaptivity_amd/fem.py, libgadapt_fem.so) against the test-side
restatement of the reference's differentiable FEM (tests/fem_restatement.py), and the model trained through it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fem_restatement as R  # noqa: E402

from g_adaptivity_amd import GNN, MeshDataset, collate, fem_poisson, hot_path_opt, l1_loss, torch_FEM_2D  # noqa: E402
from g_adaptivity_amd.mesh_graph import MeshTopology, square_mesh  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
LAT = torch.linspace(0, 1, 101)
QUAD = list(torch.meshgrid(LAT, LAT, indexing='ij'))


def _params(k, seed):
    rng = np.random.default_rng(seed)
    return {'centers': [rng.uniform(0, 1, 2).astype('f') for _ in range(k)],
            'scales': [rng.uniform(0.1, 0.5, 2).astype('f') for _ in range(k)]}


def _coords(n, kind, seed=0):
    m = square_mesh(n)
    x = m.x_comp.clone()
    if kind == 'jittered':
        g = torch.Generator().manual_seed(seed)
        d = (torch.rand(x.shape, generator=g) * 2 - 1) * 0.2 / (n - 1)
        d[m.boundary_nodes] = 0.0
        x = x + d
    elif kind == 'folded':
        # an interior node pushed past its neighbour: its triangles overlap theirs, lattice points lie in two triangles
        i = (n // 2) * n + n // 2
        x[i, 0] += 1.3 / (n - 1)
    return x, m


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def _gpu(xs, meshes, params):
    cells = torch.cat([m.cells + off for m, off in zip(meshes, np.cumsum([0] + [mm.num_nodes for mm in meshes[:-1]]))], 0)
    bnd = torch.cat([m.boundary_nodes for m in meshes])
    x = torch.cat(xs).to(DEV).requires_grad_(True)
    coeffs, sol = fem_poisson(x, cells, bnd, [m.num_nodes for m in meshes], params, QUAD)
    return x, coeffs, sol


def _ref(x, m, p, dtype):
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    c, s = R.fem2d(xx, m.cells, m.boundary_nodes, p['centers'], p['scales'], LAT.to(dtype))
    return xx, c, s


@pytest.mark.one_dispatch
@pytest.mark.parametrize('n', [7, 11, 15, 20, 23])
@pytest.mark.parametrize('kind', ['unmoved', 'jittered'])
def test_forward_matches_restatement(n, kind):
    x, m = _coords(n, kind, seed=n)
    _check_forward(x, m, _params(2, n))


def _check_forward(x, m, p):
    """1e-5 against fp64, or the fp32 reference's own distance from fp64 times 1.5 where that is larger: on unmoved meshes
    Simpson and lattice points lie on element edges, and which triangles the reference's inclusive test counts there depends
    on the precision (fp32 vs fp64 differ by ~3e-4 in coeffs at 11 x 11)."""
    _, coeffs, sol = _gpu([x], [m], [p])
    c, s = coeffs.detach().cpu().double().view(-1), sol.detach().cpu().double()
    _, c64, s64 = _ref(x, m, p, torch.float64)
    _, c32, s32 = _ref(x, m, p, torch.float32)
    c32, s32 = c32.detach().double(), s32.detach().double()
    assert _rel(c, c64.detach()) <= max(1e-5, 1.5 * _rel(c32, c64.detach())), (_rel(c, c64.detach()), _rel(c32, c64.detach()))
    assert _rel(s, s64.detach()) <= max(1e-5, 1.5 * _rel(s32, s64.detach())), (_rel(s, s64.detach()), _rel(s32, s64.detach()))


@pytest.mark.one_dispatch
def test_forward_folded_mesh():
    x, m = _coords(11, 'folded')
    _check_forward(x, m, _params(3, 5))


@pytest.mark.one_dispatch
def test_forward_mixed_batch_one_call():
    sizes, gauss = [12, 23, 17, 14], [1, 6, 3, 2]
    xs, ms = zip(*[_coords(n, 'jittered', seed=n) for n in sizes])
    ps = [_params(k, 40 + k) for k in gauss]
    _, coeffs, sol = _gpu(list(xs), list(ms), ps)
    off = 0
    for b, (x, m, p) in enumerate(zip(xs, ms, ps)):
        _, c64, s64 = _ref(x, m, p, torch.float64)
        _, c32, s32 = _ref(x, m, p, torch.float32)
        c, s = coeffs[off:off + m.num_nodes].detach().cpu().double().view(-1), sol[b * 101 * 101:(b + 1) * 101 * 101].detach().cpu().double()
        assert _rel(c, c64.detach()) <= max(1e-5, 1.5 * _rel(c32.detach().double(), c64.detach())), b
        assert _rel(s, s64.detach()) <= max(1e-5, 1.5 * _rel(s32.detach().double(), s64.detach())), b
        off += m.num_nodes


def _grad_case(x, m, p, seed):
    g = torch.Generator().manual_seed(seed)
    w_sol = torch.randn(101 * 101, generator=g)
    w_c = torch.randn(m.num_nodes, generator=g)
    xg, coeffs, sol = _gpu([x], [m], [p])
    ((sol * w_sol.to(DEV)).sum() + (coeffs.view(-1) * w_c.to(DEV)).sum()).backward()
    out = {}
    for dt in (torch.float32, torch.float64):
        xx, c, s = _ref(x, m, p, dt)
        ((s * w_sol.to(dt)).sum() + (c * w_c.to(dt)).sum()).backward()
        out[dt] = xx.grad.double()
    return xg.grad.cpu().double(), out[torch.float32], out[torch.float64]


@pytest.mark.one_dispatch
@pytest.mark.parametrize('n,kind', [(7, 'jittered'), (15, 'jittered'), (11, 'gnn_moved')])
def test_gradient_against_fp64(n, kind):
    if kind == 'gnn_moved':
        ds = MeshDataset([n, n], 1, seed=3)
        opt = hot_path_opt(mesh_dims=[n, n], hidden_dim=8, num_layers=4)
        torch.manual_seed(0)
        model = GNN(ds, opt)
        with torch.no_grad():
            for prm in model.parameters():
                prm.add_(0.3 * torch.randn_like(prm))
        o = dict(opt); o['device'] = str(DEV)
        gm = GNN(ds, o).to(DEV)
        gm.load_state_dict(model.state_dict())
        x = gm(collate(ds.samples).to(DEV)).detach().cpu()
        m = square_mesh(n)
    else:
        x, m = _coords(n, kind, seed=n + 1)
    g_hip, g32, g64 = _grad_case(x, m, _params(2, n), seed=n)
    noise = _rel(g32, g64)
    assert _rel(g_hip, g64) <= max(1e-4, 1.5 * noise), (_rel(g_hip, g64), noise)


@pytest.mark.one_dispatch
@pytest.mark.parametrize('n', [7, 15])
def test_gradient_unmoved_against_fp32(n):
    # Simpson points and lattice points on element edges: classified as the fp32 reference does (no FMA contraction,
    # torch.linspace's point formula)
    x, m = _coords(n, 'unmoved')
    g_hip, g32, g64 = _grad_case(x, m, _params(2, 2 * n), seed=n)
    assert _rel(g_hip, g32) <= 1e-4, (_rel(g_hip, g32), _rel(g32, g64))


@pytest.mark.one_dispatch
def test_torch_FEM_2D_signature():
    x, m = _coords(11, 'jittered', seed=2)
    p = _params(2, 9)
    mesh = MeshTopology(m.cells.numpy())
    coeffs, pts, sol = torch_FEM_2D({'device': DEV}, mesh, x.to(DEV), QUAD, 11,
                                    [torch.from_numpy(c) for c in p['centers']], [torch.from_numpy(s) for s in p['scales']])
    assert coeffs.shape == (121, 1) and sol.shape == (101, 101)
    _, c64, s64 = _ref(x, m, p, torch.float64)
    _, c32, s32 = _ref(x, m, p, torch.float32)
    assert _rel(sol.detach().cpu().double().reshape(-1), s64.detach()) <= max(1e-5, 1.5 * _rel(s32.detach().double(), s64.detach()))


@pytest.mark.one_dispatch
def test_deterministic():
    sizes = [15, 20]
    xs, ms = zip(*[_coords(n, 'jittered', seed=n) for n in sizes])
    ps = [_params(3, 1), _params(2, 2)]
    runs = []
    for _ in range(2):
        x, coeffs, sol = _gpu(list(xs), list(ms), ps)
        (sol.square().sum() + coeffs.sum()).backward()
        runs.append((coeffs.detach().cpu(), sol.detach().cpu(), x.grad.cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.one_dispatch
def test_band_limit_raises():
    x, m = _coords(30, 'unmoved')
    with pytest.raises(NotImplementedError, match='LDS'):
        _gpu([x], [m], [_params(1, 0)])


def _pde_opt(n):
    return hot_path_opt(mesh_dims=[n, n], hidden_dim=8, num_layers=4, time_step=0.1, loss_type='pde_loss', loss_fn='l1')


def test_gnn_end_to_end_parameter_gradients():
    from oracle.pyg_restatement import OracleGNN
    n = 15
    ds = MeshDataset([n, n], 2, seed=7, pde_loss_fields=True)
    data = collate(ds.samples)
    opt = _pde_opt(n)
    torch.manual_seed(0)
    oracle_opt = dict(opt); oracle_opt['loss_type'] = 'mesh_loss'
    oracle = OracleGNN(ds, oracle_opt)
    with torch.no_grad():
        for prm in oracle.parameters():
            prm.add_(0.2 * torch.randn_like(prm))
    o = dict(opt); o['device'] = str(DEV)
    model = GNN(ds, o).to(DEV)
    model.load_state_dict(oracle.state_dict())
    dd = data.clone().to(DEV)
    coeffs, x_phys, sol = model(dd)
    assert coeffs.shape == (2 * n * n, 1) and sol.shape == (2 * 101 * 101,)
    l1_loss(sol.view(-1, 1), dd.u_true_fine_tensor.view(-1, 1)).backward()
    grads = {k: p.grad.detach().cpu().double() for k, p in model.named_parameters() if p.grad is not None}
    assert grads

    ref = {}
    for dt in (torch.float32, torch.float64):
        oracle.zero_grad()
        xo = oracle(data)
        sols = []
        for b in range(2):
            xb = xo[b * n * n:(b + 1) * n * n].to(dt)
            _, s = R.fem2d(xb, ds.base.cells, ds.base.boundary_nodes, data.pde_params[b]['centers'], data.pde_params[b]['scales'],
                           LAT.to(dt))
            sols.append(s)
        loss = (torch.cat(sols) - data.u_true_fine_tensor.to(dt)).abs().mean()
        loss.backward()
        ref[dt] = {k: p.grad.detach().double().clone() for k, p in oracle.named_parameters() if p.grad is not None}
    # scale floor: lin_key.bias has a zero gradient (it cancels in the softmax); its reference value is rounding noise
    floor = 1e-2 * max(r.abs().max().item() for r in ref[torch.float64].values())

    def rel(a, b):
        return ((a - b).abs().max() / max(b.abs().max().item(), floor)).item()
    for k, g in grads.items():
        noise = rel(ref[torch.float32][k], ref[torch.float64][k])
        assert rel(g, ref[torch.float64][k]) <= max(1e-4, 1.5 * noise), (k, rel(g, ref[torch.float64][k]), noise)


def test_training_lowers_the_loss():
    n = 15
    ds = MeshDataset([n, n], 8, seed=11, pde_loss_fields=True)
    opt = _pde_opt(n); opt['device'] = str(DEV)
    torch.manual_seed(1)
    model = GNN(ds, opt).to(DEV).train()
    optim = torch.optim.Adam(model.parameters(), lr=1e-2)
    dd = collate(ds.samples).to(DEV)
    losses = []
    for _ in range(20):
        optim.zero_grad()
        _, _, sol = model(dd)
        loss = l1_loss(sol.view(-1, 1), dd.u_true_fine_tensor.view(-1, 1))
        loss.backward()
        optim.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses
