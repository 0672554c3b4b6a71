"""loss_type='modular' in 2-D on the MI355X: gradient_meshpoints_2D (g_adaptivity_amd/fem.py, libgadapt_fem.so) against the
test-side restatement of the reference's three gradient types (tests/modular2d_restatement.py), and the model trained
through its pseudo-loss.

The gradient rule here, rel <= max(1e-4, 1.5 x the fp32 restatement's own deviation), is taken over ALL nodes, and there it is
loose: the fp32 restatement itself is 1e-3 to 3e-2 from fp64 on jittered meshes, from the boundary nodes, whose Simpson points
lie on element edges that fp32 and fp64 class differently.  tests/fem_lattices.py and tests/test_gpu_fem_lattices.py hold
the same kernels to 1e-4 on the interior nodes, where that deviation stays under 6.6e-5 (5 x 5 and 7 x 7 meshes)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fem_restatement as R  # noqa: E402
import modular2d_restatement as M  # noqa: E402

from g_adaptivity_amd import GNN, MeshDataset, collate, gradient_meshpoints_2D, hot_path_opt  # noqa: E402
from g_adaptivity_amd import _native_fem  # noqa: E402
from g_adaptivity_amd.fem import modular_loss_2d  # noqa: E402
from g_adaptivity_amd.mesh_graph import MeshData, square_mesh  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TYPES = ['PDE_loss_direct_mse', 'PDE_loss_direct_L2', 'PDE_loss_adjoint_L2']
LOSS_FLOOR = 2e-4          # see test_against_fp64


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
    elif kind == 'gnn_moved':
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
    return x, m


def _opt(gt, n, **kw):
    return dict(grad_type=gt, mesh_dims=[n, n], eval_quad_points=101, load_quad_points=101, **kw)


def _gpu(gt, x, m, p, **kw):
    data = MeshData(cells=m.cells, boundary_nodes=m.boundary_nodes, pde_params=[p])
    loss, g = gradient_meshpoints_2D(_opt(gt, int(round(m.num_nodes ** 0.5)), **kw), data, x.to(DEV))
    return loss.cpu().double(), g.cpu().double()


def _ref(gt, x, m, p, dtype):
    args = (x.to(dtype), m.cells, m.boundary_nodes, p['centers'], p['scales'])
    if gt == 'PDE_loss_direct_mse':
        loss, g = M.direct('mse', *args, R.SIMPSON_N, 101)
    elif gt == 'PDE_loss_direct_L2':
        loss, g = M.direct('L2', *args, R.SIMPSON_N, R.SIMPSON_N)
    else:
        loss, g = M.adjoint_L2(*args, R.SIMPSON_N, R.SIMPSON_N)
    return loss.double(), g.double()


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.one_dispatch
@pytest.mark.parametrize('gt', TYPES)
@pytest.mark.parametrize('n,kind', [(7, 'jittered'), (11, 'jittered'), (15, 'jittered'), (23, 'jittered'),
                                    (11, 'gnn_moved'), (23, 'gnn_moved')])
def test_against_fp64(gt, n, kind):
    """x_grads: 1e-4 against fp64, or 1.5 x the fp32 restatement's own distance from fp64 where larger (the pde_loss
    rule).  The loss gets a 2e-4 floor: it is quadratic in e = sol - u_true, which cancels to ~1e-3 of sol on the finer
    meshes, so an fp32 solve's rounding (~1e-7 of sol; banded Cholesky here, LU in the restatement) moves it by ~1e-4
    relative, and which of two fp32 solves lands nearer fp64 is chance (measured at 23 x 23: 1.2e-4 here, 4e-5 there)."""
    x, m = _coords(n, kind, seed=n + 1)
    p = _params(2, n)
    loss, g = _gpu(gt, x, m, p)
    l64, g64 = _ref(gt, x, m, p, torch.float64)
    l32, g32 = _ref(gt, x, m, p, torch.float32)
    assert g.shape == (n * n, 2)
    assert _rel(loss, l64) <= max(LOSS_FLOOR, 1.5 * _rel(l32, l64)), (_rel(loss, l64), _rel(l32, l64))
    assert _rel(g, g64) <= max(1e-4, 1.5 * _rel(g32, g64)), (_rel(g, g64), _rel(g32, g64))


@pytest.mark.one_dispatch
@pytest.mark.parametrize('gt', TYPES)
@pytest.mark.parametrize('n', [7, 15])
def test_unmoved_against_fp32(gt, n):
    # lattice and Simpson points on element edges: classified as the fp32 reference does (a point counted in another
    # triangle moves the loss and x_grads by 1e-2 or more); the rest is the two fp32 solves' rounding, amplified in the
    # loss and its gradient by the cancellation in e = sol - u_true (see test_against_fp64)
    x, m = _coords(n, 'unmoved')
    p = _params(2, 2 * n)
    loss, g = _gpu(gt, x, m, p)
    l32, g32 = _ref(gt, x, m, p, torch.float32)
    assert _rel(loss, l32) <= LOSS_FLOOR and _rel(g, g32) <= LOSS_FLOOR, (_rel(loss, l32), _rel(g, g32))


def _batch(sizes, gauss, seed0=40):
    xs, ms = zip(*[_coords(n, 'jittered', seed=n) for n in sizes])
    ps = [_params(k, seed0 + k) for k in gauss]
    offs = np.cumsum([0] + [m.num_nodes for m in ms[:-1]])
    cells = torch.cat([m.cells + int(o) for m, o in zip(ms, offs)], 0)
    bnd = torch.cat([m.boundary_nodes for m in ms])
    batch = torch.repeat_interleave(torch.arange(len(ms)), torch.tensor([m.num_nodes for m in ms]))
    data = MeshData(cells=cells, boundary_nodes=bnd, pde_params=ps, batch=batch, _num_graphs=len(ms))
    return torch.cat(xs).to(DEV), data, xs, ms, ps


@pytest.mark.one_dispatch
@pytest.mark.parametrize('reduction,n_lat', [('mse', 101), ('simpson', 9)])
def test_mixed_batch_bit_identical_to_one_mesh_calls(reduction, n_lat):
    sizes, gauss = [12, 23, 17, 14], [1, 6, 3, 2]
    x, data, xs, ms, ps = _batch(sizes, gauss)
    counts = [m.num_nodes for m in ms]
    loss, g = modular_loss_2d(x, data.cells, data.boundary_nodes, counts, ps, n_lat, reduction, n_load=R.SIMPSON_N)
    off = 0
    for b, (xb, m, p) in enumerate(zip(xs, ms, ps)):
        lb, gb = modular_loss_2d(xb.to(DEV), m.cells, m.boundary_nodes, [m.num_nodes], [p], n_lat, reduction)
        assert torch.equal(loss[b:b + 1], lb), b
        assert torch.equal(g[off:off + m.num_nodes], gb), b
        off += m.num_nodes
    gt = 'PDE_loss_direct_mse' if reduction == 'mse' else 'PDE_loss_direct_L2'
    mean, g2 = gradient_meshpoints_2D(_opt(gt, 12), data, x)
    assert mean.dim() == 0 and mean.device == x.device
    assert torch.equal(mean, loss.mean()) and torch.equal(g2, g)


@pytest.mark.one_dispatch
@pytest.mark.parametrize('gt', TYPES)
def test_deterministic(gt):
    x, data, *_ = _batch([15, 20], [3, 2], seed0=1)
    runs = [gradient_meshpoints_2D(_opt(gt, 15), data, x) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.one_dispatch
def test_adjoint_quad_counts():
    x, m = _coords(11, 'jittered', seed=5)
    p = _params(2, 6)
    data = MeshData(cells=m.cells, boundary_nodes=m.boundary_nodes, pde_params=[p])
    xd = x.to(DEV)
    la, ga = gradient_meshpoints_2D(_opt('PDE_loss_adjoint_L2', 11), data, xd)
    ld, gd = gradient_meshpoints_2D(_opt('PDE_loss_direct_L2', 11), data, xd)
    assert torch.equal(la, ld) and torch.equal(ga, gd)
    # load_quad_points 101, eval_quad_points 51: the adjoint type reads load_quad_points only (9 x 9 both)
    o = _opt('PDE_loss_adjoint_L2', 11); o['eval_quad_points'] = 51
    loss, g = gradient_meshpoints_2D(o, data, xd)
    l64, g64 = _ref('PDE_loss_adjoint_L2', x, m, p, torch.float64)
    l32, g32 = _ref('PDE_loss_adjoint_L2', x, m, p, torch.float32)
    assert _rel(loss.cpu().double(), l64) <= max(1e-5, 1.5 * _rel(l32, l64))
    assert _rel(g.cpu().double(), g64) <= max(1e-4, 1.5 * _rel(g32, g64))
    # direct_L2 with eval_quad_points 51 needs a 7-point load vector: not built
    o = _opt('PDE_loss_direct_L2', 11); o['eval_quad_points'] = 51
    with pytest.raises(NotImplementedError, match='7'):
        gradient_meshpoints_2D(o, data, xd)


def _modular_opt(n):
    return hot_path_opt(mesh_dims=[n, n], hidden_dim=8, num_layers=4, time_step=0.1, loss_type='modular',
                        grad_type='PDE_loss_direct_mse', load_quad_points=101, device=str(DEV))


def test_reference_signature_batch_one():
    ds = MeshDataset([11, 11], 1)
    opt = _modular_opt(11)
    torch.manual_seed(0)
    model = GNN(ds, opt).to(DEV).train()
    data = collate(ds.samples).to(DEV)
    x_phys = model(data)
    loss, x_grads = gradient_meshpoints_2D(opt, data, x_phys.detach())
    assert x_grads.shape == x_phys.shape and loss.dim() == 0 and torch.isfinite(loss)
    names, prms = zip(*[(k, p) for k, p in model.named_parameters() if p.requires_grad])
    # the parameters the forward uses (this config leaves some, e.g. lin_skip, out of the graph)
    used = [g is not None for g in torch.autograd.grad(x_phys.sum(), prms, retain_graph=True, allow_unused=True)]
    assert sum(used) > 0
    (x_phys * x_grads).sum().backward()
    for k, prm, u in zip(names, prms, used):
        if not u:
            continue
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), k
        if not k.endswith('lin_key.bias'):       # it cancels in the softmax: its gradient is zero up to rounding
            assert prm.grad.abs().max().item() > 0, k


def test_training_lowers_the_loss():
    n = 15
    ds = MeshDataset([n, n], 8, seed=11)
    opt = _modular_opt(n)
    torch.manual_seed(1)
    model = GNN(ds, opt).to(DEV).train()
    optim = torch.optim.Adam(model.parameters(), lr=1e-2)
    dd = collate(ds.samples).to(DEV)
    losses = []
    for _ in range(20):
        optim.zero_grad()
        x_phys = model(dd)
        loss, x_grads = gradient_meshpoints_2D(opt, dd, x_phys.detach())
        (x_phys * x_grads).sum().backward()
        optim.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses


@pytest.mark.one_dispatch
def test_limits():
    x, m = _coords(30, 'unmoved')
    data = MeshData(cells=m.cells, boundary_nodes=m.boundary_nodes, pde_params=[_params(1, 0)])
    with pytest.raises(NotImplementedError, match='LDS'):
        gradient_meshpoints_2D(_opt('PDE_loss_direct_mse', 30), data, x.to(DEV))
    lib = _native_fem.lib()
    args = [1, 4, 2] + [None] * 12 + [2, 1024, 2, _native_fem.LOSS_MSE] + [None] * 7
    assert lib.gadapt_fem_modular_forward(*args) == -1                 # GADAPT_FEM_E_BADARG: nothing launched
    assert b'null' in lib.gadapt_fem_last_error()
