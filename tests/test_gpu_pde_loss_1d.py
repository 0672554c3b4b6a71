"""The 1-D pde_loss tail on the GPU: the three launches (`fem_poisson_1d`, the loss launch, the adjoint solve: 'split') and the one
launch (`poisson_loss_1d`, gadapt_fem_poisson1d_loss: 'fused') against tests/fem1d_restatement.py in fp64, its fp32 run as the
noise: rel <= max(1e-5, 1.5 x noise) for coeffs, sol and the loss values, max(1e-4, 1.5 x noise) for the node gradient (the rules
of tests/test_gpu_fem1d.py).  Fused against split: coeffs, sol and the gradient bit for bit (the seed has the same bits); the two
loss values are summed in different orders and each meets the fp64 rule.  Then the GNN with opt['pde_loss_1d'].

Shapes: 3 nodes (one interior node), 4, 15, 64 and 65 (the workgroup grows from one wave to two), a mixed jittered batch
[3, 15, 65, 21], P in {2, 64, 65, 101}, 1 and 3 Gaussians per mesh, a mesh with a folded interval, 1017 nodes (the fused cap at
P = 101).  Where P is not 101 the points are linspace(0.013, 0.987, P): at 0 and 1 sol is the boundary value itself and
sol - u_true is rounding noise alone, which P = 2 would consist of."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fem1d_restatement as R  # noqa: E402

from g_adaptivity_amd import GNN, MeshDataset, collate, hot_path_opt, l1_loss, mse_loss  # noqa: E402
from g_adaptivity_amd import fem1d  # noqa: E402
from g_adaptivity_amd.evaluation import ERROR_COLUMNS, evaluate_model_fine  # noqa: E402
from g_adaptivity_amd.fem1d import fem_poisson_1d, last_flags, poisson_loss_1d  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]
DEV = 'cuda:0'
OPT = {'load_quad_points': 101, 'stiff_quad_points': 3, 'eval_quad_points': 101}
LOSSES = {'l1': l1_loss, 'mse': mse_loss}


def _rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _check(what, gpu, ref, floor):
    noise, err = _rel(ref[torch.float32], ref[torch.float64]), _rel(gpu, ref[torch.float64])
    print(f"{what}: gpu vs fp64 {err:.3e}, fp32 restatement vs fp64 {noise:.3e}")
    assert err <= max(floor, 1.5 * noise), (what, err, noise)


def _mesh(n, seed, folded=False):
    u = torch.linspace(0, 1, n)
    g = torch.Generator().manual_seed(seed)
    x = u + (torch.rand(n, generator=g) * 2 - 1) * 0.3 / (n - 1)
    x[0], x[-1] = 0.0, 1.0
    if folded:
        x = u.clone()
        x[7], x[8] = u[8].item(), u[7].item()
    return x


def _params(k, seed):
    rng = np.random.default_rng(seed)
    return {'centers': [rng.uniform(0.2, 0.8, 1).astype('f') for _ in range(k)], 'scales': [rng.uniform(0.1, 0.4, 1).astype('f') for _ in range(k)]}


def _cs(p, dtype):
    return ([torch.tensor(float(c[0]), dtype=dtype) for c in p['centers']], [torch.tensor(float(s[0]), dtype=dtype) for s in p['scales']])


def _points(P):
    return torch.linspace(0, 1, P) if P == 101 else torch.linspace(0.013, 0.987, P)


def _target(params, pts):
    """u_true at the points per mesh, computed in fp64 and stored as fp32 (what the datasets store): [B*P]."""
    return torch.cat([R.gauss(pts.double(), *_cs(p, torch.float64)) for p in params]).float()


# name -> (node counts, Gaussians per mesh, P, index of a folded mesh or None)
CASES = {
    'n3': ([3], [1], 101, None),
    'n4': ([4], [3], 2, None),
    'n15': ([15], [1], 64, None),
    'n64': ([64], [3], 65, None),
    'n65': ([65], [1], 101, None),
    'mixed': ([3, 15, 65, 21], [1, 3, 3, 1], 101, None),
    'mixed_p65': ([3, 15, 65, 21], [3, 1, 1, 3], 65, None),
    'folded': ([21, 15], [1, 3], 101, 1),
    'n1017': ([1017], [3], 101, None),
}
_cache = {}


def _case(name):
    """The inputs of a case and its restated results in fp32 and fp64, computed once and shared."""
    if name in _cache:
        return _cache[name]
    counts, gauss, P, fold = CASES[name]
    meshes = [_mesh(n, 10 * i + n, folded=(i == fold)) for i, n in enumerate(counts)]
    params = [_params(k, 100 * i + n) for i, (n, k) in enumerate(zip(counts, gauss))]
    pts = _points(P)
    target = _target(params, pts)
    B = len(counts)
    ref = {k: {} for k in ('coeffs', 'sol', 'l1', 'mse', 'gx_l1', 'gx_mse')}
    for dt in (torch.float32, torch.float64):
        cs, ss, g1, g2, l1, mse = [], [], [], [], 0.0, 0.0
        for b, (m, p) in enumerate(zip(meshes, params)):
            x = m.to(dt).clone().requires_grad_(True)
            c, s = R.poisson(x, *_cs(p, dt), OPT, pts.to(dt))
            d = s - target[b * P:(b + 1) * P].to(dt)
            a, q = d.abs().sum() / (B * P), (d * d).sum() / (B * P)
            g1.append(torch.autograd.grad(a, x, retain_graph=True)[0])
            g2.append(torch.autograd.grad(q, x)[0])
            cs.append(c.detach()); ss.append(s.detach())
            l1, mse = l1 + a.detach(), mse + q.detach()
        for k, v in zip(ref, (torch.cat(cs), torch.cat(ss), l1, mse, torch.cat(g1), torch.cat(g2))):
            ref[k][dt] = v
    _cache[name] = dict(counts=counts, meshes=meshes, params=params, pts=pts, target=target, ref=ref, B=B, P=P, fold=fold)
    return _cache[name]


def _split(c, kind):
    x = torch.cat(c['meshes']).to(DEV).requires_grad_(True)
    target = c['target'].to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        coeffs, sol = fem_poisson_1d(x, c['counts'], c['params'], OPT, points=c['pts'])
    flags = last_flags().clone()
    loss = LOSSES[kind](sol.view(-1, 1), target.view(-1, 1))
    loss.backward()
    return dict(loss=loss.detach(), coeffs=coeffs.detach(), sol=sol.detach().view(-1), gx=x.grad.clone(), flags=flags)


def _fused(c, kind, only=None):
    """The one launch on the case, or on its mesh `only` alone; `partials` included."""
    idx = range(c['B']) if only is None else [only]
    x = torch.cat([c['meshes'][b] for b in idx]).to(DEV).requires_grad_(True)
    target = torch.cat([c['target'][b * c['P']:(b + 1) * c['P']] for b in idx]).to(DEV)
    bt = fem1d._Batch([c['counts'][b] for b in idx], [c['params'][b] for b in idx], x.device)
    loss, coeffs, sol, partials = fem1d._poisson_loss_on(bt, x, target, OPT['load_quad_points'], OPT['stiff_quad_points'],
                                                         c['pts'].to(DEV), kind)
    flags = last_flags().clone()
    loss.backward()
    return dict(loss=loss.detach(), coeffs=coeffs, sol=sol, gx=x.grad.clone(), flags=flags, partials=partials)


@pytest.mark.parametrize('name', [n for n in CASES if n != 'n1017'])
def test_split_and_fused_against_fp64_and_each_other(name):
    c = _case(name)
    ref = c['ref']
    for kind in ('l1', 'mse'):
        s, f = _split(c, kind), _fused(c, kind)
        for tag, got in (('split', s), ('fused', f)):
            _check(f'{name} {kind} {tag} coeffs', got['coeffs'], ref['coeffs'], 1e-5)
            _check(f'{name} {kind} {tag} sol', got['sol'], ref['sol'], 1e-5)
            _check(f'{name} {kind} {tag} loss', got['loss'], ref[kind], 1e-5)
            _check(f'{name} {kind} {tag} gx', got['gx'], ref['gx_' + kind], 1e-4)
            assert got['flags'].tolist() == [1 if b == c['fold'] else 0 for b in range(c['B'])]
        for k in ('coeffs', 'sol', 'gx', 'flags'):
            assert torch.equal(f[k], s[k]), (name, kind, k)
        assert f['sol'].shape == (c['B'] * c['P'],) and f['loss'].shape == () and f['gx'].abs().max() > 0
        again = _fused(c, kind)                                                 # two runs give the same bits
        for k in ('loss', 'coeffs', 'sol', 'gx', 'partials'):
            assert torch.equal(again[k], f[k]), (name, kind, k)
        # the loss is the partials added in index order, times 1 / (B P)
        total = torch.zeros((), dtype=torch.float32)
        for v in f['partials'].cpu():
            total = total + v
        assert torch.equal(f['loss'].cpu(), total * (torch.ones((), dtype=torch.float32) / float(c['B'] * c['P'])))


def test_public_entry_is_the_fused_launch():
    c = _case('mixed')
    x = torch.cat(c['meshes']).to(DEV).requires_grad_(True)
    loss, coeffs, sol = poisson_loss_1d(x, c['counts'], c['params'], c['target'].to(DEV), OPT, loss='mse', points=c['pts'])
    assert not coeffs.requires_grad and not sol.requires_grad and loss.requires_grad
    (3.0 * loss).backward()
    f = _fused(c, 'mse')
    assert torch.equal(loss.detach(), f['loss']) and torch.equal(coeffs, f['coeffs']) and torch.equal(sol, f['sol'])
    assert torch.equal(x.grad, f['gx'] * 3.0)                                   # backward is g * gx
    with pytest.raises(ValueError, match="'l1', 'mse'"):
        poisson_loss_1d(x, c['counts'], c['params'], c['target'].to(DEV), OPT, loss='huber')
    with pytest.raises(ValueError, match='target of 7 values'):
        poisson_loss_1d(x, c['counts'], c['params'], torch.zeros(7, device=DEV), OPT)


@pytest.mark.parametrize('kind', ['l1', 'mse'])
def test_a_mesh_alone_is_the_mesh_in_the_mixed_batch(kind):
    """coeffs, sol, flags and the partial of a mesh do not depend on its batch (nor on the workgroup's size, which follows the
    largest mesh: 65 nodes, two waves).  The gradient depends on it through 1 / (B P) alone: B = 4, a power of two, so it is
    the batch's gradient times 4 exactly."""
    c = _case('mixed')
    assert c['B'] == 4
    batch = _fused(c, kind)
    off = np.concatenate([[0], np.cumsum(c['counts'])])
    for b in range(4):
        alone = _fused(c, kind, only=b)
        n0, n1, P = int(off[b]), int(off[b + 1]), c['P']
        assert torch.equal(alone['coeffs'], batch['coeffs'][n0:n1]) and torch.equal(alone['sol'], batch['sol'][b * P:(b + 1) * P])
        assert torch.equal(alone['partials'], batch['partials'][b:b + 1]) and torch.equal(alone['flags'], batch['flags'][b:b + 1])
        assert torch.equal(alone['gx'], batch['gx'][n0:n1] * 4.0)


def test_fused_at_its_node_cap():
    """1017 nodes at 101 points: the last size whose seed row fits beside the solve.  1018 is refused before any launch."""
    c = _case('n1017')
    for kind in ('l1', 'mse'):
        f = _fused(c, kind)
        _check(f'n1017 {kind} coeffs', f['coeffs'], c['ref']['coeffs'], 1e-5)
        _check(f'n1017 {kind} sol', f['sol'], c['ref']['sol'], 1e-5)
        _check(f'n1017 {kind} loss', f['loss'], c['ref'][kind], 1e-5)
        _check(f'n1017 {kind} gx', f['gx'], c['ref']['gx_' + kind], 1e-4)
        assert f['flags'].tolist() == [0]
    s = _split(c, 'l1')
    f = _fused(c, 'l1')
    for k in ('coeffs', 'sol', 'gx'):
        assert torch.equal(f[k], s[k]), k
    x = torch.linspace(0, 1, 1018).to(DEV)
    with pytest.raises(NotImplementedError, match='1018 nodes.*65556 B'):
        poisson_loss_1d(x, [1018], c['params'], c['target'].to(DEV), OPT)
    fem_poisson_1d(x, [1018], c['params'], OPT)                                 # the split tail takes it


# ------------------------------------------------------------------------------------------------ the GNN
N, BATCH = 15, 3


def _gnn_opt(**kw):
    return hot_path_opt(mesh_dims=[N], hidden_dim=8, num_layers=4, time_step=0.1, loss_type='pde_loss', loss_fn='l1', pde_loss_1d=True,
                        **kw)


@pytest.fixture(scope='module')
def gnn():
    """A 15-node pde_loss model, its mesh_loss twin with the same weights (the initial ones plus 0.05 randn), and the oracle."""
    from oracle.pyg_restatement import OracleGNN
    ds = MeshDataset([N], BATCH, seed=7, pde_loss_fields=True)
    opt = _gnn_opt()
    torch.manual_seed(0)
    oracle = OracleGNN(ds, dict(opt, loss_type='mesh_loss'))
    with torch.no_grad():
        for prm in oracle.parameters():
            prm.add_(0.05 * torch.randn_like(prm))
    model = GNN(ds, dict(opt, device=DEV)).to(DEV)
    twin = GNN(ds, dict(opt, device=DEV, loss_type='mesh_loss')).to(DEV)
    model.load_state_dict(oracle.state_dict())
    twin.load_state_dict(oracle.state_dict())
    return ds, oracle, model, twin


def test_gnn_forward_shapes_and_the_mesh_loss_twin(gnn):
    ds, _, model, twin = gnn
    data = collate(ds.samples).to(DEV)
    coeffs, x_phys, sol = model(data)
    assert coeffs.shape == (BATCH * (N - 2), 1) and x_phys.shape == (BATCH * N,) and sol.shape == (BATCH * 101,)
    out = twin(data)
    assert out.shape == (BATCH * N, 1) and torch.equal(x_phys, out.reshape(-1))   # the twin's [N,1], flattened: the same bits
    # what torch_FEM_1D gives per mesh: the interior coefficients
    full, sol2 = fem_poisson_1d(x_phys.detach(), [N] * BATCH, data.pde_params, model.opt)
    assert torch.equal(sol, sol2.view(-1)) and torch.equal(coeffs.view(BATCH, N - 2), full.view(BATCH, N)[:, 1:-1])
    flags = last_flags().clone()
    # a batch that carries its descriptor is solved through it
    data._pde_batch = fem1d.Pde1dBatch.from_data(model, data)
    c2, x2, s2 = model(data)
    assert torch.equal(c2, coeffs) and torch.equal(x2, x_phys) and torch.equal(s2, sol)
    assert last_flags().is_cuda and torch.equal(last_flags(), flags)            # the descriptor's flags stay on the device


def test_gnn_parameter_gradients(gnn):
    """Parameter gradients of l1_loss(sol, u_true_fine_tensor) within max(1e-4, 1.5 x noise) of the fp64 oracle with the restated
    tail (the pattern of tests/test_gpu_fem_wave_grad.py's model test)."""
    ds, oracle, model, _ = gnn
    data = collate(ds.samples)
    dd = data.clone().to(DEV)
    model.zero_grad()
    _, _, sol = model(dd)
    l1_loss(sol.view(-1, 1), dd.u_true_fine_tensor.view(-1, 1)).backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    assert grads
    pts = torch.linspace(0, 1, 101)
    ref = {}
    for dt in (torch.float32, torch.float64):
        oracle.zero_grad()
        xo = oracle(data)
        sols = []
        for b in range(BATCH):
            xb = xo[b * N:(b + 1) * N].reshape(-1).to(dt)
            sols.append(R.poisson(xb, *_cs(data.pde_params[b], dt), OPT, pts.to(dt))[1])
        (torch.cat(sols) - data.u_true_fine_tensor.to(dt)).abs().mean().backward()
        ref[dt] = {k: p.grad.detach().double().clone() for k, p in oracle.named_parameters() if p.grad is not None}
    assert ref[torch.float64].keys() == grads.keys()
    # scale floor: lin_key.bias has a zero gradient (it cancels in the softmax); its reference value is rounding noise
    floor = 1e-2 * max(r.abs().max().item() for r in ref[torch.float64].values())

    def rel(a, b):
        return ((a - b).abs().max() / max(b.abs().max().item(), floor)).item()
    for k, g in grads.items():
        noise = rel(ref[torch.float32][k], ref[torch.float64][k])
        err = rel(g.cpu().double(), ref[torch.float64][k])
        print(f"{k}: gpu vs fp64 {err:.3e}, fp32 restatement vs fp64 {noise:.3e}")
        assert err <= max(1e-4, 1.5 * noise), (k, err, noise)


def test_evaluate_model_fine_gives_the_rows_of_the_twin(gnn):
    ds, _, model, twin = gnn
    rows = evaluate_model_fine(model, ds, dict(model.opt), batch_size=BATCH)[0]
    want = evaluate_model_fine(twin, ds, dict(twin.opt), batch_size=BATCH)[0]
    for k in ERROR_COLUMNS:
        assert np.array_equal(np.asarray(rows[k], dtype=float), np.asarray(want[k], dtype=float)), k
    assert len(rows['L1_MLmodel']) == BATCH
