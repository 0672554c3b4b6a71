"""The 1-D FEM tails (g_adaptivity_amd.fem1d) at the sizes where their launch shape changes: whole waves (63/64/65 ... 1023/1024
nodes), the smallest meshes, the LDS budget (1024 nodes, and 1024 coarse + 465 fine), a fine mesh longer than the coarse one,
several Gaussians per mesh, the smallest quadrature and point counts, more points than lanes, and the backward's serial
spill pass on a folded mesh.

The rule and the floors are those of test_gpu_fem1d.py: rel(gpu, fp64) <= max(floor, 1.5 rel(fp32, fp64)), both runs from
fem1d_restatement.py, floor 1e-5 for coefficients, sol, fine_sol and error norms, 1e-4 for gradients.  The restatement is
the dense one up to 257 nodes; above that Burgers uses the banded mass assembly (pinned to the dense one in
test_fem1d_host.py) and Poisson stays dense.  Every case prints its err and noise (docs/measurements.md has the table).
"""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_restatement as E  # noqa: E402
import fem1d_restatement as R  # noqa: E402

from g_adaptivity_amd import poisson_eval_errors  # noqa: E402
from g_adaptivity_amd.fem1d import (burgers_1d, fem_poisson_1d, get_Burgers_initial_coeffs, gradient_meshpoints_1D,  # noqa: E402
                                    last_flags, torch_FEM_Burgers_1D)
from g_adaptivity_amd.mesh_graph import MeshData  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
BASE = {'gauss_amplitude': 0.25, 'tau': 1 / 20.0, 'nu': 0.001, 'stiff_quad_points': 3, 'num_fine_mesh_points': 40,
        'num_time_steps': 1}
DENSE_MAX = 257                       # the dense Burgers restatement up to here, the banded one above


def _opt(k, **kw):
    return dict(BASE, load_quad_points=k, eval_quad_points=k, **kw)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _check(label, gpu, f32, f64, floor):
    noise, err = _rel(f32, f64), _rel(gpu, f64)
    print(f"fem1d {label}: err {err:.3e} noise {noise:.3e}")
    assert bool(torch.isfinite(f64).all()) and bool(torch.isfinite(gpu).all()), label
    assert err <= max(floor, 1.5 * noise), (label, err, noise)


def _mesh(n, kind, seed=None):
    """linspace(0, 1, n), or that with every interior node moved by up to 0.3 of a cell (fp32 values, as _meshes() does)."""
    u = torch.linspace(0, 1, n)
    if kind == 'jittered':
        g = torch.Generator().manual_seed(n if seed is None else seed)
        u = u + (torch.rand(n, generator=g) * 2 - 1) * 0.3 / (n - 1)
        u[0], u[-1] = 0.0, 1.0
    return u


def _params(seed, counts):
    """One dict per mesh with counts[b] Gaussians: centres in 0.3..0.7, scales in 0.05..0.2."""
    rng = np.random.default_rng(seed)
    return [{'centers': [rng.uniform(0.3, 0.7, 1).astype('f') for _ in range(g)],
             'scales': [rng.uniform(0.05, 0.2, 1).astype('f') for _ in range(g)]} for g in counts]


def _cs(p, dtype):
    return ([torch.tensor(float(c[0]), dtype=dtype) for c in p['centers']],
            [torch.tensor(float(s[0]), dtype=dtype) for s in p['scales']])


def _burgers_ref(x, p, opt, T, pts, dtype, banded=None):
    """(c, sol, fine_sol, d sum(sol^2) / d x) of the restatement on one mesh."""
    banded = x.numel() > DENSE_MAX if banded is None else banded
    c, s = _cs(p, dtype)
    xx = x.to(dtype).clone().requires_grad_(True)
    u, sol, fine = R.burgers(xx, c, s, opt, T, pts.to(dtype), banded=banded)
    (sol ** 2).sum().backward()
    return u.detach(), sol.detach(), fine, xx.grad


def _burgers_gpu(xs, params, opt, T, pts):
    x = torch.cat(xs).to(DEV).requires_grad_(True)
    c, sol, fine = burgers_1d(x, [m.numel() for m in xs], params, opt, T, points=pts)
    (sol ** 2).sum().backward()
    return c.detach(), sol.detach(), fine, x.grad


def _weight(B, P):
    return torch.randn(B, P, generator=torch.Generator().manual_seed(0))


def _poisson_ref(x, p, opt, pts, w, dtype):
    """(c, sol, d sum(sol * w) / d x) of the restatement on one mesh."""
    c, s = _cs(p, dtype)
    xx = x.to(dtype).clone().requires_grad_(True)
    co, so = R.poisson(xx, c, s, opt, pts.to(dtype))
    (so * w.to(dtype)).sum().backward()
    return co.detach(), so.detach(), xx.grad


def _poisson_gpu(xs, params, opt, pts, w):
    x = torch.cat(xs).to(DEV).requires_grad_(True)
    c, sol = fem_poisson_1d(x, [m.numel() for m in xs], params, opt, points=pts)
    (sol * w.to(DEV)).sum().backward()
    return c.detach(), sol.detach(), x.grad


def _check_norms(label, x, p, opt, n_eval):
    l1, l2 = poisson_eval_errors(x.to(DEV), [x.numel()], [p], n_eval, opt=opt)
    e64 = E.errors_1d(x, p['centers'], p['scales'], opt, n_eval, F64)
    e32 = E.errors_1d(x, p['centers'], p['scales'], opt, n_eval, F32)
    for name, g, r64, r32 in zip(('L1', 'L2'), (l1.item(), l2.item()), e64, e32):
        err, noise = E.rel(g, r64), E.rel(r32, r64)
        print(f"fem1d {label} {name}: err {err:.3e} noise {noise:.3e}")
        assert np.isfinite(g) and np.isfinite(r64), (label, name)
        assert err <= max(1e-5, 1.5 * noise), (label, name, err, noise)


KINDS = ('uniform', 'jittered')
BURGERS_SIZES = [(n, 21) for n in (2, 3, 4, 63, 64, 65, 127, 128, 129)] + [(n, 11) for n in (255, 256, 257)] + \
                [(n, 5) for n in (1023, 1024)]
POISSON_SIZES = (3, 4, 63, 64, 65, 128, 129, 256, 257, 1023, 1024)


# ------------------------------------------------------------------------------------------------------ node counts
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,k', BURGERS_SIZES)
def test_burgers_node_counts(n, k, kind):
    """One mesh per launch, T = 2: u^T, sol, fine_sol (40 fine nodes) and the x gradient of sum(sol^2)."""
    x, p, opt = _mesh(n, kind), _params(n, [1])[0], _opt(k)
    pts = torch.linspace(0, 1, k)
    gpu = _burgers_gpu([x], [p], opt, 2, pts)
    assert last_flags().cpu().tolist() == [0]
    r32, r64 = _burgers_ref(x, p, opt, 2, pts, F32), _burgers_ref(x, p, opt, 2, pts, F64)
    for i, (name, floor) in enumerate((('c', 1e-5), ('sol', 1e-5), ('fine_sol', 1e-5), ('x.grad', 1e-4))):
        _check(f"burgers n={n} k={k} {kind} {name}", gpu[i].view(-1), r32[i].view(-1), r64[i].view(-1), floor)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', POISSON_SIZES)
def test_poisson_node_counts(n, kind):
    """Coefficients, sol, the x gradient under a fixed random weight, and the error norms of the evaluation's entry point."""
    x, p, opt = _mesh(n, kind), _params(n, [1])[0], _opt(11)
    pts, w = torch.linspace(0, 1, 11), _weight(1, 11)
    gpu = _poisson_gpu([x], [p], opt, pts, w)
    assert last_flags().cpu().tolist() == [0]
    r32, r64 = _poisson_ref(x, p, opt, pts, w[0], F32), _poisson_ref(x, p, opt, pts, w[0], F64)
    for i, (name, floor) in enumerate((('c', 1e-5), ('sol', 1e-5), ('x.grad', 1e-4))):
        _check(f"poisson n={n} k=11 {kind} {name}", gpu[i].view(-1), r32[i].view(-1), r64[i].view(-1), floor)
    _check_norms(f"poisson n={n} k=11 {kind} norm", x, p, opt, 11)


# ------------------------------------------------------------------------------------------------- one mixed launch
MIXED = [3, 64, 65, 1024, 21]
MIXED_GAUSS = [2, 1, 3, 2, 3]


def _mixed():
    return [_mesh(n, 'jittered', seed=100 + n) for n in MIXED], _params(23, MIXED_GAUSS)


def test_burgers_mixed_launch_within_the_rule_and_bitwise_equal_to_solo():
    xs, params = _mixed()
    opt, pts = _opt(5), torch.linspace(0, 1, 5)
    c, sol, fine, g = _burgers_gpu(xs, params, opt, 2, pts)
    assert last_flags().cpu().tolist() == [0] * len(xs)
    off = 0
    for b, (x, p) in enumerate(zip(xs, params)):
        n = x.numel()
        mine = (c[off:off + n], sol[b], fine[b], g[off:off + n])
        r32, r64 = _burgers_ref(x, p, opt, 2, pts, F32), _burgers_ref(x, p, opt, 2, pts, F64)
        for i, (name, floor) in enumerate((('c', 1e-5), ('sol', 1e-5), ('fine_sol', 1e-5), ('x.grad', 1e-4))):
            _check(f"burgers mixed n={n} gauss={MIXED_GAUSS[b]} {name}", mine[i], r32[i], r64[i], floor)
        alone = _burgers_gpu([x], [p], opt, 2, pts)
        for name, a, m in zip(('c', 'sol', 'fine_sol', 'x.grad'), alone, mine):
            assert torch.equal(a.view(-1), m.view(-1)), (n, name)
        off += n


def test_poisson_mixed_launch_within_the_rule_and_bitwise_equal_to_solo():
    xs, params = _mixed()
    opt, pts, w = _opt(11), torch.linspace(0, 1, 11), _weight(len(MIXED), 11)
    c, sol, g = _poisson_gpu(xs, params, opt, pts, w)
    l1, l2 = poisson_eval_errors(torch.cat(xs).to(DEV), MIXED, params, 11, opt=opt)
    off = 0
    for b, (x, p) in enumerate(zip(xs, params)):
        n = x.numel()
        mine = (c[off:off + n], sol[b], g[off:off + n])
        r32, r64 = _poisson_ref(x, p, opt, pts, w[b], F32), _poisson_ref(x, p, opt, pts, w[b], F64)
        for i, (name, floor) in enumerate((('c', 1e-5), ('sol', 1e-5), ('x.grad', 1e-4))):
            _check(f"poisson mixed n={n} gauss={MIXED_GAUSS[b]} {name}", mine[i], r32[i], r64[i], floor)
        _check_norms(f"poisson mixed n={n} gauss={MIXED_GAUSS[b]} norm", x, p, opt, 11)
        alone = _poisson_gpu([x], [p], opt, pts, w[b:b + 1])
        for name, a, m in zip(('c', 'sol', 'x.grad'), alone, mine):
            assert torch.equal(a.view(-1), m.view(-1)), (n, name)
        a1, a2 = poisson_eval_errors(x.to(DEV), [n], [p], 11, opt=opt)
        assert torch.equal(a1, l1[b:b + 1]) and torch.equal(a2, l2[b:b + 1]), n
        off += n


# ------------------------------------------------------------------------------------- fine mesh and the LDS budget
@pytest.mark.parametrize('n_fine', [64, 65, 129])
@pytest.mark.parametrize('n', [11, 21])
def test_fine_mesh_longer_than_the_coarse_one(n, n_fine):
    """The workgroup is sized by the fine mesh; most lanes idle in the coarse pass."""
    x, p, opt = _mesh(n, 'jittered'), _params(n + n_fine, [2])[0], _opt(21, num_fine_mesh_points=n_fine)
    pts = torch.linspace(0, 1, 21)
    gpu = _burgers_gpu([x], [p], opt, 2, pts)
    r32, r64 = _burgers_ref(x, p, opt, 2, pts, F32), _burgers_ref(x, p, opt, 2, pts, F64)
    for i, (name, floor) in enumerate((('c', 1e-5), ('sol', 1e-5), ('fine_sol', 1e-5), ('x.grad', 1e-4))):
        _check(f"fine n={n} n_fine={n_fine} {name}", gpu[i].view(-1), r32[i].view(-1), r64[i].view(-1), floor)


def test_lds_edge_1024_coarse_with_465_fine_runs_and_466_is_refused():
    """11 (1024 + 465) floats = 65 516 B fits the 65 536 B budget, 11 (1024 + 466) floats = 65 560 B does not."""
    x, p = _mesh(1024, 'jittered', seed=7), _params(465, [1])[0]
    pts = torch.linspace(0, 1, 5)
    opt = _opt(5, num_fine_mesh_points=465)
    gpu = _burgers_gpu([x], [p], opt, 2, pts)
    r32, r64 = _burgers_ref(x, p, opt, 2, pts, F32), _burgers_ref(x, p, opt, 2, pts, F64)
    for i, (name, floor) in enumerate((('c', 1e-5), ('sol', 1e-5), ('fine_sol', 1e-5), ('x.grad', 1e-4))):
        _check(f"lds-edge n=1024 n_fine=465 {name}", gpu[i].view(-1), r32[i].view(-1), r64[i].view(-1), floor)
    with pytest.raises(NotImplementedError, match='LDS'):
        burgers_1d(x.to(DEV), [1024], [p], _opt(5, num_fine_mesh_points=466), 2, points=pts)


# ---------------------------------------------------------------------------------- quadrature and point counts
@pytest.mark.parametrize('P', [1, 2, 64, 65, 1025])
@pytest.mark.parametrize('n', [21, 65])
def test_quadrature_and_point_counts(n, P):
    """load_quad_points 2 and 3, stiff_quad_points 1 and 3 (Burgers always takes 3, as the reference does), P points between
    the nodes.  The projection keeps eval_quad_points = 21."""
    x, p = _mesh(n, 'jittered', seed=n + P), _params(n + P, [2])[0]
    pts, w = torch.linspace(0.013, 0.987, P), _weight(1, P)
    for kl in (2, 3):
        opt = dict(_opt(21), load_quad_points=kl)
        gpu = _burgers_gpu([x], [p], opt, 2, pts)
        r32, r64 = _burgers_ref(x, p, opt, 2, pts, F32), _burgers_ref(x, p, opt, 2, pts, F64)
        _check(f"counts burgers n={n} P={P} load={kl} sol", gpu[1].view(-1), r32[1], r64[1], 1e-5)
        _check(f"counts burgers n={n} P={P} load={kl} x.grad", gpu[3], r32[3], r64[3], 1e-4)
        for ks in (1, 3):
            opt = dict(_opt(21), load_quad_points=kl, stiff_quad_points=ks)
            gpu = _poisson_gpu([x], [p], opt, pts, w)
            r32, r64 = _poisson_ref(x, p, opt, pts, w[0], F32), _poisson_ref(x, p, opt, pts, w[0], F64)
            _check(f"counts poisson n={n} P={P} load={kl} stiff={ks} sol", gpu[1].view(-1), r32[1], r64[1], 1e-5)
            _check(f"counts poisson n={n} P={P} load={kl} stiff={ks} x.grad", gpu[2], r32[2], r64[2], 1e-4)
            if P >= 2:
                _check_norms(f"counts poisson n={n} P={P} load={kl} stiff={ks} norm", x, p, opt, P)
            else:
                with pytest.raises(ValueError, match='at least 2'):
                    poisson_eval_errors(x.to(DEV), [n], [p], P, opt=opt)


# ------------------------------------------------------------------------------------------------ several Gaussians
GAUSS = [1, 2, 3]


def test_several_gaussians_projection_burgers_poisson():
    xs = [_mesh(21, 'jittered', seed=40 + g) for g in GAUSS]
    params = _params(29, GAUSS)
    opt, pts, w = _opt(21), torch.linspace(0, 1, 21), _weight(3, 21)
    bg = _burgers_gpu(xs, params, opt, 2, pts)
    pg = _poisson_gpu(xs, params, opt, pts, w)
    for b, (x, p, g) in enumerate(zip(xs, params, GAUSS)):
        sl = slice(21 * b, 21 * (b + 1))
        u0, u0f = get_Burgers_initial_coeffs(torch.linspace(0, 1, 40, device=DEV), 40, x.to(DEV), 21, p, 21, opt)
        ref = {dt: (R.project(x.to(dt), *_cs(p, dt), 0.25, 21, 21), R.project(torch.linspace(0, 1, 40, dtype=dt), *_cs(p, dt), 0.25, 210, 21))
               for dt in (F32, F64)}
        _check(f"gauss={g} projection", u0, ref[F32][0], ref[F64][0], 1e-5)
        _check(f"gauss={g} fine projection", u0f, ref[F32][1], ref[F64][1], 1e-5)
        mine = (bg[0][sl], bg[1][b], bg[2][b], bg[3][sl])
        r32, r64 = _burgers_ref(x, p, opt, 2, pts, F32), _burgers_ref(x, p, opt, 2, pts, F64)
        for i, (name, floor) in enumerate((('c', 1e-5), ('sol', 1e-5), ('fine_sol', 1e-5), ('x.grad', 1e-4))):
            _check(f"gauss={g} burgers {name}", mine[i], r32[i], r64[i], floor)
        mine = (pg[0][sl], pg[1][b], pg[2][sl])
        r32, r64 = _poisson_ref(x, p, opt, pts, w[b], F32), _poisson_ref(x, p, opt, pts, w[b], F64)
        for i, (name, floor) in enumerate((('c', 1e-5), ('sol', 1e-5), ('x.grad', 1e-4))):
            _check(f"gauss={g} poisson {name}", mine[i], r32[i], r64[i], floor)


@pytest.mark.parametrize('gt', ['burgers_timestep_loss_direct_mse', 'PDE_loss_direct_mse', 'PDE_loss_direct_L2'])
def test_several_gaussians_modular_loss(gt):
    xs = [_mesh(21, 'jittered', seed=50 + g) for g in GAUSS]
    params = _params(31, GAUSS)
    opt = dict(_opt(21), grad_type=gt, mesh_dims=[21], num_time_steps=2)
    data = MeshData(pde_params=params, _num_graphs=3)
    loss, gx = gradient_meshpoints_1D(opt, data, torch.cat(xs).to(DEV))
    ref = {}
    for dt in (F32, F64):
        ls, gs = [], []
        for x, p in zip(xs, params):
            xx = x.to(dt).clone().requires_grad_(True)
            l = R.modular_loss(xx, *_cs(p, dt), opt, torch.linspace(0, 1, 21, dtype=dt))
            l.backward()
            ls.append(l.detach()); gs.append(xx.grad)
        ref[dt] = (torch.stack(ls), gs)
    _check(f"gauss=1,2,3 {gt} loss", loss.view(1), ref[F32][0].mean().view(1), ref[F64][0].mean().view(1), 1e-5)
    for b, g in enumerate(GAUSS):
        _check(f"gauss={g} {gt} x.grad", gx[21 * b:21 * (b + 1)], ref[F32][1][b], ref[F64][1][b], 1e-4)


# ------------------------------------------------------------------------------- steps and explicit boundary values
@pytest.mark.parametrize('T', [1, 4])
@pytest.mark.parametrize('n', [65, 129])
def test_step_counts(n, T):
    x, p, opt = _mesh(n, 'jittered', seed=n + T), _params(n + T, [1])[0], _opt(21)
    pts = torch.linspace(0, 1, 21)
    gpu = _burgers_gpu([x], [p], opt, T, pts)
    r32, r64 = _burgers_ref(x, p, opt, T, pts, F32), _burgers_ref(x, p, opt, T, pts, F64)
    for i, (name, floor) in enumerate((('c', 1e-5), ('sol', 1e-5), ('fine_sol', 1e-5), ('x.grad', 1e-4))):
        _check(f"steps n={n} T={T} {name}", gpu[i].view(-1), r32[i].view(-1), r64[i].view(-1), floor)


@pytest.mark.parametrize('n', [65, 129])
def test_rollout_step_with_given_u0_and_boundary_values(n):
    """torch_FEM_Burgers_1D with u0, BC1 and BC2: u1, u0.grad and x.grad, as test_rollout_step_gradient_in_coefficients at 21."""
    m, p, opt = _mesh(n, 'jittered', seed=n + 9), _params(n + 9, [1])[0], _opt(21)
    b1, b2 = 0.0125, -0.0075
    ref = {}
    for dt in (F32, F64):
        u0 = R.project(m.to(dt), *_cs(p, dt), 0.25, 21, 21).clone().requires_grad_(True)
        xx = m.to(dt).clone().requires_grad_(True)
        u1, sol = R.burgers_step(xx, u0, opt['tau'], opt['nu'], 21, torch.linspace(0, 1, 21, dtype=dt), bc=torch.tensor([b1, b2], dtype=dt))
        (sol ** 2).sum().backward()
        ref[dt] = (u0.detach(), u1.detach(), u0.grad, xx.grad)
    u0 = ref[F32][0].to(DEV).requires_grad_(True)
    x = m.to(DEV).requires_grad_(True)
    u1, _, sol, o1, o2 = torch_FEM_Burgers_1D(opt, x, torch.linspace(0, 1, 21, device=DEV), n, u0, BC1=torch.tensor([b1]), BC2=torch.tensor([b2]))
    (sol ** 2).sum().backward()
    assert float(o1) == np.float32(b1) and float(o2) == np.float32(b2)
    for i, (name, got, floor) in enumerate((('u1', u1, 1e-5), ('u0.grad', u0.grad, 1e-4), ('x.grad', x.grad, 1e-4)), start=1):
        _check(f"rollout-bc n={n} {name}", got, ref[F32][i], ref[F64][i], floor)


# ------------------------------------------------------------------------------------------ folded mesh, backward
def _folded(n, i):
    x = torch.linspace(0, 1, n)
    x[i], x[i + 1] = x[i + 1].item(), x[i].item()
    return x


def _far_points(x, k):
    """Quadrature points of the load located outside their own interval's four neighbouring nodes i-1 .. i+2: what the
    backward cannot add from interval i's lane and leaves to the serial pass."""
    xq = R.quad_points(x, k)
    I = R.locate(x, xq.reshape(-1)).reshape(xq.shape)
    i = torch.arange(x.numel() - 1)[:, None]
    J = torch.clamp(I, max=x.numel() - 2)
    return ((I < i - 1) | (torch.clamp(I + 1, max=x.numel() - 1) > i + 2) | (J < i - 1) | (J + 1 > i + 2)).sum().item()


@pytest.mark.parametrize('n,i', [(21, 7), (65, 30)])
def test_folded_mesh_gradient_reaches_the_spill_pass(n, i):
    """Nodes i and i+1 swapped.  The kernel assembles the tridiagonal mass matrix whatever the mesh, and the banded restatement
    is that function, so the x gradient is compared with the banded restatement's autograd."""
    x, p, opt = _folded(n, i), _params(n, [1])[0], _opt(21)
    pts = torch.linspace(0, 1, 21)
    assert _far_points(x, 21) > 0 and _far_points(x.double(), 21) > 0
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        gpu = _burgers_gpu([x], [p], opt, 2, pts)
        assert last_flags().cpu().tolist() == [1]
    r32, r64 = _burgers_ref(x, p, opt, 2, pts, F32, banded=True), _burgers_ref(x, p, opt, 2, pts, F64, banded=True)
    _check(f"folded n={n} swap={i} sol", gpu[1].view(-1), r32[1], r64[1], 1e-5)
    _check(f"folded n={n} swap={i} x.grad", gpu[3], r32[3], r64[3], 1e-4)
