"""CPU checks of the 1-D FEM tails: the test-side restatement pinned from independent sides, and the API surface of
g_adaptivity_amd.fem1d that needs no GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fem1d_restatement as R  # noqa: E402

from g_adaptivity_amd import MeshDataset, gradient_meshpoints_1D  # noqa: E402
from g_adaptivity_amd import _native_fem  # noqa: E402
from g_adaptivity_amd._native import NativeError  # noqa: E402
from g_adaptivity_amd.fem1d import burgers_1d, fem_poisson_1d  # noqa: E402
from g_adaptivity_amd.mesh_graph import MeshData  # noqa: E402

C, S = [torch.tensor(0.45, dtype=torch.float64)], [torch.tensor(0.12, dtype=torch.float64)]
OPT = {'gauss_amplitude': 0.25, 'tau': 1 / 20.0, 'nu': 0.001, 'load_quad_points': 101, 'eval_quad_points': 101,
       'stiff_quad_points': 3, 'num_fine_mesh_points': 40, 'num_time_steps': 1, 'mesh_dims': [21]}


def _mesh(n, jitter=0.0, seed=0, dtype=torch.float64):
    x = torch.linspace(0, 1, n, dtype=dtype)
    if jitter:
        g = torch.Generator().manual_seed(seed)
        d = (torch.rand(n, generator=g, dtype=dtype) * 2 - 1) * jitter / (n - 1)
        d[0] = d[-1] = 0
        x = x + d
    return x


def test_mass_sums_to_one_and_stiffness_rows_to_zero():
    x = _mesh(15, jitter=0.3)
    M = R.mass_matrix(x, 101)
    assert abs(M.sum().item() - 1.0) < 1e-10
    A = R.stiffness_matrix(x, 3)
    assert A.sum(1).abs().max().item() < 1e-9


def test_constant_state_stays_constant():
    x = _mesh(21, jitter=0.3, seed=1)
    u = torch.full((21,), 0.7, dtype=torch.float64)
    u1, sol = R.burgers_step(x, u, OPT['tau'], OPT['nu'], 101, torch.linspace(0, 1, 11, dtype=torch.float64))
    assert (u1 - 0.7).abs().max().item() < 1e-12
    assert (sol - 0.7).abs().max().item() < 1e-12


def test_poisson_error_falls_as_h_squared():
    # (1-D P1 with an accurate load is exact at the nodes up to quadrature, so the error is measured between them)
    errs = []
    opt = dict(OPT, load_quad_points=401)
    pts = torch.linspace(0, 1, 1001, dtype=torch.float64)
    for n in (11, 21, 41):
        x = _mesh(n)
        _, sol = R.poisson(x, C, S, opt, pts)
        errs.append((sol - R.gauss(pts, C, S)).abs().max().item())
    rates = [np.log(errs[i] / errs[i + 1]) / np.log(2.0) for i in range(2)]
    assert all(r > 1.6 for r in rates), (errs, rates)


def _jittered(n, seed):
    """A jittered mesh on which no quadrature point changes interval within the finite-difference step: with 2^p + 1
    points per interval, a + (d*(k-1))/(k-1) = a + d, which is exactly b wherever b - a is exact (b/2 <= a)."""
    x = _mesh(n, jitter=0.3, seed=seed)
    assert all(x[i] == 0 or x[i] >= x[i + 1] / 2 for i in range(n - 1))
    return x


def test_gradcheck_burgers_fp64():
    x0 = _jittered(9, 6)
    pts = torch.linspace(0.013, 0.987, 13, dtype=torch.float64)
    u0 = R.project(x0, C, S, 0.25, 101, 33)

    def f(xi):
        x = torch.cat([x0[:1], xi, x0[-1:]])
        u = u0
        for _ in range(2):
            u, sol = R.burgers_step(x, u, 0.05, 0.001, 33, pts)
        return sol

    assert torch.autograd.gradcheck(f, (x0[1:-1].clone().requires_grad_(True),), eps=1e-7, atol=1e-5, rtol=1e-4)


def test_gradcheck_poisson_fp64():
    x0 = _jittered(9, 4)
    pts = torch.linspace(0.013, 0.987, 13, dtype=torch.float64)

    def f(xi):
        x = torch.cat([x0[:1], xi, x0[-1:]])
        return R.poisson(x, C, S, dict(OPT, load_quad_points=33), pts)[1]

    assert torch.autograd.gradcheck(f, (x0[1:-1].clone().requires_grad_(True),), eps=1e-7, atol=1e-5, rtol=1e-4)


def test_header_symbols_match_prototypes():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'gadapt_fem.h')).read()
    names = set(re.findall(r'\b(gadapt_fem\w*)\s*\(', hdr))
    assert names == set(_native_fem.PROTOTYPES)
    assert f"#define GADAPT_FEM_ABI {_native_fem.ABI_VERSION}" in hdr


def test_bad_grad_type_raises():
    d = MeshData(pde_params={'centers': [np.array([0.5], 'f')], 'scales': [np.array([0.1], 'f')]})
    with pytest.raises(ValueError):
        gradient_meshpoints_1D({}, d, torch.linspace(0, 1, 5))
    with pytest.raises(ValueError):
        gradient_meshpoints_1D({'grad_type': 'nope'}, d, torch.linspace(0, 1, 5))


def test_cpu_tensors_raise():
    params = [{'centers': [np.array([0.5], 'f')], 'scales': [np.array([0.1], 'f')]}]
    with pytest.raises(NativeError):
        burgers_1d(torch.linspace(0, 1, 5), [5], params, OPT, 1)
    with pytest.raises(NativeError):
        fem_poisson_1d(torch.linspace(0, 1, 5), [5], params, OPT)
    d = MeshData(pde_params=params[0])
    with pytest.raises(NativeError):
        gradient_meshpoints_1D(dict(OPT, grad_type='PDE_loss_direct_mse'), d, torch.linspace(0, 1, 21))


def test_dataset_defaults_unchanged_and_burgers_draws():
    a = MeshDataset([21], 4, seed=3)
    rng = np.random.default_rng(3)
    for s in a.samples:                  # today's draws: centres U(0,1), scales U(0.1,0.5), then the target noise
        c = [rng.uniform(0.0, 1.0, 1).astype('f') for _ in range(2)]
        sc = [rng.uniform(0.1, 0.5, 1).astype('f') for _ in range(2)]
        rng.standard_normal((21, 1))
        assert all(np.array_equal(u, v) for u, v in zip(s.pde_params['centers'], c))
        assert all(np.array_equal(u, v) for u, v in zip(s.pde_params['scales'], sc))
    b = MeshDataset([21], 20, seed=3, num_gauss=1, burgers=True)
    for s in b.samples:
        c, sc = float(s.pde_params['centers'][0][0]), float(s.pde_params['scales'][0][0])
        assert 0.3 <= c <= 0.7 and 0.05 <= sc <= 0.2


# ------------------------------------------------------------------------ the banded restatement against the dense one
BANDED_N = (2, 3, 4, 21, 65)


def _pin_meshes(dtype):
    for n in BANDED_N:
        yield f"n={n} uniform", _mesh(n, dtype=dtype)
        yield f"n={n} jittered", _mesh(n, jitter=0.3, seed=n, dtype=dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('k', [2, 11, 101])
def test_banded_mass_is_the_tridiagonal_part_of_the_dense_one(k, dtype):
    for label, x in _pin_meshes(dtype):
        M = R.mass_matrix(x, k)
        lo, di, up = R.mass_bands(x, k)
        assert di.dtype == dtype
        assert torch.equal(di, torch.diagonal(M)), (label, k)
        assert torch.equal(lo, torch.diagonal(M, -1)) and torch.equal(up, torch.diagonal(M, 1)), (label, k)
        assert torch.equal(R.mass_matrix(x, k, banded=True), torch.tril(torch.triu(M, -1), 1)), (label, k)


@pytest.mark.parametrize('k', [2, 11, 101])
def test_dense_mass_beyond_the_three_diagonals_is_rounding_level(k):
    """The 'rounding-level terms' the kernel header says mass_rows drops: at most 1e-12 of the largest entry in fp64."""
    for label, x in _pin_meshes(torch.float64):
        M = R.mass_matrix(x, k)
        far = (M - torch.tril(torch.triu(M, -1), 1)).abs().max().item()
        assert far <= 1e-12 * M.abs().max().item(), (label, k, far, M.abs().max().item())


@pytest.mark.parametrize('k', [2, 11, 101])
def test_banded_burgers_and_its_mesh_gradient_equal_the_dense_run(k):
    """fp64 rounding: 1e-11 of the largest value (the banded run differs by the dropped terms, 1e-12 of M, through two
    solves whose condition is of order 10; a missing or misplaced band would be an O(1) difference)."""
    opt = dict(OPT, load_quad_points=k, eval_quad_points=k)
    pts = torch.linspace(0.013, 0.987, 17, dtype=torch.float64)
    for label, x in _pin_meshes(torch.float64):
        out = {}
        for banded in (False, True):
            xx = x.clone().requires_grad_(True)
            u, sol, fsol = R.burgers(xx, C, S, opt, 2, pts, banded=banded)
            (sol ** 2).sum().backward()
            out[banded] = (u.detach(), sol.detach(), fsol, xx.grad)
        for name, a, b in zip(('u', 'sol', 'fine_sol', 'x.grad'), out[True], out[False]):
            assert (a - b).abs().max().item() <= 1e-11 * max(b.abs().max().item(), 1e-3), (label, k, name)
    xx = _mesh(21, jitter=0.3, seed=2).requires_grad_(True)
    o = dict(opt, grad_type='burgers_timestep_loss_direct_mse', num_time_steps=2)
    assert abs(R.modular_loss(xx, C, S, o, pts, banded=True).item() - R.modular_loss(xx, C, S, o, pts).item()) <= 1e-14
