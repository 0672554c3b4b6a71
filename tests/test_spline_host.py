"""CPU checks of the spline and the Burgers evaluation: the fp64 restatement against scipy's recorded answers (and scipy
itself where it imports) - which pins what "the reference's spline" means -, exactness on cubics, the C-ABI row and the
refusals that must come before anything touches a GPU."""
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spline_restatement as S  # noqa: E402

from g_adaptivity_amd import (MeshDataset, _native_fem, cubic_spline_1d, evaluate_model_fine_burgers,  # noqa: E402
                              evaluate_model_fine_burgers_time_step)
from g_adaptivity_amd import evaluation_burgers as eb  # noqa: E402
from g_adaptivity_amd._native import NativeError  # noqa: E402

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'burgers_eval', 'spline_*.npz')))


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def test_fixtures_exist():
    assert len(GOLDEN) == 5


@pytest.mark.parametrize('path', GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_restatement_equals_scipy_fixture(path):
    d = np.load(path)
    for deriv, names in ((0, ('s0', 'c0')), (1, ('c1',)), (2, ('s2', 'c2'))):
        r = S.spline(d['x'], d['y'], d['q'], deriv).numpy()
        for name in names:                                   # s*: UnivariateSpline(s=0); c*: CubicSpline(bc_type='not-a-knot')
            assert _rel(r, d[name]) <= 1e-10, (name, _rel(r, d[name]))


@pytest.mark.parametrize('path', GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_restatement_equals_scipy_directly(path):
    interpolate = pytest.importorskip('scipy.interpolate')
    d = np.load(path)
    x, y, q = (d[k].astype(np.float64) for k in ('x', 'y', 'q'))
    us = interpolate.UnivariateSpline(x, y, s=0)
    assert _rel(S.spline(x, y, q, 0).numpy(), us(q)) <= 1e-10
    assert _rel(S.spline(x, y, q, 2).numpy(), us.derivative(2)(q)) <= 1e-10
    assert _rel(S.spline(x, y, q, 1).numpy(), us.derivative(1)(q)) <= 1e-10


def test_four_points_reproduce_a_cubic():
    p = lambda t: 0.3 - 1.1 * t + 2.0 * t ** 2 - 0.7 * t ** 3
    x = torch.tensor([0.0, 0.2, 0.65, 1.0], dtype=torch.float64)
    q = torch.linspace(-0.1, 1.1, 25, dtype=torch.float64)
    assert torch.allclose(S.spline(x, p(x), q, 0), p(q), rtol=0, atol=1e-13)
    assert torch.allclose(S.spline(x, p(x), q, 1), -1.1 + 4.0 * q - 2.1 * q ** 2, rtol=0, atol=1e-12)


@pytest.mark.parametrize('n', [4, 5, 17])
def test_second_derivative_of_a_cubic_is_linear(n):
    p = lambda t: 0.3 - 1.1 * t + 2.0 * t ** 2 - 0.7 * t ** 3
    x = torch.sort(torch.rand(n, dtype=torch.float64, generator=torch.Generator().manual_seed(n))).values
    q = torch.linspace(float(x[0]) - 0.05, float(x[-1]) + 0.05, 31, dtype=torch.float64)
    assert torch.allclose(S.spline(x, p(x), q, 2), 4.0 - 4.2 * q, rtol=0, atol=1e-9)


def test_header_row_and_library():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'gadapt_fem.h')).read()
    decl = re.search(r'\bgadapt_fem1d_spline\s*\(([^;]*)\);', hdr).group(1)
    assert len(decl.split(',')) == len(_native_fem.PROTOTYPES['gadapt_fem1d_spline'][1])
    for name, v in (('OK', _native_fem.SPLINE_OK), ('NOT_INCREASING', _native_fem.SPLINE_NOT_INCREASING),
                    ('NOT_FINITE', _native_fem.SPLINE_NOT_FINITE), ('BAD_COUNT', _native_fem.SPLINE_BAD_COUNT)):
        assert re.search(r'#define GADAPT_SPLINE_S_%s\s+%d\b' % (name, v), hdr)
    lib = _native_fem.lib()
    assert lib.gadapt_fem1d_spline(1, 4, None, None, None, 1, None, None, 0, None, None, None) == -1
    assert b'gadapt_fem1d_spline' in lib.gadapt_fem_last_error()
    import ctypes
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)
    assert lib.gadapt_fem1d_spline(1, 3, p, p, p, 1, p, None, 0, p, p, None) == -1          # fewer than four points
    assert lib.gadapt_fem1d_spline(1, 1025, p, p, p, 1, p, None, 0, p, p, None) == -5       # GADAPT_FEM_E_LDS
    assert lib.gadapt_fem1d_spline(1, 4, p, p, p, 1, p, None, 3, p, p, None) == -1          # deriv
    assert lib.gadapt_fem1d_spline(1, 4, p, p, p, 0, p, None, 0, p, p, None) == -1          # no shared query


def test_cubic_spline_1d_refuses_cpu_tensors():
    x = torch.linspace(0, 1, 5)
    with pytest.raises(NativeError, match='no CPU fallback'):
        cubic_spline_1d(x, x, [5], x)
    with pytest.raises(TypeError):
        cubic_spline_1d(x.numpy(), x, [5], x)


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the argument checks run before anything is launched."""
    is_cuda = True


def _fake(t):
    return t.as_subclass(_FakeCuda)


@pytest.mark.parametrize('kw,match', [
    (dict(counts=[3]), r'4\.\.1024'), (dict(counts=[1025]), r'4\.\.1024'), (dict(counts=[]), 'no data sets'),
    (dict(counts=[4]), 'counts summing'), (dict(deriv=3), 'deriv'), (dict(q_counts=[2, 2]), 'q_counts'),
    (dict(q_counts=[4]), 'q_counts')])
def test_cubic_spline_1d_argument_refusals(kw, match):
    x = _fake(torch.linspace(0, 1, 5))
    args = dict(counts=[5], q_counts=None, deriv=0)
    if 'counts' in kw and kw['counts'] in ([3], [1025]):
        x = _fake(torch.linspace(0, 1, kw['counts'][0]))
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        cubic_spline_1d(x, x, args['counts'], _fake(torch.linspace(0, 1, 5)), q_counts=args['q_counts'], deriv=args['deriv'])


class _NoModel:
    end_MLmodel = None

    def __call__(self, data):
        raise AssertionError("the model must not run before the refusals")


OPT = {'device': 'cpu', 'tau': 0.05, 'nu': 1e-3, 'num_fine_mesh_points': 20, 'mon_reg': 0.1, 'mon_power': 0.2,
       'num_time_steps': 1, 'num_eval_time_steps': 4}


@pytest.mark.parametrize('fn', [evaluate_model_fine_burgers, evaluate_model_fine_burgers_time_step])
def test_evaluation_refusals(fn):
    with pytest.raises(NotImplementedError, match='1-D'):
        fn(_NoModel(), MeshDataset([7, 7], 2, seed=0), OPT)
    ds = MeshDataset([11], 2, seed=0, num_gauss=1, burgers=True)
    with pytest.raises(NotImplementedError, match='Burgers'):
        fn(_NoModel(), ds, dict(OPT, pde_type='Poisson'))
    keys = ['tau', 'nu', 'num_fine_mesh_points'] + (['mon_reg', 'mon_power'] if fn is evaluate_model_fine_burgers_time_step else [])
    for k in keys:
        with pytest.raises(ValueError, match=k):
            fn(_NoModel(), ds, {a: b for a, b in OPT.items() if a != k})
    with pytest.raises(ValueError, match='batch_size'):
        fn(_NoModel(), ds, OPT, batch_size=0)
    with pytest.raises(NativeError):                        # past the refusals: the GPU-only FEM tail, no CPU fallback
        fn(_NoModel(), ds, OPT)


def test_rollout_needs_two_evaluation_steps():
    ds = MeshDataset([11], 1, seed=0, num_gauss=1, burgers=True)
    with pytest.raises(ValueError, match='num_eval_time_steps'):
        evaluate_model_fine_burgers_time_step(_NoModel(), ds, dict(OPT, num_eval_time_steps=1))


def test_columns_are_the_references():
    assert eb.BURGERS_ERROR_COLUMNS == ['L2_grid', 'L2_MA', 'L2_MLmodel', 'L2_reduction_MA', 'L2_reduction_MLmodel']
    assert eb.BURGERS_TIME_COLUMNS == ['MA_time', 'MLmodel_time']
    assert eb.BURGERS_ROLLOUT_TIME_COLUMNS == ['MA_time', 'MA_mesh_time', 'MLmodel_time', 'ML_mesh_time']
    assert eb.MMPDE5_DEFAULTS == dict(cfl=0.05, tol=1e-6, max_steps=10000)
