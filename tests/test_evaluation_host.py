"""CPU checks of the evaluation (g_adaptivity_amd/evaluation.py): the numpy helpers against the test-side restatement, the
C-ABI table, the refusals and the shape of the returned tables."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_restatement as E  # noqa: E402

from g_adaptivity_amd import MeshDataset, _native_fem, evaluation as ev  # noqa: E402
from g_adaptivity_amd._native import NativeError  # noqa: E402
from g_adaptivity_amd.mesh_graph import square_mesh  # noqa: E402

NEW_SYMBOLS = ('gadapt_fem_eval_errors', 'gadapt_fem1d_poisson_eval_errors')


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_numpy_helpers_match_the_restatement(seed):
    rng = np.random.default_rng(seed)
    n = 17 + seed
    x = np.sort(rng.uniform(0, 1, n)); x[0], x[-1] = 0.0, 1.0
    uu, ut = rng.standard_normal(n), rng.standard_normal(n)
    l1, l2 = ev.evaluate_error_np(uu, ut, x)
    r1, r2 = E.trapezium_1d(torch.from_numpy(uu), torch.from_numpy(ut), torch.from_numpy(x))
    assert l1 == pytest.approx(float(r1), rel=1e-12) and l2 == pytest.approx(float(r2), rel=1e-12)
    # 2-D: the reference's grid is np.meshgrid(x, y) ('xy'); the restatement reads the same field in 'ij'
    X, Y = np.meshgrid(x, x)
    f_ij, g_ij = rng.standard_normal((n, n)), rng.standard_normal((n, n))            # [i, j] <-> (x_i, y_j)
    l1, l2 = ev.evaluate_error_np_2d(f_ij.T.reshape(-1), g_ij.T.reshape(-1), np.array([X, Y]))
    r1, r2 = E.trapezium_2d(torch.from_numpy(f_ij.reshape(-1)), torch.from_numpy(g_ij.reshape(-1)), torch.from_numpy(x))
    assert l1 == pytest.approx(float(r1), rel=1e-12) and l2 == pytest.approx(float(r2), rel=1e-12)


def test_uniform_lattice_weights_are_one_half_quarter():
    n = 9
    ax = np.linspace(0, 1, n)
    X, Y = np.meshgrid(ax, ax)
    e = np.random.default_rng(3).standard_normal((n, n))
    w = np.ones(n); w[0] = w[-1] = 0.5
    h = 1.0 / (n - 1)
    l1, l2 = ev.evaluate_error_np_2d(e.reshape(-1), np.zeros(n * n), np.array([X, Y]))
    assert l1 == pytest.approx(h * h * (np.abs(e) * w[:, None] * w[None, :]).sum(), rel=1e-12)
    assert l2 == pytest.approx(np.sqrt(h * h * (e ** 2 * w[:, None] * w[None, :]).sum()), rel=1e-12)


def test_calculate_error_reduction():
    assert ev.calculate_error_reduction(2.0, 1.0) == -50.0
    assert ev.calculate_error_reduction(0.3, 0.45) == (0.45 - 0.3) / 0.3 * 100 == E.reduction(0.3, 0.45)
    assert ev.calculate_error_reduction(1.0, 0.) is None and E.reduction(1.0, 0.) is None


def test_header_table_and_library_agree():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'gadapt_fem.h')).read()
    names = set(re.findall(r'\b(gadapt_fem\w*)\s*\(', hdr))
    assert names == set(_native_fem.PROTOTYPES) and set(NEW_SYMBOLS) <= names
    assert _native_fem.ABI_VERSION == 4 and "#define GADAPT_FEM_ABI 4" in hdr
    if not os.path.exists(_native_fem.LIB_PATH):
        pytest.fail("libgadapt_fem.so not built")
    lib = _native_fem.lib()
    assert lib.gadapt_fem_abi_version() == 4
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
        # arity of the ctypes row = parameters of the declaration
        decl = re.search(r'\b' + name + r'\s*\(([^;]*)\);', hdr).group(1)
        assert len(decl.split(',')) == len(_native_fem.PROTOTYPES[name][1]), name
    assert lib.gadapt_fem_eval_partials_floats(3) == 3 * 8 * 2


def test_entry_points_validate_before_launching():
    lib = _native_fem.lib()
    args = [1, 4, 2] + [None] * 12 + [2, 1024, 2] + [None] * 6
    assert lib.gadapt_fem_eval_errors(*args) == -1 and b'gadapt_fem_eval_errors' in lib.gadapt_fem_last_error()
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)
    assert lib.gadapt_fem1d_poisson_eval_errors(1, 5, None, None, None, None, 101, 3, 101, None, None, None, None) == -1
    assert lib.gadapt_fem1d_poisson_eval_errors(1, 2000, p, p, p, p, 101, 3, 101, p, p, p, None) == -5      # GADAPT_FEM_E_LDS
    assert lib.gadapt_fem1d_poisson_eval_errors(1, 5, p, p, p, p, 101, 3, 1, p, p, p, None) == -1           # one point: no interval


def _params2d():
    return [{'centers': [np.array([0.4, 0.5], 'f')], 'scales': [np.array([0.3, 0.2], 'f')]}]


def test_cpu_tensors_raise():
    m = square_mesh(7)
    with pytest.raises(NativeError, match='no CPU fallback'):
        ev.poisson_eval_errors(m.x_comp, [49], _params2d(), 101, cells=m.cells, boundary=m.boundary_nodes)
    with pytest.raises(NativeError):
        ev.poisson_eval_errors(torch.linspace(0, 1, 11), [11], [{'centers': [np.array([0.5], 'f')], 'scales': [np.array([0.1], 'f')]}], 101)


class _NoModel:
    end_MLmodel = None

    def __call__(self, data):
        raise AssertionError("the model must not run before the refusals")


@pytest.mark.parametrize('opt,fine,match', [({'solver': 'firedrake'}, True, 'Firedrake'), ({'evaler': 'fd_*'}, True, 'Firedrake'),
                                            ({}, False, 'fine_eval=False')])
def test_refusals(opt, fine, match):
    ds = MeshDataset([7, 7], 2, seed=0)
    with pytest.raises(NotImplementedError, match=match):
        ev.evaluate_model_fine(_NoModel(), ds, dict(opt, device='cpu'), fine_eval=fine)
    if fine:
        with pytest.raises(NotImplementedError, match=match):
            ev.eval_grid_MMPDE_MA(ds, dict(opt, device='cpu'))


def test_defaults_reach_the_native_call():
    # no solver / evaler / eval_quad_points keys: torch_FEM, analytical, 101 - the call gets as far as the GPU-only FEM tail
    ds = MeshDataset([7, 7], 2, seed=0)
    with pytest.raises(NativeError):
        ev.eval_grid_MMPDE_MA(ds, {'device': 'cpu'})


def test_table_columns_and_order():
    class Still:                                          # a model that leaves the mesh where it is
        end_MLmodel = 0.0

        def __call__(self, data):
            import time
            self.end_MLmodel = time.time()
            return data.x_comp

    ds = MeshDataset([7, 7], 3, seed=0)
    for i, s in enumerate(ds.samples):                    # pre-processed evaluation data, as the reference's datasets carry it
        s.eval_errors = {k: torch.tensor(v * (i + 1)) for k, v in (('L1_grid', 0.02), ('L2_grid', 0.03), ('L1_MA', 0.01), ('L2_MA', 0.02))}
    keep = ev._errors_of
    ev._errors_of = lambda coords, samples, n_eval, opt, dev: torch.tensor([[0.01, 0.0]] * len(coords))
    try:
        df, dt = ev.evaluate_model_fine(Still(), ds, {'device': 'cpu', 'overfit_num': [0, 2]})
    finally:
        ev._errors_of = keep
    assert list(df.keys()) == ['L1_grid', 'L2_grid', 'L1_MA', 'L2_MA', 'L1_MLmodel', 'L2_MLmodel', 'L1_reduction_MA',
                               'L2_reduction_MA', 'L1_reduction_MLmodel', 'L2_reduction_MLmodel'] == ev.ERROR_COLUMNS
    assert list(dt.keys()) == ['MA_time', 'MLmodel_time'] == ev.TIME_COLUMNS
    assert len(df['L1_grid']) == 2 and len(dt['MA_time']) == 2                       # overfit_num: samples 0 and 2
    assert float(np.asarray(df['L1_grid'])[1]) == pytest.approx(0.06, rel=1e-6)
    assert float(np.asarray(df['L1_reduction_MA'])[0]) == pytest.approx(-50.0, rel=1e-6)
    assert np.isnan(np.asarray(df['L2_reduction_MLmodel'], dtype=float)).all()       # e_adapted == 0 -> None -> NaN in the table
    assert np.isnan(np.asarray(dt['MA_time'], dtype=float)).all()                    # no build_time recorded
    assert (np.asarray(dt['MLmodel_time'], dtype=float) >= 0).all()
