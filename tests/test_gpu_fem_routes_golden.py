"""The 2-D FEM tails on both band routes against bits recorded before their host code was reorganised
(tests/golden/fem2d_routes/fem2d_routes.npz, tools/make_fem2d_golden.py: the cases, and the commit the fixture is from).

fem_poisson with its gradient, modular_loss_2d ('mse', 'simpson') and poisson_eval_errors on 'lds' and 'window',
mesh_descent_2d on 'lds', one mixed batch of three small meshes: every launch sequence behind the C-ABI of
fem_csrc/fem_kernels.hip and descent_kernels.hip.  The kernels use no float atomics and every sum runs in a fixed order, so
the comparison is torch.equal: host code that passes another argument, LDS size or launch order to a kernel shows here.
The results are computed once and shared by the tests."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]                    # no graph is built: one kernel dispatch
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'fem2d_routes', 'fem2d_routes.npz')

_spec = importlib.util.spec_from_file_location('make_fem2d_golden', os.path.join(HERE, '..', 'tools', 'make_fem2d_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

LDS_ONLY = ['descent_x', 'descent_loss_hist', 'descent_mesh_hist', 'descent_first_tangled', 'descent_min_area']
PER_ROUTE = ['coeffs', 'sol', 'grad', 'mse_loss', 'mse_x_grads', 'simpson_loss', 'simpson_x_grads', 'L1', 'L2']
NAMES = [f'{r}_{w}' for r in G.ROUTES for w in PER_ROUTE] + [f'lds_{w}' for w in LDS_ONLY]


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def _computed(tri_slab):
    return G.compute(_golden(), torch.device('cuda:0'), tri_slab=tri_slab)


def test_fixture_is_of_these_cases():
    g = _golden()
    assert sorted(k for k in g if not k.startswith('in_')) == sorted(NAMES)
    inp = G.inputs()
    assert all(np.array_equal(g[k], inp[k]) for k in ('in_centers', 'in_scales'))
    x0, _, bnd, _, _ = G.topology()
    assert np.array_equal(g['in_x'][bnd.numpy()], x0.numpy()[bnd.numpy()])      # boundary nodes stay where the grid has them


@pytest.mark.parametrize('name', NAMES)
def test_bits(name):
    want, got = torch.from_numpy(_golden()[name]), torch.from_numpy(_computed(0)[name])
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(got, want), f"{name}: {(got.double() - want.double()).abs().max().item():.3e} from the recorded bits"


def test_window_does_not_depend_on_tri_slab():
    """tri_slab = 32 (the largest mesh's 242 triangles in eight slabs) against tri_slab = 0 (one slab)."""
    a, b = _computed(0), _computed(32)
    for name in NAMES:
        if name.startswith('window_'):
            assert torch.equal(torch.from_numpy(a[name]), torch.from_numpy(b[name])), name
