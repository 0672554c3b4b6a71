"""The eight 1-D entry points of libgadapt_fem.so against bits recorded before their host code was reorganised
(tests/golden/fem1d_routes/fem1d_routes.npz, tools/make_fem1d_golden.py: the cases, and the commit the fixture is from).

Burgers and Poisson forward and backward, the evaluation's error norms, the descent, the projection-only call, fn_expansion and
the spline, at the smallest shapes at which host code can hand a kernel a wrong size: the node cap (the Poisson layout at exactly
65536 B, the Burgers forward at 65516 B), wave and workgroup edges, both spline launch shapes.  The kernels use no float atomics
and every sum runs in a fixed order, so the comparison is torch.equal on the bit patterns (NaN and inf included): host code that
passes another argument, LDS size or workgroup size to a kernel shows here.  The inputs come from the fixture; the results are
computed once and shared by the tests."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]                    # no graph is built: one kernel dispatch
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'fem1d_routes', 'fem1d_routes.npz')

_spec = importlib.util.spec_from_file_location('make_fem1d_golden', os.path.join(HERE, '..', 'tools', 'make_fem1d_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def _computed():
    g = _golden()
    return G.computed({k: v for k, v in g.items() if k.startswith('in_')}, torch.device('cuda:0'))


def _bits(a):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_fixture_is_of_these_cases():
    g = _golden()
    assert len(G.NAMES) == len(set(G.NAMES)) == 85
    assert sorted(k for k in g if not k.startswith('in_')) == sorted(G.NAMES)
    inp = G.inputs()
    assert sorted(k for k in g if k.startswith('in_')) == sorted(inp)
    assert all(g[k].shape == inp[k].shape and g[k].dtype == np.float32 for k in inp)
    assert all(g[f'in_{case}_x'].shape == (sum(counts),) for case, counts in G.COUNTS.items())
    x = g['in_not_increasing_x']
    assert x[4] < x[3] and (np.diff(x[9:]) > 0).all()                        # one folded mesh beside a good one
    assert g['poisson_cap_flags'].dtype == np.int32 and g['not_increasing_flags'].tolist() == [1, 0]
    assert g['spline_a_shared_d0_status'].tolist() == [0, 0, 1] and g['spline_b_own_d2_status'].tolist() == [0, 0]


@pytest.mark.parametrize('name', G.NAMES)
def test_bits(name):
    want, got = _golden()[name], _computed()[name]
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(_bits(got), _bits(want)), f"{name}: {int((_bits(got) != _bits(want)).sum())} of {want.size} values differ from the recorded bits"
