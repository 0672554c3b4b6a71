"""The seven Monge-Ampere kernels against bits recorded before their shared iteration was stated once
(tests/golden/ma_routes/ma_routes.npz, tools/make_ma_golden.py: the cases, and the commit the fixture is from).

ma_kernel, ma_m2n_kernel, ma_m2n_slow_kernel, ma_table_kernel and the three strided kernels, three launches each: a mixed batch
stopped by the cap after 30 updates, a small batch run to tol, one mesh that loses convexity.  The kernels use no atomics and
every reduction runs in a fixed order, so the comparison is torch.equal on coords, steps, residual and status (and, under the
slow monitor, the monitor): a helper that reassociates a sum, a barrier that moved or an LDS row that changed shows here.
The results are computed once and shared by the tests."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]                    # no graph is built: one kernel dispatch a launch
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'ma_routes', 'ma_routes.npz')

_spec = importlib.util.spec_from_file_location('make_ma_golden', os.path.join(HERE, '..', 'tools', 'make_ma_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def _computed():
    return G.compute(_golden(), torch.device('cuda:0'))


def test_fixture_is_of_these_cases():
    g = _golden()
    assert os.path.getsize(GOLDEN) <= G.MAX_BYTES
    assert sorted(k for k in g if '_in_' not in k) == sorted(G.names())
    inp = G.inputs()
    assert sorted(k for k in g if '_in_' in k) == sorted(inp)
    for k, v in inp.items():
        assert g[k].dtype == v.dtype and np.array_equal(g[k], v), k
    for kernel in G.KERNELS:                               # each exit of each kernel at least once, and where it was wanted
        seen = set()
        for launch in G.LAUNCHES:
            status = g[f'{kernel}_{launch}_status'].tolist()
            assert status == [G.WANTED[launch]] * len(g[f'{kernel}_{launch}_in_sides']), (kernel, launch, status)
            seen |= set(status)
        assert seen == {G.CONVERGED, G.CAP, G.NONCONVEX}, (kernel, seen)
        assert g[f'{kernel}_cap_steps'].tolist() == [G.SOLVER['cap']['max_steps']] * len(g[f'{kernel}_cap_steps'])


@pytest.mark.parametrize('name', G.names())
def test_bits(name):
    want, got = torch.from_numpy(_golden()[name]), torch.from_numpy(_computed()[name])
    assert got.dtype == want.dtype and got.shape == want.shape
    same = torch.equal(got, want) or (name.endswith('_residual') and torch.equal(got.view(torch.int32), want.view(torch.int32)))
    assert same, f"{name}: {(got.double() - want.double()).abs().nan_to_num(float('inf')).max().item():.3e} from the recorded bits"
