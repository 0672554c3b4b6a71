"""The message-passing block routes against bits recorded before the host code behind their C-ABI was reorganised
(tests/golden/block_routes/block_routes.npz, tools/make_block_golden.py: the cases, and the commit the fixture is from).

Tiled dense and compact blocks, the wide forward, the narrow route in its forward modes and backward forms, hidden 64 on a
shuffled graph, hidden 128, the fused training step with its three tails and the evaluation forward, each through the
package's own caller.  The routes sum per-workgroup partials and slab rows in a fixed order, so the comparison is
torch.equal (arrays stored as a digest: equality of digest, shape and dtype): host code that passes another argument, grid,
LDS size or launch order to a kernel shows here.  The {d dt, d score_scale} pair of gadapt_layer_backward is accumulated with
float atomics and is not part of the fixture (tests/test_gpu_ops.py keeps its tolerance).  Each case is computed once and
shared by its arrays' tests."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]                    # every case sets graph.WIDE_MIN_NODES itself
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'block_routes', 'block_routes.npz')

_spec = importlib.util.spec_from_file_location('make_block_golden', os.path.join(HERE, '..', 'tools', 'make_block_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

CASES = ['tiled8_shared', 'tiled8_layers', 'tiled32_shared', 'tiled32_layers', 'layer8', 'compact32_L3_inplace', 'compact32_L3_apart',
         'compact32_L2_learn', 'wide64_dense', 'wide64_compact', 'wide64_compact_8waves',
         'narrow64_L4_f1_b1', 'narrow64_L4_f2_b0', 'narrow64_L4_f0_b1', 'narrow64_L6_f1_b1', 'narrow64_L6_f2_b0', 'narrow64_L6_f0_b1',
         'tiled64_shuffled', 'h128_rowmajor', 'h128_shuffled', 'fused_small_narrow', 'fused_small_tiled', 'fused_large_narrow',
         'eval_narrow', 'eval_tiled']


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def _computed(case):
    return G.compute(torch.device('cuda:0'), only=(case,))


def test_fixture_is_of_these_cases():
    assert sorted({k.split('.')[0] for k in _golden()}) == sorted(CASES) == sorted(G.cases(None))
    assert not any('d_scale' in k or 'sums' in k for k in _golden())


@pytest.mark.parametrize('case', CASES)
def test_bits(case):
    want = {k: v for k, v in _golden().items() if k.split('.')[0] == case}
    got = _computed(case)
    assert sorted(got) == sorted(want) and want
    for name in sorted(want):
        w, g = torch.from_numpy(want[name]), torch.from_numpy(got[name])
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if w.dtype == torch.uint8:                                          # sha256 | shape | dtype of a large array
            assert torch.equal(g, w), f"{name}: {bytes(got[name]).decode()} computed, {bytes(want[name]).decode()} recorded"
        else:
            assert torch.equal(g, w), f"{name}: {(g.double() - w.double()).abs().max().item():.3e} from the recorded bits"
