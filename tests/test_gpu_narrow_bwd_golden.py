"""The one-node-per-lane backward target passes against bits recorded before their wave sums moved from the LDS crossbar to DPP and
lane-swap steps (tests/golden/narrow_bwd/narrow_bwd.npz, tools/make_narrow_bwd_golden.py: the cases, and the commit the fixture is from).

What tests/golden/block_routes does not reach: 5 x 5 b1 (25 nodes: one partial wave), 16 x 16 b1 (exactly one 256-node workgroup),
17 x 17 b1 (a second workgroup of 33 nodes), 23 x 23 b7, 32 x 32 b3 and every graph of tests/narrow_graphs.py at the C-ABI level, hidden 64,
packed slab, with the top layer's target pass inside the forward launch and as a launch of its own - every slab row (rows without nodes
included), the dxd rows, both edge buffers, the gradient work buffers and the flat gradient after the tail - and the compact layer-0
kernel at hidden 32 with d dt (SUMS = 1) and d dt + d score_scale (SUMS = 2) through the per-workgroup partials.  Arrays are compared as
int32 bit patterns with torch.equal (arrays stored as a digest: equality of digest, shape and dtype).  Each case is computed once and
shared by its arrays."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import narrow_graphs as ng

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]                    # every case sets graph.WIDE_MIN_NODES itself
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'narrow_bwd', 'narrow_bwd.npz')

_spec = importlib.util.spec_from_file_location('make_narrow_bwd_golden', os.path.join(HERE, '..', 'tools', 'make_narrow_bwd_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

CASES = ['sq5_b1', 'sq16_b1', 'sq17_b1', 'sq23_b7', 'sq32_b3'] + [f'ng_{i}' for i in ng.IDS] + ['learn32_sums1', 'learn32_sums2']
# per switch position of a narrow case: what the backward call and the tail leave
AFTER = ('ran', 'slab', 'dxd', 'pairs0', 'pairs1', 'g', 'flat', 'loss')


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def _computed(case):
    return G.compute(torch.device('cuda:0'), only=(case,))


def test_fixture_is_of_these_cases():
    gold = _golden()
    assert sorted({k.split('.')[0] for k in gold}) == sorted(CASES) == sorted(G.cases(None))
    for case in CASES:
        if case.startswith('learn32'):
            continue
        for tag in ('in_fwd', 'apart'):                                     # nothing was left out as unstable when it was recorded
            assert all(f'{case}.{tag}.{what}' in gold for what in AFTER), (case, tag)
        assert int(gold[f'{case}.apart.ran'][0]) == 0
        big = case.startswith('ng_') and ng.CASES[case[3:]].big             # the 512-row window has no halo: the old launches
        assert int(gold[f'{case}.in_fwd.ran'][0]) == (0 if big else 1), case
        assert all((f'{case}.in_fwd.{what}' in gold) == (not big) for what in ('f_dxd', 'f_pairs', 'f_slab')), case
    assert 'learn32_sums1.d_steps' in gold and 'learn32_sums2.d_lp' in gold


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
            assert torch.equal(g, w), f"{name}: {(g != w).sum().item()} of {w.numel()} words differ from the recorded bits"
