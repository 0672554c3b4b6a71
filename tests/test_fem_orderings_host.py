"""Host side of the 2-D FEM tail on node orders other than square_mesh's (tests/fem_meshes.py): the band that
gadapt_fem_topology_host finds on each named case, which side of the 64 KB LDS budget each falls on, the ring slack of the
windowed solve at the widest bands, the equivariance of the fp64 restatement under a renumbering (what licenses it as the
reference on any ordering, tests/test_gpu_fem_orderings.py) and the union-jack triangulation.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fem_meshes as F  # noqa: E402
import fem_restatement as R  # noqa: E402
from test_gpu_modular2d import _coords, _params  # noqa: E402  (the mesh and Gaussian recipes)

from g_adaptivity_amd import _native_fem as nf  # noqa: E402
from g_adaptivity_amd.fem import FemTopology, _tri_counts  # noqa: E402
from g_adaptivity_amd.mesh_graph import square_mesh  # noqa: E402

BUDGET = 65536
# (side, seed, the band the seed was named for)
NAMED = [(11, F.SEED_N11_W77, 77), (11, F.SEED_N11_W78, 78), (11, F.SEED_N11_W79, 79), (11, F.SEED_N11_W80, 80),
         (12, F.SEED_N12_WIDE, F.W_N12_WIDE)]


def _named(n, seed):
    m = square_mesh(n)
    return F.permuted(m, m.x_comp, seed=seed)


@pytest.mark.parametrize('n,seed,w', NAMED)
def test_topology_band_of_named_cases(n, seed, w):
    x, cells, bnd, perm = _named(n, seed)
    m = square_mesh(n)
    assert torch.equal(x[torch.from_numpy(perm)], m.x_comp) and torch.equal(bnd[torch.from_numpy(perm)], m.boundary_nodes)
    assert F.band_of(cells, bnd) == w
    topo = FemTopology(cells.numpy(), bnd.numpy(), [n * n], [cells.shape[0]], 'cpu')      # 'lds' takes all five
    assert int(topo.band[0]) == w and int(topo.n_int[0]) == (n - 2) ** 2
    # the interior numbering band_of assumes: interior nodes in increasing node id
    assert np.array_equal(topo.host['int_node'][:topo.n_int[0]], np.flatnonzero(~bnd.numpy()))


def test_named_seeds_are_the_first_hits():
    assert F.first_seed(11, lambda b: b == 80) == F.SEED_N11_W80          # the latest of the five
    assert F.first_seed(11, lambda b: b == 79) == F.SEED_N11_W79
    assert F.first_seed(11, lambda b: b == 78) == F.SEED_N11_W78
    assert F.first_seed(11, lambda b: b == 77) == F.SEED_N11_W77
    assert F.first_seed(12, lambda b: b >= 90) == F.SEED_N12_WIDE and F.W_N12_WIDE >= 90


def test_natural_band_and_band_of_agree():
    for n in (3, 4, 7, 12):
        m = square_mesh(n)
        assert F.band_of(m.cells, m.boundary_nodes) == (n - 2 if n > 3 else 0)     # 3 x 3: one unknown, no band
    x, cells, bnd = F.union_jack(9)
    assert F.band_of(cells, bnd) == 8                                     # the other diagonal joins (ix, iy) and (ix+1, iy+1)


def test_each_case_on_its_side_of_the_budget():
    lib = nf.lib()
    assert int(lib.gadapt_fem_lds_budget()) == BUDGET
    n_int = 81
    assert lib.gadapt_fem_window_lds_bytes(n_int, 77) == 61308
    assert lib.gadapt_fem_window_lds_bytes(n_int, 78) == 63516
    assert lib.gadapt_fem_window_lds_bytes(n_int, 79) == 64480 <= BUDGET      # the windowed maximum, whatever the mesh
    assert lib.gadapt_fem_window_lds_bytes(n_int, 80) == 66744 > BUDGET
    assert lib.gadapt_fem_factor_lds_bytes(n_int, 80) == 39528 <= BUDGET      # ... which the resident band takes at 11 x 11
    lds12 = lib.gadapt_fem_factor_lds_bytes(100, F.W_N12_WIDE)
    assert lds12 == 100 * (F.W_N12_WIDE + 1) * 4 + 400 + F.W_N12_WIDE * (F.W_N12_WIDE + 1) // 2 * 4 <= BUDGET
    # FemTopology draws the same line
    x, cells, bnd, _ = _named(11, F.SEED_N11_W79)
    assert FemTopology(cells.numpy(), bnd.numpy(), [121], [200], 'cpu', band='window').lds_bytes == 64480
    x, cells, bnd, _ = _named(11, F.SEED_N11_W80)
    with pytest.raises(NotImplementedError, match='half-bandwidth 80'):
        FemTopology(cells.numpy(), bnd.numpy(), [121], [200], 'cpu', band='window')
    assert FemTopology(cells.numpy(), bnd.numpy(), [121], [200], 'cpu').lds_bytes == 39528
    # the documented maxima: 26 x 26 resident, 27 x 27 not; 81 x 81 windowed (w = 79), 82 x 82 not
    assert lib.gadapt_fem_factor_lds_bytes(24 * 24, 24) == 61104 <= BUDGET < lib.gadapt_fem_factor_lds_bytes(25 * 25, 25)
    assert lib.gadapt_fem_window_lds_bytes(79 * 79, 79) <= BUDGET < lib.gadapt_fem_window_lds_bytes(80 * 80, 80)


@pytest.mark.parametrize('w', [77, 78, 79])
def test_far_swap_gives_a_band_wider_than_the_ring_is_long(w):
    """12 x 12 with two interior nodes swapped: band w on 100 unknowns, more than the ring's R = w + S rows."""
    m = square_mesh(12)
    x, cells, bnd, perm = F.permuted(m, m.x_comp, perm=F.far_swap(12, w))
    assert (perm != np.arange(144)).sum() == 2 and not bnd[perm != np.arange(144)].any()
    assert F.band_of(cells, bnd) == w
    topo = FemTopology(cells.numpy(), bnd.numpy(), [144], [cells.shape[0]], 'cpu', band='window')
    assert int(topo.band[0]) == w and int(topo.n_int[0]) == 100 > w + _ring_slack(w, BUDGET)
    assert 81 <= 77 + _ring_slack(77, BUDGET)                   # the 11 x 11 cases: every row has its own slot, no wrap


def _ring_slack(w, lds_bytes):
    """win_layout's S (fem_csrc/fem_window_kernels.hip): the rows the ring's LDS holds, less the band, at most half, at most 64."""
    ld = w + 1
    ldp, pairs = (ld + 1) & ~1, w * (w + 1) // 2
    rows = (lds_bytes - 4 * pairs) // (8 * (ldp + 1))
    return min(rows - w, rows // 2, 64)


def test_ring_slack_at_the_widest_bands():
    """At the full budget the ring of w = 77 / 78 / 79 has 84 / 82 / 81 rows: S = 7 / 4 / 2 (at w = 78 three rows beyond the
    minimum of w + 1, which is S = 4), R = w + S, against S = 64 at 27 x 27 and 49 at 64 x 64."""
    assert [_ring_slack(w, BUDGET) for w in (77, 78, 79)] == [7, 4, 2]
    assert _ring_slack(25, BUDGET) == 64 and _ring_slack(62, BUDGET) == 49
    lib = nf.lib()
    for w in (77, 78, 79):                                                 # S = 1 at the bytes the library asks for
        assert _ring_slack(w, lib.gadapt_fem_window_lds_bytes(81, w)) == 1
    assert _ring_slack(80, BUDGET) < 1


def test_tri_counts_of_a_renumbered_batch():
    """fem._tri_counts splits a batch's cells at the meshes' node ranges; within a renumbered mesh the ids are in no order."""
    parts, counts, off = [], [], 0
    for n, seed in ((3, None), (12, F.SEED_N12_WIDE), (11, F.SEED_N11_W79), (5, None)):
        cells = square_mesh(n).cells if seed is None else _named(n, seed)[1]
        parts.append(cells + off)
        counts.append(n * n)
        off += n * n
    assert _tri_counts(torch.cat(parts, 0), counts) == [p.shape[0] for p in parts]


def test_fp64_restatement_is_equivariant():
    """fem_restatement.fem2d on a renumbered mesh: the natural result's coefficients, reindexed, and its lattice values."""
    n = 12
    x, m = _coords(n, 'jittered', seed=n + 1)
    p = _params(2, n)
    lat = torch.linspace(0, 1, 101, dtype=torch.float64)
    c0, s0 = R.fem2d(x.double(), m.cells, m.boundary_nodes, p['centers'], p['scales'], lat)
    xp, cells, bnd, perm = F.permuted(m, x, seed=F.SEED_N12_WIDE)
    c1, s1 = R.fem2d(xp.double(), cells, bnd, p['centers'], p['scales'], lat)
    dc, ds = (c1[torch.from_numpy(perm)] - c0).abs().max().item(), (s1 - s0).abs().max().item()
    print(f"FEM-ORDERINGS fp64 restatement, 12 x 12 renumbered (w = {F.W_N12_WIDE}): coeffs {dc:.1e} sol {ds:.1e} (|c|max {c0.abs().max().item():.2f})")
    assert dc <= 1e-12 and ds <= 1e-12
    # and under another triangle order
    c2, s2 = R.fem2d(x.double(), F.shuffled_triangles(m.cells, 5), m.boundary_nodes, p['centers'], p['scales'], lat)
    assert (c2 - c0).abs().max().item() <= 1e-12 and (s2 - s0).abs().max().item() <= 1e-12


def test_shuffled_triangles_holds_the_same_triangles():
    cells = square_mesh(11).cells
    sh = F.shuffled_triangles(cells, 5)
    assert not torch.equal(sh, cells)
    assert sorted(map(tuple, sh.tolist())) == sorted(map(tuple, cells.tolist()))


@pytest.mark.parametrize('n', [3, 4, 9, 12])
def test_union_jack(n):
    x, cells, bnd = F.union_jack(n)
    m = square_mesh(n)
    assert cells.shape == (2 * (n - 1) ** 2, 3) and torch.equal(x, m.x_comp)
    assert torch.equal(bnd, m.boundary_nodes)
    tri = x.double()[cells]
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    signed = 0.5 * ((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0]))
    tm = x.double()[m.cells]
    ref = 0.5 * ((tm[:, 1, 0] - tm[:, 0, 0]) * (tm[:, 2, 1] - tm[:, 0, 1]) - (tm[:, 1, 1] - tm[:, 0, 1]) * (tm[:, 2, 0] - tm[:, 0, 0]))
    assert bool((signed * ref[0].sign() > 0).all()) and bool((ref * ref[0].sign() > 0).all())     # square_mesh's orientation
    assert abs(signed.abs().sum().item() - 1.0) < 1e-12
    valence = torch.bincount(cells.reshape(-1), minlength=n * n)
    assert set(valence[~bnd].tolist()) <= {4, 8}
    if n >= 4:
        assert set(valence[~bnd].tolist()) == {4, 8}
    # every jittered mesh of the GPU tests keeps its triangles the right way round
    xj, _ = _coords(n, 'jittered', seed=n + 1)
    tj = xj.double()[cells]
    sj = (tj[:, 1, 0] - tj[:, 0, 0]) * (tj[:, 2, 1] - tj[:, 0, 1]) - (tj[:, 1, 1] - tj[:, 0, 1]) * (tj[:, 2, 0] - tj[:, 0, 0])
    assert bool((sj * ref[0].sign() > 0).all())
