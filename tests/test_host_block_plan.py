"""The tile plan of the narrow route's one-launch forward (csrc/gadapt_block_plan.h), on the host: the halo rule
(`gadapt_narrow_block_halo_host`) against a brute-force restatement, and the per-tile, per-layer compute ranges the kernel follows
(`gadapt_narrow_block_range_host`: the same arithmetic) - they partition the nodes, stay 32-aligned, and every in-neighbour of a node a
tile computes at layer k + 1 is a node it computed at layer k (layer 0: a row it loaded)."""
import ctypes as C

import pytest
import torch

from g_adaptivity_amd import MeshDataset, MeshGraph, collate, prepare_edge_index, square_mesh
from g_adaptivity_amd import _native
from oracle.pyg_restatement import masked_edge_index

TILE = 512
# (mesh side, batch, the halo the rule gives)
CASES = [(64, 2, 64), (32, 3, 32), (23, 7, 32), (16, 1, 32)]
IDS = ['64x64-b2', '32x32-b3', '23x23-b7', '16x16-b1']


def _csr(mesh_n, batch):
    ds = MeshDataset([mesh_n, mesh_n], batch, seed=0)
    d = collate(ds.samples)
    n = d.x_comp.shape[0]
    g = MeshGraph(masked_edge_index(d, 2, mesh_n), n, 'cpu')
    return g, n, g.rowptr_t.tolist(), g.col_t.tolist()


def _halo(rowptr_t, col_t, n):
    h = C.c_int32(-1)
    assert _native.lib().gadapt_narrow_block_halo_host(rowptr_t.data_ptr(), col_t.data_ptr(), n, C.addressof(h)) == 0
    return h.value


def _rule(rp, cl, n, h):
    """Every row has at most 8 entries and every in-neighbour of i lies in [32 (i // 32) - h, 32 (i // 32) + 32 + h)."""
    return max(rp[i + 1] - rp[i] for i in range(n)) <= 8 and \
        all(32 * (i // 32) - h <= j < 32 * (i // 32) + 32 + h for i in range(n) for j in cl[rp[i]:rp[i + 1]])


def _range(n, h, layers, tile, layer):
    lo, hi = C.c_int64(-1), C.c_int64(-1)
    assert _native.lib().gadapt_narrow_block_range_host(n, h, layers, tile, layer, C.addressof(lo), C.addressof(hi)) == 0
    return lo.value, hi.value


@pytest.mark.parametrize("mesh_n,batch,want", CASES, ids=IDS)
def test_halo_is_the_smallest_that_satisfies_the_rule(mesh_n, batch, want):
    g, n, rp, cl = _csr(mesh_n, batch)
    got = _halo(g.rowptr_t, g.col_t, n)
    brute = next((h for h in (32, 64) if _rule(rp, cl, n, h)), 0)
    assert got == brute == want
    assert max(abs(i - j) for i in range(n) for j in cl[rp[i]:rp[i + 1]]) == mesh_n     # a neighbour sits one mesh row away
    # the graph class registers it for the graphs the wide forward takes (the only ones on the narrow route)
    assert g.narrow_block_halo == (got if (g.wide_deg['t'] > 0 or g.wide_big_deg > 0) else 0)


@pytest.mark.parametrize("mesh_n,batch,want", CASES, ids=IDS)
@pytest.mark.parametrize("layers", [1, 2, 3, 4])
def test_ranges_partition_align_and_nest(mesh_n, batch, want, layers):
    g, n, rp, cl = _csr(mesh_n, batch)
    h = _halo(g.rowptr_t, g.col_t, n)
    n32 = (n + 31) // 32 * 32
    tiles = (n + TILE - 1) // TILE
    owned = [_range(n, h, layers, t, layers - 1) for t in range(tiles)]
    # the last layer's ranges are the owned ranges: consecutive, 512 nodes each, together [0, ceil32(N))
    assert owned[0][0] == 0 and owned[-1][1] == n32
    assert all(owned[t][1] == owned[t + 1][0] for t in range(tiles - 1))
    assert all(hi - lo == TILE for lo, hi in owned[:-1]) and 0 < owned[-1][1] - owned[-1][0] <= TILE
    for t in range(tiles):
        r = [_range(n, h, layers, t, k) for k in range(-1, layers)]     # r[0]: the load range, r[k + 1]: layer k
        for k, (lo, hi) in enumerate(r):
            assert lo % 32 == 0 and hi % 32 == 0 and 0 <= lo < hi <= n32, (t, k - 1, lo, hi)
            w = (layers - k) * h                                         # the owned range widened by (K - 1 - layer) h, clamped
            assert (lo, hi) == (max(0, TILE * t - w), min(n32, TILE * (t + 1) + w))
        for k in range(layers):                                          # what layer k computes needs only what the step before left
            (plo, phi), (lo, hi) = r[k], r[k + 1]
            assert plo <= lo and hi <= phi
            for i in range(lo, min(hi, n)):
                assert all(plo <= j < phi for j in cl[rp[i]:rp[i + 1]]), (t, k, i)
                assert plo <= i < phi
    # the kernel's frame: the load range rounded out to 64-node blocks never exceeds 1024 rows
    assert TILE + 2 * ((layers * h + 63) // 64 * 64) <= 1024


def test_ineligible_graphs_report_zero():
    """A 64 x 64 mesh whose nodes are numbered at random, and a 129-wide mesh, have in-neighbours further than 64 nodes away."""
    m = square_mesh(64)
    d = collate([m]); d.corner_nodes = [m.corner_nodes]
    ei = prepare_edge_index(d, 2, 64, True, False, 64 * 64)
    g = MeshGraph(ei, 64 * 64, 'cpu')
    assert _halo(g.rowptr_t, g.col_t, 64 * 64) == 64
    perm = torch.randperm(64 * 64, generator=torch.Generator().manual_seed(3))
    gp = MeshGraph(perm[ei], 64 * 64, 'cpu')
    assert _halo(gp.rowptr_t, gp.col_t, 64 * 64) == 0
    assert not _rule(gp.rowptr_t.tolist(), gp.col_t.tolist(), 64 * 64, 64)
    m = square_mesh(129)
    d = collate([m]); d.corner_nodes = [m.corner_nodes]
    gw = MeshGraph(prepare_edge_index(d, 2, 129, True, False, 129 * 129), 129 * 129, 'cpu')
    assert _halo(gw.rowptr_t, gw.col_t, 129 * 129) == 0


def test_bad_arguments_are_refused():
    lib = _native.lib()
    lo, hi = C.c_int64(0), C.c_int64(0)
    for args in ((0, 64, 4, 0, 0), (1000, 48, 4, 0, 0), (1000, 64, 5, 0, 0), (1000, 64, 4, 2, 0), (1000, 64, 4, 0, 4), (1000, 64, 4, 0, -2)):
        assert lib.gadapt_narrow_block_range_host(*args, C.addressof(lo), C.addressof(hi)) == -1, args
    assert lib.gadapt_narrow_block_halo_host(None, None, 10, None) == -1
    # registration: halo 0, 32 or 64 on a graph with its ELL copy; an unregistered graph answers 0
    g = MeshGraph(torch.tensor([[0, 1], [1, 0]]), 2, 'cpu')
    assert lib.gadapt_narrow_block_register(g.c_ref, 48) == -1 and b'narrow_block_register' in lib.gadapt_last_error()
    assert lib.gadapt_narrow_block_register(None, 32) == -1
    assert lib.gadapt_narrow_block_halo(g.c_ref, 64) == (g.narrow_block_halo if g.narrow_route(64) else 0)
    assert lib.gadapt_narrow_block_register(g.c_ref, 0) == 0                   # forgotten: one launch per layer
    assert lib.gadapt_narrow_block_halo(g.c_ref, 64) == 0 and lib.gadapt_narrow_block_halo(None, 64) == 0
    assert lib.gadapt_narrow_block_halo(g.c_ref, 32) == 0                      # hidden 64 only
