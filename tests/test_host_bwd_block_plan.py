"""The plan of the narrow route's one-launch backward below the top layer (csrc/gadapt_block_plan.h, csrc/gadapt_narrow_bwd_block.inc,
DESIGN.md section 5), on the host.  `gadapt_narrow_bwd_block_range_host` is the arithmetic the kernel uses for the nodes a tile runs at
fused stage s of K: the owned ranges partition the nodes, every range is 32-aligned, every OUT-neighbour of a node of stage s + 1 is a
node of stage s, the {alpha dt, ds} pairs a stage leaves the next fit the LDS buffer they are given, and the slab rows a tile writes are
2 t and 2 t + 1.  Then the refusals of the new registration and of the new entry point."""
import ctypes as C

import pytest
import torch

import narrow_graphs as ng
from g_adaptivity_amd import GNN, MeshDataset, MeshGraph, collate, hot_path_opt
from g_adaptivity_amd import _native
from g_adaptivity_amd import graph as graph_mod
from oracle.pyg_restatement import masked_edge_index

TILE = 512


def _range(n, h, K, tile, stage):
    lo, hi, cap = C.c_int64(-1), C.c_int64(-1), C.c_int32(-1)
    assert _native.lib().gadapt_narrow_bwd_block_range_host(n, h, K, tile, stage, C.addressof(lo), C.addressof(hi), C.addressof(cap)) == 0
    return lo.value, hi.value, cap.value


# 1 .. 2199 nodes, and the sizes around the caps: 512 tiles of the forward's loss partials, 131072 nodes of a 512-row slab
SIZES = list(range(1, 2200)) + [TILE * 256 - 1, TILE * 256, TILE * 256 + 1, 131071, 131072, TILE * 512 - 1, TILE * 512]


@pytest.mark.parametrize("halo", [32, 64])
@pytest.mark.parametrize("K", [2, 3])
def test_ranges_partition_align_and_nest(halo, K):
    lib = _native.lib()
    margin = lib.gadapt_narrow_bwd_block_margin_host(halo, K)
    assert margin == ((K - 1) * halo + 63) // 64 * 64 and TILE + 2 * margin <= 768      # the frame the LDS g rows are sized for
    for n in SIZES:
        n32 = (n + 31) // 32 * 32
        tiles = (n + TILE - 1) // TILE
        some = range(tiles) if tiles <= 8 else [0, 1, 2, tiles // 2, tiles - 3, tiles - 2, tiles - 1]
        prev_hi = None
        for t in some:
            r = [_range(n, halo, K, t, s) for s in range(K)]
            for s, (lo, hi, cap) in enumerate(r):
                assert lo % 32 == 0 and hi % 32 == 0 and 0 <= lo < hi <= n32, (n, t, s, lo, hi)
                w = (K - 1 - s) * halo                                   # the owned range widened by (K - 1 - s) h, clamped
                assert (lo, hi) == (max(0, TILE * t - w), min(n32, TILE * (t + 1) + w))
                assert TILE * t - margin <= lo and hi <= TILE * (t + 1) + margin       # inside the frame
                # the pairs stage s - 1 leaves for stage s: at most 8 per row of the range
                assert cap == (0 if s == 0 else 8 * (TILE + (128 if (K == 3 and s == 1) else 0))) and (s == 0 or 8 * (hi - lo) <= cap)
                if s:
                    assert r[s - 1][0] <= lo and hi <= r[s - 1][1]
            lo, hi, _ = r[K - 1]                                         # the last stage's range is the owned range
            assert lo == TILE * t and hi == min(n32, TILE * (t + 1))
            if prev_hi is not None and t == prev_t + 1:
                assert lo == prev_hi
            prev_hi, prev_t = hi, t
        assert _range(n, halo, K, 0, K - 1)[0] == 0 and _range(n, halo, K, tiles - 1, K - 1)[1] == n32
        # slab rows 2 t and 2 t + 1 of every tile lie below the slab's row count wherever a row is one 256-node range (eligibility)
        rows = lib.gadapt_backward_slab_rows(n, 64)
        if n <= 256 * rows:
            assert 2 * (tiles - 1) + 1 < rows, (n, tiles, rows)


def test_groups_of_stages():
    lib = _native.lib()
    def groups(n):
        out, done = [], 0
        while (k := lib.gadapt_narrow_bwd_block_groups_host(n, done)) > 0:
            out.append(k); done += k
        return out
    assert groups(2) == [2] and groups(3) == [3] and groups(4) == [2, 2] and groups(5) == [3, 2] and groups(6) == [3, 3] and groups(7) == [3, 2, 2]
    assert all(sum(groups(n)) == n and min(groups(n)) >= 2 and max(groups(n)) <= 3 for n in range(2, 40))
    assert lib.gadapt_narrow_bwd_block_groups_host(1, 0) == -1 and lib.gadapt_narrow_bwd_block_groups_host(3, -1) == -1


def _nests(g, n, K):
    """Every out-neighbour of a node of stage s + 1 lies in stage s's range; a stage's source-order edge window fits its LDS buffer."""
    h = g.narrow_block_halo_source
    rp, cl = g.rowptr_s.cpu().long(), g.col_s.cpu().long()
    assert int((rp[1:] - rp[:-1]).max()) <= 8
    for t in range((n + TILE - 1) // TILE):
        r = [_range(n, h, K, t, s) for s in range(K)]
        for s in range(1, K):
            (plo, phi, _), (lo, hi, cap) = r[s - 1], r[s]
            e0, e1 = int(rp[min(lo, n)]), int(rp[min(hi, n)])
            assert e1 - e0 <= cap, (t, s)
            if e1 > e0:
                nb = cl[e0:e1]
                assert plo <= int(nb.min()) and int(nb.max()) < min(phi, n), (t, s)


SQUARES = [(16, 1, 32), (23, 7, 32), (32, 3, 32), (64, 2, 64)]


@pytest.mark.parametrize("mesh_n,batch,want", SQUARES, ids=['16x16-b1', '23x23-b7', '32x32-b3', '64x64-b2'])
@pytest.mark.parametrize("K", [2, 3])
def test_out_neighbours_of_a_stage_lie_in_the_stage_before_square_meshes(mesh_n, batch, want, K, monkeypatch):
    monkeypatch.setattr(graph_mod, 'WIDE_MIN_NODES', 0)
    d = collate(MeshDataset([mesh_n, mesh_n], batch, seed=0).samples)
    n = d.x_comp.shape[0]
    g = MeshGraph(masked_edge_index(d, 2, mesh_n), n, 'cpu')
    assert g.narrow_block_halo == want and g.narrow_block_halo_source == want
    _nests(g, n, K)


@pytest.mark.parametrize("case_id", ng.IDS)
def test_out_neighbours_of_a_stage_lie_in_the_stage_before_narrow_graphs(case_id, monkeypatch):
    c = ng.CASES[case_id]
    monkeypatch.setattr(graph_mod, 'WIDE_MIN_NODES', 0)
    if c.half_max is not None:
        monkeypatch.setattr(graph_mod, 'WIDE_HALF_MAX_NODES', c.half_max)
    opt = hot_path_opt(mesh_dims=list(c.dims), hidden_dim=64, num_layers=c.layers, conv_type='GRAND_plus', device='cpu', **c.opt)
    ds = ng.MixedMeshDataset(c.mixed, c.batch, seed=c.seed) if c.mixed else MeshDataset(c.dims, c.batch, seed=c.seed)
    data = collate(ds.samples)
    if c.edits is not None:
        data = c.edits(data)
    torch.manual_seed(c.seed)
    model = GNN(ds, opt)
    n = data.x_comp.shape[0]
    g = model._graph(data, n, torch.device('cpu'))
    assert g.num_nodes == c.nodes
    # the 512-row window has no forward halo, and out-rows beyond 8 have no source halo: those keep the old launches
    if c.big or c.deg_s[1] > 8:
        assert g.narrow_block_halo_source == 0
        return
    assert g.narrow_block_halo_source in (32, 64)
    for K in (2, 3):
        _nests(g, n, K)


def test_bad_arguments_are_refused():
    lib = _native.lib()
    lo, hi = C.c_int64(0), C.c_int64(0)
    for args in ((0, 64, 3, 0, 0), (1000, 48, 3, 0, 0), (1000, 64, 4, 0, 0), (1000, 64, 1, 0, 0), (1000, 64, 3, 2, 0), (1000, 64, 3, 0, 3),
                 (1000, 64, 3, 0, -1)):
        assert lib.gadapt_narrow_bwd_block_range_host(*args, C.addressof(lo), C.addressof(hi), None) == -1, args
    assert lib.gadapt_narrow_bwd_block_range_host(1000, 64, 3, 0, 0, None, C.addressof(hi), None) == -1
    assert lib.gadapt_narrow_bwd_block_margin_host(48, 3) == -1 and lib.gadapt_narrow_bwd_block_margin_host(64, 4) == -1
    # registration of the source halo: 0, 32 or 64 on a graph with the ELL copy of its out-edges
    g = MeshGraph(torch.tensor([[0, 1], [1, 0]]), 2, 'cpu')
    assert lib.gadapt_narrow_block_register_source(g.c_ref, 48) == -1 and b'narrow_block_register_source' in lib.gadapt_last_error()
    assert lib.gadapt_narrow_block_register_source(None, 32) == -1
    assert lib.gadapt_narrow_block_register_source(g.c_ref, 32) == 0 and lib.gadapt_narrow_block_register_source(g.c_ref, 0) == 0
    # the entry point: nowhere to report, null pointers, one conv per layer (the packed slab has one shared conv) - refused before
    # anything is launched, with the report cleared
    ran = C.c_int(7)
    one = torch.zeros(64)
    p = one.data_ptr()
    ok = [g.c_ref, p, 4, p, p, 2, 4, p, 0, p, 0, p, p, p, p, p, None, 0, None, 64, None]
    assert lib.gadapt_block_backward_narrow_packed_block(*ok, 1, None) == -1 and b'block' in lib.gadapt_last_error()
    for k in (1, 3, 4, 7, 9, 11, 12, 13, 14, 15):
        bad = list(ok); bad[k] = None
        ran.value = 7
        assert lib.gadapt_block_backward_narrow_packed_block(*bad, 1, C.addressof(ran)) == -1 and ran.value == 0, k
    per_layer = list(ok); per_layer[8], per_layer[10] = 64 * 64, 64
    assert lib.gadapt_block_backward_narrow_packed_block(*per_layer, 0, C.addressof(ran)) == -1 and ran.value == 0
    assert lib.gadapt_block_backward_narrow_packed_block(None, *ok[1:], 0, C.addressof(ran)) == -1
    assert lib.gadapt_debug_set_narrow_backward_block(0) == 0 and lib.gadapt_debug_set_narrow_backward_block(1) == 0
