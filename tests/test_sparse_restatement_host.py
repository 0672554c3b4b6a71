"""CPU: what tests/test_gpu_sparse_primitives.py assumes, proved without a kernel.

1. every case of tests/sparse_graphs.py is what its record claims (recounted from the library's CSR);
2. the restated target- and source-CSR orders are `eid_t` / `perm_s` of `MeshGraph(..., 'cpu')`;
3. an fp32 evaluation slot by slot in CSR order meets every bar of tests/sparse_restatement.py against the fp64 reference;
4. each planted fault, put into a copy of the fp64 reference, leaves the elementwise bar in the case named for it.
Every figure is printed as `[sparse-host] ...` before it is asserted (docs/measurements.md, "Message-passing primitives against fp64")."""
import pytest
import torch

import sparse_graphs as G
import sparse_restatement as R
from sparse_restatement import F32, F64

DISTINCT = [(name, c) for name in G.GRAPHS for c in ((4, 8, 16, 32, 64, 128, 256, 516) if name.startswith('block_edge') else (4,))]
_orders = {}


def orders(name, c):
    key = repr(G.case(name, c))
    if key not in _orders:
        _orders[key] = R.graph_orders(*G.case(name, c))
    return _orders[key]


def on_edges(name, c):
    """(ei, n, inputs) of one (case, width)."""
    ei, n = G.case(name, c)
    return ei, n, G.inputs(name, c)


# ------------------------------------------------------------------------------------------------------ 1. the cases
@pytest.mark.parametrize("name,c", DISTINCT)
def test_case_is_what_its_record_claims(name, c):
    case = G.case(name, c)
    ei, n = case
    eid_t, perm_s, rowptr_t, rowptr_s = orders(name, c)
    in_len, out_len = rowptr_t[1:] - rowptr_t[:-1], rowptr_s[1:] - rowptr_s[:-1]
    hist = {int(v): int(k) for v, k in zip(*torch.unique(in_len, return_counts=True))}
    claims = case.claims
    assert hist == claims['row_lengths'], (hist, claims['row_lengths'])
    assert int(out_len[-1]) == claims['last_out_degree']
    pairs = set()
    dup = loops = 0
    for j, i in ei.t().tolist():
        dup += (j, i) in pairs
        loops += j == i
        pairs.add((j, i))
    assert dup == claims['duplicates'] and loops == claims['self_loops'], (dup, loops, claims)
    for row in claims.get('empty_rows', ()):
        assert int(in_len[row]) == 0
    if 'threads_past_512' in claims:                                # block_edge: n LPN against two full workgroups, long last rows
        d = int(name[len('block_edge'):])
        assert n * G.lanes(c) - 512 == claims['threads_past_512'] == d * G.lanes(c)
        assert int(in_len[-1]) == int(out_len[-1]) == 17 == claims['last_in_degree']
    if name == 'rows0to9':                                          # odd and even tails of the two-in-flight loop, 0 .. 3 and above
        assert set(range(10)) == set(hist) and dup > 0 and loops > 0
    if name == 'long5':
        assert hist == {0: 3, 1: 1, 700: 1} and int(in_len[0]) == 700 and int(in_len[4]) == 1 and n * 8 < 64
    if name == 'empty130':
        assert ei.shape[1] == 0 and n == 130
    if name == 'one3':
        assert n == 1 and ei.tolist() == [[0, 0, 0], [0, 0, 0]]


def test_widths_cover_every_lane_group():
    """Every LPN = 1 .. 64 at c4 == LPN, and a width one chunk past every c4 == LPN (it lands on the next LPN; at 64: a second trip
    for member 0 only); c4 == 129: three trips for member 0."""
    by_lanes = {}
    for c in G.WIDTHS:
        by_lanes.setdefault(G.lanes(c), []).append(G.chunks(c))
    assert sorted(by_lanes) == [1, 2, 4, 8, 16, 32, 64]
    assert all(l in by_lanes[l] for l in by_lanes)
    assert {3, 5, 9, 17, 33, 65, 129} <= {G.chunks(c) for c in G.WIDTHS}
    assert sorted({G.lanes(c) for c in G.EDGE_VEC_WIDTHS}) == [1, 2, 4, 8, 16, 32, 64]


# ----------------------------------------------------------------------------------------------------- 2. the orders
@pytest.mark.parametrize("name,c", DISTINCT)
def test_restated_csr_orders_are_the_library_s(name, c):
    ei, n = G.case(name, c)
    mine, lib = R.csr_orders(ei, n), orders(name, c)
    for a, b, what in zip(mine, lib, ('eid_t', 'perm_s', 'rowptr_t', 'rowptr_s')):
        assert torch.equal(a, b), what
    eid_t, perm_s = mine[0], mine[1]
    assert torch.equal(ei[1][eid_t], torch.sort(ei[1]).values) and torch.equal(ei[0][eid_t][perm_s], torch.sort(ei[0]).values)
    same_row = ei[1][eid_t][1:] == ei[1][eid_t][:-1]
    assert bool((eid_t[1:] > eid_t[:-1])[same_row].all())           # stable: the caller's order within a row
    same_src = ei[0][eid_t][perm_s][1:] == ei[0][eid_t][perm_s][:-1]
    assert bool((perm_s[1:] > perm_s[:-1])[same_src].all())         # stable: target slots ascend within a source row


def test_perturbed_softmax_without_a_seed_is_pyg_softmax():
    for name in ('hub300', 'rows0to9', 'long5', 'one3'):
        ei, n, inp = on_edges(name, 4)
        for dtype in (F32, F64):
            assert torch.equal(R.edge_softmax_perturbed(ei, n, inp['scores'], None, dtype), R.edge_softmax(ei, n, inp['scores'], dtype))


# -------------------------------------------------------------------------------------- 3. fp32 in CSR order meets every bar
def _say(op, name, c, ratio):
    print(f"[sparse-host] {op} {name} C={c} {ratio:.4f}")
    return ratio


@pytest.mark.parametrize("c", G.WIDTHS)
@pytest.mark.parametrize("name", G.GRAPHS)
def test_fp32_evaluation_meets_the_width_bars(name, c):
    ei, n, inp = on_edges(name, c)
    od = orders(name, c)
    x, a, b, w = inp['x'], inp['a'], inp['b'], inp['w']
    worst = {}
    for transpose in (False, True):
        for wt in (w, None):
            for self_scale in (0.0, -1.0, 0.5):
                got = R.spmm_f32(ei, n, od, wt, x, transpose, self_scale)
                key = f"spmm{'_t' if transpose else ''}"
                worst[key] = max(worst.get(key, 0.0), R.spmm_ratio(got, ei, n, wt, x, transpose, self_scale))
                assert R.empty_rows_exact(got, ei, n, x, transpose, self_scale)
    worst['sddmm'] = R.sddmm_ratio(torch.tensor(0.37, dtype=F32) * (a[ei[1]] * b[ei[0]]).sum(-1), ei, a, b, 0.37)
    if c % 4 == 0:
        bv = inp['bvec']
        worst['edge_node_dot'] = R.edge_node_dot_ratio((a[ei[1]] * bv).sum(-1), ei, a, bv)
        worst['edge_weighted_rowsum'] = R.edge_weighted_rowsum_ratio(R.edge_weighted_rowsum_f32(ei, n, od, w, bv), ei, n, w, bv)
        assert torch.equal(w.unsqueeze(-1) * a[ei[1]], R.edge_scale_gather(ei, w, a, F32))
    for op, ratio in worst.items():
        _say(op, name, c, ratio)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("name", G.GRAPHS)
def test_fp32_evaluation_meets_the_per_edge_scalar_bars(name):
    ei, n, inp = on_edges(name, 4)
    od = orders(name, 4)
    worst = {}
    for by_source in (False, True):
        got = R.edge_rowsum_f32(ei, n, od, inp['vals'], by_source)
        worst[f"edge_rowsum{'_s' if by_source else ''}"] = R.edge_rowsum_ratio(got, ei, n, inp['vals'], by_source)
    alpha = R.edge_softmax_f32(ei, n, od, inp['scores'])
    worst['edge_softmax'] = R.edge_softmax_ratio(alpha, ei, n, inp['scores'])
    worst['edge_softmax_backward'] = R.edge_softmax_backward_ratio(
        R.edge_softmax_backward_f32(ei, n, od, alpha, inp['g_edge']), ei, n, alpha, inp['g_edge'])
    for op, ratio in worst.items():
        _say(op, name, 4, ratio)
    assert max(worst.values()) <= 1.0, worst


def test_softmax_exact_cases_in_fp32():
    """One-entry rows give exactly 1, rows of L equal scores exactly fl(1 / L): expf(0) = 1, the sum is exact, 1e-16 vanishes."""
    ei, n = G.case('rows0to9')
    od = orders('rows0to9', 4)
    length = torch.bincount(ei[1], minlength=n)
    equal = torch.full((ei.shape[1],), 1.7, dtype=F32)
    for alpha in (R.edge_softmax_f32(ei, n, od, equal), R.edge_softmax(ei, n, equal, F32)):
        assert torch.equal(alpha, (torch.tensor(1.0, dtype=F32) / length.to(F32))[ei[1]])
    ei, n, inp = on_edges('long5', 4)
    alpha = R.edge_softmax_f32(ei, n, orders('long5', 4), inp['scores'])
    assert float(alpha[ei[1] == 4]) == 1.0


# ------------------------------------------------------------------------------------------------ 4. the bars have teeth
def _caught(fault, name, c, ratio):
    print(f"[sparse-host] fault '{fault}' {name} C={c}: error / bound {ratio:.3g} {'caught' if ratio > 1.0 else 'MISSED'}")
    assert ratio > 1.0, (fault, name, c, ratio)


def _odd_tail_slots(od, transpose):
    """Caller's edge ids of the last slot of every odd-length row of the orientation."""
    eid_t, perm_s, rowptr_t, rowptr_s = od
    rowptr, emap = (rowptr_s, eid_t[perm_s]) if transpose else (rowptr_t, eid_t)
    length = rowptr[1:] - rowptr[:-1]
    return emap[rowptr[1:][length % 2 == 1] - 1]


@pytest.mark.parametrize("c", [4, 36, 260])
def test_fault_last_slot_of_odd_rows_dropped(c):
    name = 'rows0to9'
    ei, n, inp = on_edges(name, c)
    od = orders(name, c)
    for transpose in (False, True):
        keep = torch.ones(ei.shape[1], dtype=torch.bool)
        keep[_odd_tail_slots(od, transpose)] = False
        for w in (inp['w'], None):
            got = R.spmm(ei[:, keep], n, None if w is None else w[keep], inp['x'], transpose)
            _caught(f"odd tail dropped, spmm{'_t' if transpose else ''}", name, c, R.spmm_ratio(got, ei, n, w, inp['x'], transpose))
        got = R.edge_rowsum(ei[:, keep], n, inp['vals'][keep], transpose)
        _caught(f"odd tail dropped, edge_rowsum{'_s' if transpose else ''}", name, c, R.edge_rowsum_ratio(got, ei, n, inp['vals'], transpose))
    keep = torch.ones(ei.shape[1], dtype=torch.bool)
    keep[_odd_tail_slots(od, False)] = False
    got = R.edge_weighted_rowsum(ei[:, keep], n, inp['w'][keep], inp['bvec'][keep])
    _caught("odd tail dropped, edge_weighted_rowsum", name, c, R.edge_weighted_rowsum_ratio(got, ei, n, inp['w'], inp['bvec']))


@pytest.mark.parametrize("c", [260, 516])
@pytest.mark.parametrize("name", ['hub300', 'rows0to9', 'long5', 'block_edge+1', 'one3'])
def test_fault_second_trip_dropped(name, c):
    """The chunks q >= LPN are left out: columns from 4 LPN = 256 on."""
    ei, n, inp = on_edges(name, c)
    cut = 4 * G.lanes(c)
    x, a, b, w, bv = inp['x'], inp['a'], inp['b'], inp['w'], inp['bvec']
    for transpose in (False, True):
        got = R.spmm(ei, n, w, x, transpose)
        got[:, cut:] = 0
        _caught(f"second trip dropped, spmm{'_t' if transpose else ''}", name, c, R.spmm_ratio(got, ei, n, w, x, transpose))
    _caught("second trip dropped, sddmm", name, c, R.sddmm_ratio(R.sddmm(ei, a[:, :cut], b[:, :cut], 0.37), ei, a, b, 0.37))
    _caught("second trip dropped, edge_node_dot", name, c, R.edge_node_dot_ratio(R.edge_node_dot(ei, a[:, :cut], bv[:, :cut]), ei, a, bv))
    got = R.edge_weighted_rowsum(ei, n, w, bv)
    got[:, cut:] = 0
    _caught("second trip dropped, edge_weighted_rowsum", name, c, R.edge_weighted_rowsum_ratio(got, ei, n, w, bv))
    got = R.edge_scale_gather(ei, w, a)
    got[:, cut:] = 0
    assert not torch.equal(got.float(), R.edge_scale_gather(ei, w, a, F32))


@pytest.mark.parametrize("c", G.WIDTHS)
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_fault_last_row_left_at_zero(c, d):
    name = f'block_edge{d:+d}'
    ei, n, inp = on_edges(name, c)
    x, a, b, w = inp['x'], inp['a'], inp['b'], inp['w']
    for transpose in (False, True):
        got = R.spmm(ei, n, w, x, transpose)
        got[-1] = 0
        _caught(f"last row zero, spmm{'_t' if transpose else ''}", name, c, R.spmm_ratio(got, ei, n, w, x, transpose))
        got = R.edge_rowsum(ei, n, inp['vals'], transpose)
        got[-1] = 0
        _caught(f"last row zero, edge_rowsum{'_s' if transpose else ''}", name, c, R.edge_rowsum_ratio(got, ei, n, inp['vals'], transpose))
    last = ei[1] == n - 1
    got = R.sddmm(ei, a, b, 0.37)
    got[last] = 0
    _caught("last row zero, sddmm", name, c, R.sddmm_ratio(got, ei, a, b, 0.37))
    got = R.edge_softmax(ei, n, inp['scores'])
    got[last] = 0
    _caught("last row zero, edge_softmax", name, c, R.edge_softmax_ratio(got, ei, n, inp['scores']))
    if c % 4 == 0:
        got = R.edge_weighted_rowsum(ei, n, w, inp['bvec'])
        got[-1] = 0
        _caught("last row zero, edge_weighted_rowsum", name, c, R.edge_weighted_rowsum_ratio(got, ei, n, w, inp['bvec']))
        got = R.edge_node_dot(ei, a, inp['bvec'])
        got[last] = 0
        _caught("last row zero, edge_node_dot", name, c, R.edge_node_dot_ratio(got, ei, a, inp['bvec']))


@pytest.mark.parametrize("name", ['rows0to9', 'long5'])
def test_fault_identity_in_place_of_perm_s(name):
    """The transposed products read the weight of source-CSR slot e at target slot e, not at perm_s[e] - everywhere, and then on the
    slots of duplicate edges only (their weights differ: the fault must show there too)."""
    c = 8
    ei, n, inp = on_edges(name, c)
    eid_t, perm_s, _, _ = orders(name, c)
    w_t = inp['w'][eid_t]                                           # weights in target-CSR order, as the library holds them
    key = ei[0] * n + ei[1]
    uniq, counts = torch.unique(key, return_counts=True)
    dup_edge = torch.isin(key, uniq[counts > 1])                    # caller's edges whose (source, target) pair occurs more than once
    assert bool(dup_edge.any())
    for only_dups in (False, True):
        slot_is_dup = dup_edge[eid_t[perm_s]]
        wrong_t = torch.where(slot_is_dup | (not only_dups), w_t, w_t[perm_s])      # value read at source-CSR slot e
        moved = wrong_t != w_t[perm_s]
        assert bool((moved & slot_is_dup).any())                    # a duplicate edge gets another weight than its own
        w_caller = torch.empty_like(w_t)
        w_caller[eid_t[perm_s]] = wrong_t                           # the same fault, told in the caller's edge order
        tag = "identity for perm_s" + (" on duplicate edges" if only_dups else "")
        _caught(tag + ", spmm_t", name, c, R.spmm_ratio(R.spmm(ei, n, w_caller, inp['x'], True), ei, n, inp['w'], inp['x'], True))
        _caught(tag + ", edge_rowsum_s", name, c, R.edge_rowsum_ratio(R.edge_rowsum(ei, n, w_caller, True), ei, n, inp['w'], True))


NO_LAST_MEMBER_CHUNK = tuple(c for c in G.WIDTHS if G.chunks(c) < G.lanes(c))      # 12, 20, 36, 68, 132: member LPN - 1 owns no chunk


@pytest.mark.parametrize("c", G.WIDTHS)
@pytest.mark.parametrize("name", ['hub300', 'rows0to9'])
def test_fault_last_member_left_out_of_the_dot_product(name, c):
    """Member LPN - 1 of a lane group owns the chunks q = LPN - 1 (mod LPN).  Where c4 < LPN it owns none and the fault changes
    nothing; everywhere else it must be caught."""
    ei, n, inp = on_edges(name, c)
    l, c4 = G.lanes(c), G.chunks(c)
    pad = lambda t: torch.nn.functional.pad(t, (0, 4 * c4 - c))    # noqa: E731
    keep = (torch.arange(4 * c4) // 4) % l != l - 1
    a, b = inp['a'], inp['b']
    got = R.sddmm(ei, pad(a)[:, keep], pad(b)[:, keep], 0.37)
    if c in NO_LAST_MEMBER_CHUNK:
        assert bool(keep.all()) and torch.equal(got, R.sddmm(ei, a, b, 0.37))
        return
    _caught("member LPN - 1 left out, sddmm", name, c, R.sddmm_ratio(got, ei, a, b, 0.37))
    if c % 4 == 0:
        got = R.edge_node_dot(ei, a[:, keep], inp['bvec'][:, keep])
        _caught("member LPN - 1 left out, edge_node_dot", name, c, R.edge_node_dot_ratio(got, ei, a, inp['bvec']))


@pytest.mark.parametrize("name", ['hub300', 'rows0to9', 'long5', 'block_edge+1'])
def test_fault_softmax_over_rows_shifted_by_one_slot(name):
    ei, n, inp = on_edges(name, 4)
    eid_t = orders(name, 4)[0]
    dst_t = ei[1][eid_t]
    shifted = torch.cat([dst_t[1:], dst_t[-1:]])                    # slot e is normalised with the row of slot e + 1
    got = torch.empty(ei.shape[1], dtype=F64)
    got[eid_t] = R.edge_softmax(torch.stack([ei[0][eid_t], shifted]), n, inp['scores'][eid_t])
    _caught("softmax rows shifted by one slot", name, 4, R.edge_softmax_ratio(got, ei, n, inp['scores']))
    alpha = R.edge_softmax(ei, n, inp['scores'], F32)
    got[eid_t] = R.edge_softmax_backward(torch.stack([ei[0][eid_t], shifted]), n, alpha[eid_t], inp['g_edge'][eid_t])
    _caught("softmax backward rows shifted by one slot", name, 4, R.edge_softmax_backward_ratio(got, ei, n, alpha, inp['g_edge']))
