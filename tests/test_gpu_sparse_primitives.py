"""The message-passing primitives (csrc/gadapt_sparse.inc behind g_adaptivity_amd/sparse_ops.py) against fp64 at lane-group edges.

Every operation runs through the public functions of `sparse_ops` (and `_spmm_raw` / `_sddmm_raw` for `self_scale` and `scale`, which
nothing public reaches) on the graphs of tests/sparse_graphs.py at the widths C = 1 .. 516 that instantiate every LPN = 1 .. 64 at
c4 == LPN and one chunk past it, and is compared ELEMENTWISE with the fp64 restatement of tests/sparse_restatement.py under the bars
derived there (none is fitted; tests/test_sparse_restatement_host.py shows on the CPU that an fp32 evaluation in CSR order meets them
and that each planted fault leaves them).  The autograd wrappers run with a seeded upstream gradient, so that each transposed
product (dx, db, du) is compared as the primitive it is, with the out-degree as its row length.  Per-edge arrays go to the library
in target-CSR order (`eid_t`) and come back to the caller's order for the comparison.

Every test prints `[sparse] operation case C=width error/bound` before it asserts (docs/measurements.md, "Message-passing
primitives against fp64")."""
import functools
import math

import pytest
import torch

import sparse_graphs as G
import sparse_restatement as R
from g_adaptivity_amd import MeshGraph
from g_adaptivity_amd import sparse_ops as Sp
from helpers import rel_err
from sparse_restatement import F32, F64, U, gamma

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]
SCALE = 0.37
PER_CASE = pytest.mark.parametrize("name,c", [(name, c) for name in G.GRAPHS for c in G.WIDTHS])


@functools.lru_cache(maxsize=None)
def _device_graph(key, dev):
    name, c = key
    ei, n = G.case(name, c)
    graph = MeshGraph(ei, n, dev)
    return graph, graph.eid_t[:ei.shape[1]].long().cpu()


class On:
    """One (case, width) on the device: the graph, its inputs, and the two edge orders."""

    def __init__(self, name, c, dev):
        self.name, self.c, self.dev = name, c, dev
        self.case = G.case(name, c)
        self.ei, self.n = self.case
        self.graph, self.order = _device_graph((name, c if name.startswith('block_edge') else 4), dev)   # only block_edge depends on C
        self.inp = G.inputs(name, c)

    def node(self, t):
        return t.to(self.dev)

    def edge(self, t):
        """caller's edge order (CPU) -> target-CSR order on the device"""
        return t[self.order].contiguous().to(self.dev)

    def back(self, t):
        """target-CSR order on the device -> caller's edge order (CPU)"""
        out = torch.empty(t.shape, dtype=t.dtype)
        out[self.order] = t.detach().cpu()
        return out

    def judge(self, figures):
        for op, ratio in figures.items():
            print(f"[sparse] {op} {self.name} C={self.c} {ratio:.4f}")
        bad = {op: ratio for op, ratio in figures.items() if not ratio <= 1.0}
        assert not bad, (self.name, self.c, bad)


def _twice(fn):
    """The result of `fn()`, asserted bit-equal to a second call."""
    first, second = fn(), fn()
    torch.cuda.synchronize()
    assert torch.equal(first, second)
    return first


def _zero_padded(t):
    return torch.nn.functional.pad(t, (0, -t.shape[1] % 4)).contiguous()


# ----------------------------------------------------------------------------------------------------------------- spmm
@PER_CASE
def test_spmm_both_orientations_and_self_scale(gpu_device, name, c):
    on = On(name, c, gpu_device)
    ei, n, graph = on.ei, on.n, on.graph
    x, w, g = on.inp['x'], on.inp['w'], on.inp['g_node']
    xd, wd, gd = on.node(x), on.edge(w), on.node(g)
    fig = {}
    for transpose in (False, True):
        for wt, wtd in ((w, wd), (None, None)):
            for self_scale in (0.0, -1.0, 0.5):
                got = _twice(lambda: Sp._spmm_raw(graph, wtd, xd, transpose, self_scale))
                key = f"spmm{'_t' if transpose else ''}{'' if self_scale == 0.0 else '+self'}"
                fig[key] = max(fig.get(key, 0.0), R.spmm_ratio(got, ei, n, wt, x, transpose, self_scale))
                assert R.empty_rows_exact(got, ei, n, x, transpose, self_scale), (key, 'empty rows')
                if c % 4:                                           # same bits as the data zero-padded by hand
                    assert torch.equal(Sp._spmm_raw(graph, wtd, _zero_padded(xd), transpose, self_scale)[:, :c], got)
    # the public function and its autograd: dx is the transposed product, dw an sddmm
    wr, xr = wd.clone().requires_grad_(True), xd.clone().requires_grad_(True)
    out = Sp.spmm(graph, wr, xr)
    assert torch.equal(out.detach(), Sp._spmm_raw(graph, wd, xd, False))
    dw, dx = torch.autograd.grad(out, (wr, xr), gd)
    fig['spmm dx (transposed)'] = R.spmm_ratio(dx, ei, n, w, g, True)
    fig['spmm dw (sddmm)'] = R.sddmm_ratio(on.back(dw), ei, g, x)
    plain = Sp.spmm(graph, None, xr)
    fig['spmm plain dx (transposed)'] = R.spmm_ratio(torch.autograd.grad(plain, xr, gd)[0], ei, n, None, g, True)
    on.judge(fig)


# ---------------------------------------------------------------------------------------------------------------- sddmm
@PER_CASE
def test_sddmm_scale_and_transposed_backward(gpu_device, name, c):
    on = On(name, c, gpu_device)
    ei, n, graph = on.ei, on.n, on.graph
    a, b, ge = on.inp['a'], on.inp['b'], on.inp['g_edge']
    ad, bd, ged = on.node(a), on.node(b), on.edge(ge)
    fig = {}
    got = _twice(lambda: Sp._sddmm_raw(graph, ad, bd, SCALE))
    fig['sddmm scale'] = R.sddmm_ratio(on.back(got), ei, a, b, SCALE)
    if c % 4:
        assert torch.equal(Sp._sddmm_raw(graph, _zero_padded(ad), _zero_padded(bd), SCALE), got)
    ar, br = ad.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    s = _twice(lambda: Sp.sddmm(graph, ar, br))
    fig['sddmm'] = R.sddmm_ratio(on.back(s), ei, a, b)
    da, db = torch.autograd.grad(s, (ar, br), ged)
    fig['sddmm da (spmm)'] = R.spmm_ratio(da, ei, n, ge, b, False)
    fig['sddmm db (transposed)'] = R.spmm_ratio(db, ei, n, ge, a, True)
    if c == 260:                                                    # the second trip, against the graph's own width siblings
        parts = Sp._sddmm_raw(graph, ad[:, :256].contiguous(), bd[:, :256].contiguous(), SCALE) \
            + Sp._sddmm_raw(graph, ad[:, 256:].contiguous(), bd[:, 256:].contiguous(), SCALE)
        fig['sddmm 260 = 256 + 4'] = R.sddmm_ratio(on.back(parts), ei, a, b, SCALE)   # one more summation order of the same 260 products
    on.judge(fig)


# ------------------------------------------------------------------------------------------------- per-edge vectors
@PER_CASE
def test_edge_vector_modes(gpu_device, name, c):
    on = On(name, c, gpu_device)
    ei, n, graph = on.ei, on.n, on.graph
    a, w, bv, ge, gn = (on.inp[k] for k in ('a', 'w', 'bvec', 'g_edge', 'g_node'))
    ad, wd, bvd, ged, gnd = on.node(a), on.edge(w), on.edge(bv), on.edge(ge), on.node(gn)
    if c % 4:                                                       # these operations take no padding: they refuse the width
        with pytest.raises(ValueError):
            Sp.edge_node_dot(graph, ad, bvd)
        with pytest.raises(ValueError):
            Sp.edge_weighted_rowsum(graph, wd, bvd)
        return
    fig = {}
    ar, bvr, wr = ad.clone().requires_grad_(True), bvd.clone().requires_grad_(True), wd.clone().requires_grad_(True)
    s = _twice(lambda: Sp.edge_node_dot(graph, ar, bvr))                                   # mode 0
    fig['edge_node_dot'] = R.edge_node_dot_ratio(on.back(s), ei, a, bv)
    da, db = torch.autograd.grad(s, (ar, bvr), ged)                                        # modes 1 and 2
    fig['edge_node_dot da (mode 1)'] = R.edge_weighted_rowsum_ratio(da, ei, n, ge, bv)
    assert torch.equal(on.back(db), R.edge_scale_gather(ei, ge, a, F32)), 'edge_node_dot db (mode 2)'
    out = _twice(lambda: Sp.edge_weighted_rowsum(graph, wr, bvr))                          # mode 1
    fig['edge_weighted_rowsum'] = R.edge_weighted_rowsum_ratio(out, ei, n, w, bv)
    dw, db = torch.autograd.grad(out, (wr, bvr), gnd)                                      # modes 0 and 2
    fig['edge_weighted_rowsum dw (mode 0)'] = R.edge_node_dot_ratio(on.back(dw), ei, gn, bv)
    assert torch.equal(on.back(db), R.edge_scale_gather(ei, w, gn, F32)), 'edge_weighted_rowsum db (mode 2)'
    gather = _twice(lambda: Sp._edge_vec_raw(graph, 2, wd, ad, None, c))                   # mode 2 as an operation of its own
    assert torch.equal(on.back(gather), R.edge_scale_gather(ei, w, a, F32)), 'edge_scale_gather'
    fig['edge_scale_gather (bit-equal)'] = 0.0
    on.judge(fig)


# ------------------------------------------------------------------------------------------------- per-edge scalars
@pytest.mark.parametrize("name", G.GRAPHS)
def test_edge_softmax_combine_rowsum(gpu_device, name):
    on = On(name, 4, gpu_device)                                    # one lane per row: block_edge has 511, 512 and 513 nodes here
    ei, n, graph = on.ei, on.n, on.graph
    sc, vals, ge, u, v = (on.inp[k] for k in ('scores', 'vals', 'g_edge', 'u', 'v'))
    fig = {}
    sr = on.edge(sc).requires_grad_(True)
    alpha = _twice(lambda: Sp.edge_softmax(graph, sr))
    fig['edge_softmax'] = R.edge_softmax_ratio(on.back(alpha), ei, n, sc)
    ds = _twice(lambda: torch.autograd.grad(alpha, sr, on.edge(ge), retain_graph=True)[0])
    fig['edge_softmax backward'] = R.edge_softmax_backward_ratio(on.back(ds), ei, n, on.back(alpha), ge)   # from the alpha returned
    one_entry = (torch.bincount(ei[1], minlength=n) == 1)[ei[1]]
    assert bool((on.back(alpha)[one_entry] == 1.0).all())
    ur, vr = on.node(u).requires_grad_(True), on.node(v).requires_grad_(True)
    add, mul = _twice(lambda: Sp.edge_add(graph, ur, vr)), _twice(lambda: Sp.edge_mul(graph, ur, vr))
    assert torch.equal(on.back(add), R.edge_add(ei, u, v, F32)) and torch.equal(on.back(mul), R.edge_mul(ei, u, v, F32))
    fig['edge_add, edge_mul (bit-equal)'] = 0.0
    for by_source in (False, True):
        got = _twice(lambda: Sp._rowsum(graph, on.edge(vals), by_source))
        fig[f"edge_rowsum{' by source' if by_source else ''}"] = R.edge_rowsum_ratio(got, ei, n, vals, by_source)
    du, dv = torch.autograd.grad(add, (ur, vr), on.edge(ge))
    fig['edge_add du (rowsum by source)'] = R.edge_rowsum_ratio(du, ei, n, ge, True)
    fig['edge_add dv (rowsum)'] = R.edge_rowsum_ratio(dv, ei, n, ge, False)
    du, dv = torch.autograd.grad(mul, (ur, vr), on.edge(ge))       # the rowsum of the fp32 products g_e v_i / g_e u_j
    fig['edge_mul du (rowsum by source)'] = R.edge_rowsum_ratio(du, ei, n, ge * v[ei[1]], True)
    fig['edge_mul dv (rowsum)'] = R.edge_rowsum_ratio(dv, ei, n, ge * u[ei[0]], False)
    on.judge(fig)


def test_edge_softmax_exact_cases(gpu_device):
    """Rows of L equal scores give exactly fl(1 / L) in every slot (expf(0) = 1, the sum is exact, 1e-16 vanishes against L: this
    fails if the division is ever replaced by a reciprocal approximation); the hub row of `test_edge_softmax_and_edge_combine` with
    scores spread over +-40 is finite and sums to 1 within (L + 4) u + 4 noise_row."""
    for name in ('rows0to9', 'hub300', 'long5', 'one3', 'block_edge+1'):
        on = On(name, 4, gpu_device)
        length = torch.bincount(on.ei[1], minlength=on.n)
        alpha = Sp.edge_softmax(on.graph, torch.full((on.ei.shape[1],), 1.7, device=gpu_device))
        assert torch.equal(on.back(alpha), (torch.tensor(1.0, dtype=F32) / length.to(F32))[on.ei[1]]), name
    ei, n = G.hub300(4)
    graph = MeshGraph(ei, n, gpu_device)
    order = graph.eid_t.long().cpu()
    gen = torch.Generator().manual_seed(0)
    s = (torch.randn(ei.shape[1], generator=gen, dtype=F64) * 3)
    hub = ei[1] == 9
    s[hub] += torch.linspace(-40, 40, int(hub.sum()), dtype=F64)
    s = s.float()
    alpha = torch.empty_like(s)
    alpha[order] = Sp.edge_softmax(graph, s[order].to(gpu_device)).cpu()
    a64, bar = R.edge_softmax_bar(ei, n, s)
    ratio = R.worst_ratio(alpha, a64, bar)
    length, row_sum = int(hub.sum()), float(alpha[hub].double().sum())
    allowed = (length + 4) * U + 4 * float(R.edge_softmax_noise(ei, n, s)[9])
    print(f"[sparse] edge_softmax hub300(seed 4) wide-scores {ratio:.4f}; hub row of {length}: |sum - 1| = {abs(row_sum - 1):.3e}, allowed {allowed:.3e}")
    assert bool(torch.isfinite(alpha).all()) and ratio <= 1.0
    assert abs(row_sum - 1) <= allowed


# ---------------------------------------------------------------------------------------------------------- padding
@pytest.mark.parametrize("c", [1, 3, 10, 100])
@pytest.mark.parametrize("name", ['hub300', 'rows0to9'])
def test_padded_widths_equal_hand_padding(gpu_device, name, c):
    on = On(name, c, gpu_device)
    xd, ad, bd, wd = on.node(on.inp['x']), on.node(on.inp['a']), on.node(on.inp['b']), on.edge(on.inp['w'])
    for transpose in (False, True):
        got = Sp._spmm_raw(on.graph, wd, xd, transpose, 0.5)
        assert got.shape == (on.n, c) and torch.equal(Sp._spmm_raw(on.graph, wd, _zero_padded(xd), transpose, 0.5)[:, :c], got)
    assert torch.equal(Sp._sddmm_raw(on.graph, ad, bd, SCALE), Sp._sddmm_raw(on.graph, _zero_padded(ad), _zero_padded(bd), SCALE))
    on.judge({'spmm': R.spmm_ratio(Sp._spmm_raw(on.graph, wd, xd, False), on.ei, on.n, on.inp['w'], on.inp['x']),
              'sddmm': R.sddmm_ratio(on.back(Sp._sddmm_raw(on.graph, ad, bd, SCALE)), on.ei, on.inp['a'], on.inp['b'], SCALE)})


# -------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("c", G.ATTENTION_WIDTHS)
@pytest.mark.parametrize("name", ['hub300', 'rows0to9'])
def test_attention_aggregate_tensor_scale_and_edge_weight(gpu_device, name, c):
    """`attention_aggregate` stage by stage - scores under the sddmm bar (two more roundings: the scale and the edge weight), the
    attention under the softmax bar from the fp32 scores it was given, the output under the spmm bar from the fp32 attention it
    returned - then the whole chain and dq, dk, dv normwise at 5e-6 against fp64 autograd of the restatement."""
    on = On(name, c, gpu_device)
    ei, n, graph = on.ei, on.n, on.graph
    q, k, v, gn, ge = (on.inp[key] for key in ('a', 'b', 'x', 'g_node', 'g_edge'))
    ew = 1 + 0.25 * on.inp['vals']
    scale = torch.tensor(1 / math.sqrt(c), dtype=F32)
    qd, kd, vd = (on.node(t).requires_grad_(True) for t in (q, k, v))
    scale_d, ew_d = scale.to(gpu_device), on.edge(ew)
    out, alpha = Sp.attention_aggregate(graph, qd, kd, vd, scale_d, ew_d)
    dq, dk, dv = torch.autograd.grad([out, alpha], (qd, kd, vd), [on.node(gn), on.edge(ge)])
    s32 = on.back(Sp.sddmm(graph, qd, kd) * scale_d * ew_d)        # the scores the softmax was given (bit-reproducible)
    fig = {}
    bound, c4 = R.sddmm_bound(ei, q, k, float(scale))
    s64 = R.sddmm(ei, q, k, float(scale)) * ew.double()
    fig['attention scores'] = R.worst_ratio(s32, s64, gamma(c4 + 4) * bound * ew.double().abs())
    fig['attention softmax'] = R.edge_softmax_ratio(on.back(alpha), ei, n, s32)
    fig['attention output'] = R.spmm_ratio(out, ei, n, on.back(alpha), v)
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    a64 = R.edge_softmax(ei, n, R.sddmm(ei, q64, k64, float(scale)) * ew.double())
    out64 = R.spmm(ei, n, a64, v64)
    g64 = torch.autograd.grad([out64, a64], (q64, k64, v64), [gn.double(), ge.double()])
    norm = {'out': rel_err(out, out64)[0], 'alpha': rel_err(on.back(alpha), a64)[0],
            'dq': rel_err(dq, g64[0])[0], 'dk': rel_err(dk, g64[1])[0], 'dv': rel_err(dv, g64[2])[0]}
    for key, val in norm.items():
        print(f"[sparse] attention normwise {key} {name} C={c} {val:.3e} (bar 5e-6)")
    on.judge(fig)
    assert max(norm.values()) <= 5e-6, norm
