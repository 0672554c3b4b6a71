"""The launch sequence of a narrow step as one plan (csrc/gadapt_narrow_plan.h; DESIGN.md "How a message-passing entry point is put
together"), on the host.  `gadapt_narrow_step_plan_host` is the pure function (facts, switches) -> plan that the entry points walk.

(a) `expected` below restates the rules from the sentences of include/gadapt_hip.h ("The launch sequence of a narrow step"), launch
    by launch in the order they run - not from the C++, which indexes a plan by launch number - and the two are compared over
    facts x switches.
(b) Invariants of every plan: what a launch reads the launch before wrote, nothing is read and written in one launch, the buffers lie
    inside the caller's.  One documented exception, stated by the header and by gadapt_narrow_bwd.inc: a FUSED launch keeps dxd in one
    member - row j is read and then written by the one lane that owns node j, no other lane touches it - so for that kind "written is
    not read" is asserted on g and on the pairs only.  A launch that does not write what it reads may also read an input of the launch
    before (the top gradient, the g rows a target pass and its source pass share): that input is intact, by the same invariant.
(c) `gadapt_narrow_step_plan` on CPU graphs equals the pure function fed with the facts read off the graph object.
(d) Refusals of both queries."""
import ctypes as C
import functools
import itertools

import pytest
import torch

import narrow_graphs as ng
from g_adaptivity_amd import GNN, MeshDataset, MeshGraph, collate, hot_path_opt
from g_adaptivity_amd import _native
from g_adaptivity_amd import graph as graph_mod
from oracle.pyg_restatement import masked_edge_index

C_ = 64
HEAD, WORDS = 18, 13
FACTS = ('n_nodes', 'n_edges', 'c', 'n_layers', 'takes', 'halo_t', 'halo_s', 'kmax', 'slab_rows', 'tiles_ok', 'ell_t', 'ell_s', 'tpos_s',
         'rowptr_s', 'col_s', 'shared', 'packed', 'target', 'buffers', 'coeffs', 'top_done', 'may_block')
SHARED, PACKED, TARGET, BUFFERS, COEFFS, TOP_DONE, MAY_BLOCK = 1, 2, 4, 8, 16, 32, 64
FLAG_OF = dict(shared=SHARED, packed=PACKED, target=TARGET, buffers=BUFFERS, coeffs=COEFFS, top_done=TOP_DONE, may_block=MAY_BLOCK)
# the calls a step is made of (forward flags | backward flags): the fused step with and without T_{L-1} in the forward, the packed and
# the full-row backward behind a forward without buffers / without a target, one conv per layer
CALLS = [SHARED | TARGET | BUFFERS | COEFFS | PACKED | MAY_BLOCK, SHARED | TARGET | BUFFERS | PACKED | MAY_BLOCK | TOP_DONE,
         SHARED | TARGET | COEFFS | PACKED, SHARED | PACKED | TOP_DONE, SHARED, 0]
SWITCHES = list(itertools.product((0, 1, 2), (0, 1), (0, 1), (0, 1)))          # narrow_forward, backward_fused, top_in_forward, backward_block
# around 1, one and two 256-node steps / 512-node tiles, 64 steps and 64 tiles (coefficient launch first or not), one range per slab row
SIZES = [1, 255, 256, 257, 511, 512, 513, 64 * 256 - 1, 64 * 256, 64 * 512 - 1, 64 * 512, 131072, 131073]
# kinds of a record
F_WIDE, F_NODE, F_GROUP, TARGET_, SOURCE_, TARGET0_, FUSED_, GROUP_ = range(8)

_facts, _sw, _out = (C.c_int64 * len(FACTS))(), (C.c_int32 * 4)(), (C.c_int32 * (HEAD + 39 * 8))()


def plan_host(f, sw, cap=len(_out)):
    _facts[:] = [f[k] for k in FACTS]
    _sw[:] = sw
    n = _native.lib().gadapt_narrow_step_plan_host(_facts, _sw, _out, cap)
    return n if n < 0 else _out[:n]


@functools.lru_cache(maxsize=None)
def _of_size(n):
    """(slab rows, whether 8 loss partials per 512-node tile stay within their maximum) at n nodes"""
    return _native.lib().gadapt_backward_slab_rows(n, C_), int(-(-n // 512) * 8 <= _native.lib().gadapt_loss_partials_max())


def facts_of(n, e, layers, flags, halo_t=0, halo_s=0, kmax=5, takes=1, **over):
    f = dict(n_nodes=n, n_edges=e, c=C_, n_layers=layers, takes=takes, halo_t=halo_t, halo_s=halo_s, kmax=kmax,
             slab_rows=_of_size(n)[0], tiles_ok=_of_size(n)[1], ell_t=1, ell_s=1, tpos_s=1, rowptr_s=1, col_s=1)
    f.update({k: int(bool(flags & v)) for k, v in FLAG_OF.items()})
    f.update(over)
    return f


@functools.lru_cache(maxsize=None)
def _stage_groups(n_stages):
    out, done = [], 0
    while (k := _native.lib().gadapt_narrow_bwd_block_groups_host(n_stages, done)) > 0:
        out.append(k); done += k
    return tuple(out)


def stage_groups(n_stages):
    return list(_stage_groups(n_stages))


def record(kind, layer, count=1, g_in=-1, g_out=-1, e_in=-1, e_out=-1, d_in=-1, d_out=-1, acc=0, first=0, last=0, top=0):
    return [kind, layer, count, g_in, g_out, e_in, e_out, d_in, d_out, acc, first, last, top]


def expected(f, sw):
    """include/gadapt_hip.h, 'The launch sequence of a narrow step', sentence by sentence."""
    fwd_sw, fused_sw, top_sw, block_sw = sw
    n, e, c, L = f['n_nodes'], f['n_edges'], f['c'], f['n_layers']
    layout = [0, n * c, 0, 4 * n + 2 * e, 0, 4 * n]
    if not f['takes'] or L < 1:
        return [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, WORDS] + layout
    one_range, short = n <= 256 * f['slab_rows'], f['kmax'] <= 8
    # FORWARD
    in_groups = fwd_sw == 1 and f['shared'] and f['halo_t'] and f['tiles_ok']
    sizes = [min(4, L - l) for l in range(0, L, 4)] if in_groups else [1] * L
    # TOP IN FORWARD
    top = bool(top_sw and in_groups and f['target'] and f['buffers'] and L >= 2 and f['ell_t'] and f['tpos_s'] and e > 0 and short and one_range)
    fwd, l = [], 0
    for k in sizes:
        last = l + k == L
        fwd.append(record(F_GROUP if in_groups else (F_NODE if fwd_sw else F_WIDE), l, k, first=int(l == 0), last=int(last), top=int(top and last),
                          e_out=0 if top and last else -1, d_out=0 if top and last else -1))
        l += k
    # COEFFICIENTS FIRST
    wgs = -(-n // 512) if in_groups else -(-n // 256)
    coeffs_first = int(bool(f['coeffs'] and wgs < 64))
    # BACKWARD
    bwd, kind, halo = [], 0, 0
    if L >= 2:
        fits = 2 * e <= ((c - 8) if L > 4 else (c - 4)) * n
        if (f['may_block'] and block_sw and fused_sw and f['halo_s'] and f['packed'] and f['shared'] and L >= 3 and e > 0 and f['ell_t'] and f['ell_s']
                and f['tpos_s'] and f['rowptr_s'] and short and one_range and fits):
            kind, halo = 2, f['halo_s']
        elif fused_sw and f['ell_s'] and f['rowptr_s'] and f['col_s'] and 2 * e <= (c - 4) * n:
            kind = 1
        t_top = record(TARGET_, L - 1, e_out=0, d_out=0, first=1)                      # accumulate = 0: writes every slab row
        if kind == 0:
            for l in range(L - 1, 0, -1):
                top_l = int(l == L - 1)
                g_in = -1 if top_l else (L - 1 - (l + 1)) & 1                       # what S_{l+1} wrote
                if not (top_l and f['top_done']):
                    bwd.append(t_top if top_l else record(TARGET_, l, g_in=g_in, e_out=0, d_out=0, acc=f['shared']))
                bwd.append(record(SOURCE_, l, g_in=g_in, g_out=(L - 1 - l) & 1, e_in=0, d_in=0, first=top_l))
            bwd.append(record(TARGET0_, 0, g_in=(L - 2) & 1, acc=f['shared'], last=1))
        else:
            if not f['top_done']:
                bwd.append(t_top)
            counts = stage_groups(L - 1) if kind == 2 else [1] * (L - 1)
            l = L - 1
            for m, k in enumerate(counts):
                last = l - k == 0
                d_in = m & 1 if kind == 2 else 0
                r = record(GROUP_ if kind == 2 else FUSED_, l, k, g_in=-1 if m == 0 else (m - 1) & 1, e_in=m & 1, d_in=d_in,
                           acc=1 if kind == 2 else f['shared'], first=int(m == 0), last=int(last))
                if not last:
                    r[4], r[6], r[8] = m & 1, (m + 1) & 1, ((m + 1) & 1 if kind == 2 else 0)
                bwd.append(r)
                l -= k
    head = [1, len(fwd), len(bwd), 2 if in_groups else (1 if fwd_sw else 0), f['halo_t'] if in_groups else 0, coeffs_first, int(top), kind, halo,
            f['top_done'], int(kind == 2), WORDS] + layout
    return head + [w for r in fwd + bwd for w in r]


def edge_counts(n, c=C_):
    """2 E at, one below and one above (c - 4) N and (c - 8) N (E whole: the nearest counts on either side)."""
    out = set()
    for bound in ((c - 4) * n, (c - 8) * n):
        out |= {bound // 2, bound // 2 + 1, max(bound // 2 - 1, 0)}
    return sorted(out)


def check_invariants(f, plan):
    """(b) of the module docstring."""
    n, e, c, L = f['n_nodes'], f['n_edges'], f['c'], f['n_layers']
    n_fwd, n_bwd = plan[1], plan[2]
    recs = [plan[HEAD + WORDS * i: HEAD + WORDS * (i + 1)] for i in range(n_fwd + n_bwd)]
    fwd, bwd = recs[:n_fwd], recs[n_fwd:]
    # the forward groups partition the layers, sizes 1..4
    assert [r[1] for r in fwd] == [sum(r[2] for r in fwd[:i]) for i in range(n_fwd)] and sum(r[2] for r in fwd) == L
    assert all(1 <= r[2] <= 4 for r in fwd) and [r[10] for r in fwd] == [1] + [0] * (n_fwd - 1) and [r[11] for r in fwd] == [0] * (n_fwd - 1) + [1]
    if not bwd:
        assert L < 2
        return
    if plan[7] == 2:                                                                # stage groups are gadapt_narrow_bwd_block_groups_host's
        assert [r[2] for r in bwd if r[0] == GROUP_] == stage_groups(L - 1)
    g_off, d_off, e_off = plan[12:14], plan[14:16], plan[16:18]
    reads = lambda r: {('g', r[3]) if r[3] >= 0 else ('g_top',) if r[10] else None, ('e', r[5]) if r[5] >= 0 else None, ('d', r[7]) if r[7] >= 0 else None} - {None}
    writes = lambda r: {('g', r[4]) if r[4] >= 0 else None, ('e', r[6]) if r[6] >= 0 else None, ('d', r[8]) if r[8] >= 0 else None} - {None}
    prev_w = {('e', 0), ('d', 0)} if f['top_done'] else set()                       # what T_{L-1} left, in the forward launch
    prev_r = {('g_top',)}
    assert ('g_top',) in reads(bwd[0])                                             # the first launch reads the top gradient
    for i, r in enumerate(bwd):
        rd, wr = reads(r), writes(r)
        in_place = {('d', 0)} if r[0] == FUSED_ else set()
        assert not (rd & wr) - in_place, (i, r)
        assert prev_w <= rd and rd - prev_w <= prev_r, (i, r, prev_w, prev_r)      # reads what the launch before wrote (+ its intact inputs)
        prev_w, prev_r = wr, rd
        # offsets + extents inside dxd_ws (N c floats), edge_ws (2 E) and g_ws (2 N c)
        for k in (r[3], r[4]):
            assert k < 0 or g_off[k] + 4 * n <= 2 * n * c
        for k in (r[7], r[8]):
            assert k < 0 or d_off[k] + 4 * n <= n * c
        for k in (r[5], r[6]):
            assert k < 0 or (e_off[0] + 2 * e <= 2 * max(e, 1) if k == 0 else e_off[1] + 2 * e <= n * c)
        if r[5] == 1 or r[6] == 1:                                                  # the second edge buffer lies behind dxd 0 and before dxd 1
            assert e_off[1] >= d_off[0] + 4 * n and (1 not in (r[7], r[8]) or d_off[1] >= e_off[1] + 2 * e)
    slab_writers = [r for r in bwd if r[0] != SOURCE_]
    if f['shared']:                                                                 # only the first slab-writing launch has accumulate = 0
        assert [r[9] for r in slab_writers] == ([] if f['top_done'] else [0]) + [1] * (len(slab_writers) - (0 if f['top_done'] else 1))
    last = bwd[-1]
    assert last[11] == 1 and last[1] - last[2] == (0 if last[0] in (FUSED_, GROUP_) else -1) and last[4] == last[6] == last[8] == -1
    assert all(r[11] == 0 for r in bwd[:-1])


@pytest.mark.parametrize("halo_s", [0, 32, 64])
@pytest.mark.parametrize("halo_t", [0, 32, 64])
@pytest.mark.parametrize("layers", range(2, 9))
def test_plan_is_the_headers_rules_and_keeps_its_invariants(layers, halo_t, halo_s):
    seen = set()
    for n in SIZES:
        for e, kmax, flags, sw in itertools.product(edge_counts(n), (8, 9), CALLS, SWITCHES):
            f = facts_of(n, e, layers, flags, halo_t, halo_s, kmax)
            plan = plan_host(f, sw)
            assert plan == expected(f, sw), (f, sw)
            key = (n, e, f['top_done'], f['shared'], tuple(plan))
            if key not in seen:
                seen.add(key)
                check_invariants(f, plan)


def test_missing_tables_edgeless_graphs_and_other_routes():
    """The facts the sweep holds fixed: each table absent in turn, no edges, tiles beyond the loss partials, a graph the route does not
    take, a single layer."""
    for layers, sw in itertools.product((1, 2, 3, 4, 6), SWITCHES):
        for flags in CALLS:
            for over in ({'ell_t': 0, 'halo_t': 0}, {'ell_s': 0, 'halo_s': 0}, {'tpos_s': 0}, {'rowptr_s': 0, 'halo_s': 0}, {'col_s': 0}, {'tiles_ok': 0},
                         {'takes': 0}, {'slab_rows': 8}):
                f = facts_of(3000, 11000, layers, flags, **{**dict(halo_t=32, halo_s=64), **over})
                plan = plan_host(f, sw)
                assert plan == expected(f, sw), (f, sw)
                if f['takes']:
                    check_invariants(f, plan)
            f = facts_of(3000, 0, layers, flags, 32, 32)
            assert plan_host(f, sw) == expected(f, sw)
    assert plan_host(facts_of(3000, 11000, 4, CALLS[0], takes=0), (1, 1, 1, 1))[:3] == [0, 0, 0]


def _graph_facts(g, layers, flags):
    """The facts of a step read off a MeshGraph (all its tables are built; the halos are the ones it registered)."""
    n = g.num_nodes
    big = g.wide_deg['t'] <= 0
    half = not big and g.wide_half_deg > 0 and -(-n // 256) <= 128
    kmax = g.wide_big_deg if big else (g.wide_half_deg if half else g.wide_deg['t'])
    return facts_of(n, g.num_edges, layers, flags, g.narrow_block_halo, g.narrow_block_halo_source, kmax, takes=int(g.narrow_route(C_)))


def _library_matches(g):
    lib = _native.lib()
    out = (C.c_int32 * len(_out))()
    setters = (lib.gadapt_debug_set_narrow_forward, lib.gadapt_debug_set_narrow_backward_fused, lib.gadapt_debug_set_narrow_top_in_forward,
               lib.gadapt_debug_set_narrow_backward_block)
    try:
        for sw in SWITCHES:
            for fn, v in zip(setters, sw):
                assert fn(v) == 0
            for layers, flags in itertools.product((2, 3, 4, 6), CALLS):
                n = lib.gadapt_narrow_step_plan(g.c_ref, C_, layers, flags, out, len(out))
                assert n > 0 and out[:n] == plan_host(_graph_facts(g, layers, flags), sw), (sw, layers, flags)
            assert lib.gadapt_narrow_block_halo(g.c_ref, C_) == (g.narrow_block_halo if sw[0] == 1 and g.narrow_route(C_) else 0)
    finally:
        for fn in setters:
            fn(1)


@pytest.mark.parametrize("mesh_n,batch,want", [(16, 1, 32), (23, 7, 32), (64, 2, 64)], ids=['16x16-b1', '23x23-b7', '64x64-b2'])
def test_library_plan_is_the_pure_function_of_the_graphs_facts_square_meshes(mesh_n, batch, want, monkeypatch):
    monkeypatch.setattr(graph_mod, 'WIDE_MIN_NODES', 0)
    d = collate(MeshDataset([mesh_n, mesh_n], batch, seed=0).samples)
    g = MeshGraph(masked_edge_index(d, 2, mesh_n), d.x_comp.shape[0], 'cpu')
    assert g.narrow_block_halo == want and g.narrow_route(C_)
    _library_matches(g)


@pytest.mark.parametrize("case_id", ng.IDS)
def test_library_plan_is_the_pure_function_of_the_graphs_facts_narrow_graphs(case_id, monkeypatch):
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
    g = GNN(ds, opt)._graph(data, data.x_comp.shape[0], torch.device('cpu'))
    assert g.num_nodes == c.nodes
    _library_matches(g)


def test_a_graph_the_route_does_not_take_has_no_launches(monkeypatch):
    monkeypatch.setattr(graph_mod, 'WIDE_KERNELS', False)                           # the tiled kernels
    g = MeshGraph(torch.tensor([[0, 1], [1, 0]]), 2, 'cpu')
    out = (C.c_int32 * HEAD)()
    assert not g.narrow_route(C_) and _native.lib().gadapt_narrow_step_plan(g.c_ref, C_, 4, CALLS[0], out, HEAD) == HEAD and out[:3] == [0, 0, 0]


def test_bad_arguments_are_refused():
    lib = _native.lib()
    f = facts_of(3000, 11000, 4, CALLS[0], 32, 32)
    need = len(plan_host(f, (1, 1, 1, 1)))
    assert need == HEAD + WORDS * (1 + 2) and plan_host(f, (1, 1, 1, 1), cap=need) != -1
    assert plan_host(f, (1, 1, 1, 1), cap=need - 1) == -1 and plan_host(f, (1, 1, 1, 1), cap=-1) == -1
    assert HEAD + 39 * 8 >= max(len(plan_host(facts_of(3000, 11000, 8, fl), sw)) for fl in CALLS for sw in SWITCHES)
    for bad in (dict(n_nodes=0), dict(n_edges=-1), dict(n_layers=0), dict(c=0), dict(halo_t=48), dict(halo_s=16), dict(kmax=-1),
                dict(n_nodes=1 << 24), dict(n_nodes=1 << 20, n_edges=(1 << 30) - (1 << 22))):     # N c 4 = 4 GiB; 8 N + 2 E = 2^31
        assert plan_host(dict(f, **bad), (1, 1, 1, 1)) == -1, bad
    assert plan_host(dict(f, n_nodes=(1 << 24) - 1, slab_rows=512), (1, 1, 1, 1)) != -1
    assert plan_host(f, (3, 1, 1, 1)) == -1 and plan_host(f, (-1, 1, 1, 1)) == -1
    _facts[:] = [f[k] for k in FACTS]
    _sw[:] = (1, 1, 1, 1)
    assert lib.gadapt_narrow_step_plan_host(None, _sw, _out, len(_out)) == -1 and lib.gadapt_narrow_step_plan_host(_facts, None, _out, len(_out)) == -1
    assert lib.gadapt_narrow_step_plan_host(_facts, _sw, None, len(_out)) == -1
    g = MeshGraph(torch.tensor([[0, 1], [1, 0]]), 2, 'cpu')
    out = (C.c_int32 * 64)()
    assert lib.gadapt_narrow_step_plan(None, C_, 4, 0, out, 64) == -1 and b'narrow_step_plan' in lib.gadapt_last_error()
    assert lib.gadapt_narrow_step_plan(g.c_ref, C_, 4, 0, None, 64) == -1 and lib.gadapt_narrow_step_plan(g.c_ref, C_, 0, 0, out, 64) == -1
    assert lib.gadapt_narrow_step_plan(g.c_ref, C_, 4, 128, out, 64) == -1 and lib.gadapt_narrow_step_plan(g.c_ref, C_, 4, -1, out, 64) == -1
    assert lib.gadapt_narrow_step_plan(g.c_ref, C_, 4, 0, out, HEAD - 1) == -1 and b'cap' in lib.gadapt_last_error()
    assert lib.gadapt_narrow_step_plan(g.c_ref, 0, 4, 0, out, 64) == -1
