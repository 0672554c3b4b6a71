"""Every case of tests/narrow_graphs.py is what it claims, on the CPU: the degrees of the graph the conv layers see, the geometry flags
of `MeshGraph` (`wide_deg`, `wide_big_deg`, `wide_half_deg`), the narrow route, and that the case is QUIET - the fp32 oracle's own
error against its fp64 twin stays below 5e-5 on every parameter gradient and below 1e-5 on the coordinates, so that a gradient of the
HIP path that misses the 1e-4 floor in tests/test_gpu_narrow_graphs.py cannot hide behind the oracle's noise."""
import pytest
import torch

import narrow_graphs as ng
from helpers import rel_err
from g_adaptivity_amd import GNN
from g_adaptivity_amd import graph as graph_mod


def _graph_and_route(b, monkeypatch):
    c = b.case
    monkeypatch.setattr(graph_mod, 'WIDE_MIN_NODES', 0)
    if c.half_max is not None:
        monkeypatch.setattr(graph_mod, 'WIDE_HALF_MAX_NODES', c.half_max)
    model = GNN(b.ds, dict(b.opt))
    d = b.data
    n = d.x_comp.shape[0]
    g = model._graph(d, n, 'cpu')
    assert isinstance(g, graph_mod.MeshGraph) and str(g.device) == 'cpu'
    xc = d.x_comp if d.x_comp.dim() == 2 else d.x_comp.unsqueeze(-1)
    o = model.opt
    r = model._route(d, g, xc, d.f_tensor if o['gnn_inc_feat_f'] else None, d.uu_tensor if o['gnn_inc_feat_uu'] else None)
    return model, g, r


@pytest.mark.parametrize("case_id", ng.IDS)
def test_case_is_what_it_claims(case_id, monkeypatch):
    b = ng.build(case_id)
    c = b.case
    model, g, r = _graph_and_route(b, monkeypatch)
    deg_t, deg_s = ng.degrees(g)
    print(f"{case_id}: N {g.num_nodes} E {g.num_edges} in-degree {deg_t} out-degree {deg_s} wide_deg {g.wide_deg} "
          f"wide_big_deg {g.wide_big_deg} wide_half_deg {g.wide_half_deg}")
    assert g.num_nodes == c.nodes
    assert deg_t == c.deg_t and deg_s == c.deg_s
    # the target orientation decides the route; the window is the 384-row one (wide_deg['t'] = longest in-row) or the 512-row one
    assert (g.wide_deg['t'] == 0) == c.big and (g.wide_big_deg > 0) == c.big
    assert g.wide_deg['t'] == (0 if c.big else c.deg_t[1]) and g.wide_big_deg == (c.deg_t[1] if c.big else 0)
    # out-rows past the ELL-8 table: no ELL form of the source orientation - the narrow source passes walk those rows in CSR
    # (the 512-row window's graphs fail the 384-row locality test in both orientations)
    assert (g.wide_deg['s'] > 0) == (c.ell_s and not c.big)
    assert (g.wide_half_deg > 0) == c.half and g.wide_half_deg in (0, c.deg_t[1])
    assert g.narrow_route(64) and not g.narrow_route(32)
    assert r.form == 'compact' and r.narrow and r.shared and r.plain and r.ident
    # the out-neighbours the fused backward needs an edge buffer for fit the spare tail of its work buffer (else the pairs run)
    assert 2 * g.num_edges <= 60 * g.num_nodes


@pytest.mark.parametrize("case_id", ng.IDS)
def test_case_is_quiet(case_id):
    b = ng.build(case_id)
    norm, elem = rel_err(b.ref, b.ref64)
    print(f"{case_id}: fp32 oracle vs fp64: coordinates normwise {norm:.2e} elementwise {elem:.2e}; gradients "
          + ", ".join(f"{k} {v:.2e}" for k, v in b.noise.items()))
    assert norm < ng.COORD_TOL and elem < ng.COORD_TOL
    for k, v in b.noise.items():
        assert v < ng.QUIET, (k, v)
        assert b.g64[k].abs().max().item() > 0
    kb = b.o64.conv_layers[0].lin_key.bias.grad.abs().max().item()
    assert kb <= 1e-9 * b.g64['lin_query.bias'].abs().max().item() + 1e-18      # vanishes analytically (softmax shift invariance)


def test_ragged_rows_are_where_the_case_says(monkeypatch):
    """The `ragged` edits, row by row, on the graph the conv layers see (after the boundary surgery of `GNN.forward`)."""
    b = ng.build('ragged')
    _, g, _ = _graph_and_route(b, monkeypatch)
    dt = (g.rowptr_t[1:] - g.rowptr_t[:-1]).tolist()
    ds_ = (g.rowptr_s[1:] - g.rowptr_s[:-1]).tolist()
    assert dt[42] == 0 and dt[611] == 0 and dt[90] == 1 and dt[106] == 7 and dt[206] == 8
    assert all(dt[j] == 7 for j in (164, 166, 168, 170, 244, 246, 248, 250))
    assert ds_[130] == 0 and ds_[210] == 14
    assert g.col_t[g.rowptr_t[90]].item() == 89
    assert {0, 1, 2, 6, 7, 8} <= set(dt) and max(dt) == 8                          # (2: boundary rows, 6: the untouched interior)
    assert sum(d > 8 for d in ds_) == 1
    # the oracle starts from the same fields: its edge list is the graph's
    with torch.no_grad():
        _, _, _, ei = b.oracle(b.data, return_all=True)
    assert torch.equal(ei, g.edge_index)


def test_edit_edges_keeps_the_masks_aligned():
    b = ng.build('temp2')
    d = b.data
    e = d.edge_index.shape[1]
    drop = torch.zeros(e, dtype=torch.bool)
    drop[::5] = True
    out = ng.edit_edges(d, drop=drop, add=([3, 4], [40, 41]))
    assert out.edge_index.shape[1] == e - int(drop.sum()) + 2 and d.edge_index.shape[1] == e      # the input batch is left alone
    assert torch.equal(out.edge_index[:, :-2], d.edge_index[:, ~drop]) and out.edge_index[:, -2:].tolist() == [[3, 4], [40, 41]]
    for m in ng.EDGE_MASKS:
        assert torch.equal(getattr(out, m)[:-2], getattr(d, m)[~drop]) and not getattr(out, m)[-2:].any()
        assert getattr(out, m).dtype == getattr(d, m).dtype
    same = ng.edit_edges(d)
    assert torch.equal(same.edge_index, d.edge_index)


def test_rebase_case_rebases(monkeypatch):
    """`rebase-ragged`: with the query / key weights scaled by 4 the scores of an in-row spread past the softmax's re-base threshold
    (a later score more than 16 above the running reference: the row's first weight ends below e^-16 = 1.2e-7).  The forward kernels
    decide per 32-node group, so the whole group of such a row re-bases - among them the group of node 206, the in-row of 8.  At
    this factor the groups of the empty rows (42, 611) and of the one-entry row (90) hold no such row: they take the other branch."""
    shares = {}
    for cid in ('rebase-ragged', 'ragged'):
        b = ng.build(cid)
        _, g, _ = _graph_and_route(b, monkeypatch)
        with torch.no_grad():
            _, _, alphas, _ = b.oracle(b.data, return_all=True)
        a = alphas[0].reshape(-1)[g.eid_t.long()[:g.num_edges]]                      # layer 0, target-CSR order
        rp = g.rowptr_t.long()
        has = rp[1:] > rp[:-1]
        first = torch.ones(g.num_nodes)
        first[has] = a[rp[:-1][has]]
        hit = first < 1.2e-7
        groups = hit.view(-1, 32).any(dim=1)
        shares[cid] = hit.float().mean().item()
        print(f"{cid}: rows whose first weight is below 1.2e-7: {int(hit.sum())} of {g.num_nodes} ({shares[cid]:.3f}), in {int(groups.sum())} of "
              f"{groups.numel()} groups; groups of nodes 42, 90, 206, 611: {[bool(groups[j // 32]) for j in (42, 90, 206, 611)]}")
        if cid == 'rebase-ragged':
            assert shares[cid] > 0.05 and groups[206 // 32] and 10 <= int(groups.sum()) < groups.numel()
    assert shares['ragged'] < 0.01
