"""The cases of tests/gat_graphs.py on the CPU: the restatement is the oracle's arithmetic, every case is what it claims - the launch
plan from the library's own `gadapt_gat_plus_partial_rows` (host code), the in-degrees from the built `MeshGraph` - and every case is
QUIET: the fp32 restatement stays below half of each floor against fp64 (5e-6 on x_L and alpha, 5e-5 on the three gradients), so a
miss of a floor in tests/test_gpu_gat_graphs.py cannot hide behind the reference's own rounding.  If an edit to `s_blocks()` moves the
thresholds, `test_case_is_what_it_claims` fails instead of the GPU tests silently testing nothing."""
import pytest
import torch
import torch.nn.functional as F

import gat_graphs as gg

from helpers import edge_order_band, make_case, oracle_fp64_twin, rel_err
from g_adaptivity_amd._native import lib
from oracle.pyg_restatement import masked_edge_index, node_features


def test_restatement_is_the_oracle():
    """`block_restated` in fp64 against the fp64 `OracleGNN` with `conv_type='GAT_plus'` behind the identity (zero-pad) encoder: x_L,
    the last layer's attention and both parameter gradients to 1e-12, per-layer and shared vectors, 'GAT_res_lap' and 'GAT_lin', with and
    without `residual`."""
    forms = ((False, 'GAT_res_lap', 'tanh', True), (True, 'GAT_lin', 'selu', True), (False, 'GAT_res_lap', 'elu', False))
    for share, kind, non_lin, residual in forms:
        opt, ds, data, oracle = make_case((9, 9), 2, 16, gg.L, 'GAT_plus', seed=2, gat_plus_type=kind, non_lin=non_lin, share_conv=share,
                                          residual=residual)
        oracle = oracle.double()
        d64 = data.clone()
        for k in ('x_comp', 'f_tensor', 'uu_tensor'):
            setattr(d64, k, getattr(d64, k).double())
        _, x_top, alphas, ei = oracle(d64, return_all=True)
        up = torch.randn(x_top.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        (x_top * up).sum().backward()
        layers = [oracle.conv_layers[0]] if share else list(oracle.conv_layers)
        att_src, att_dst = (torch.stack([getattr(l, name).reshape(-1) for l in layers]) for name in ('att_src', 'att_dst'))
        with torch.no_grad():
            x0 = oracle.enc(node_features(d64, 2, opt['gnn_inc_feat_f'], opt['gnn_inc_feat_uu']))
        assert x0.shape == (162, 16) and x0[:, 4:].abs().max().item() == 0.0 and torch.equal(ei, masked_edge_index(data, 2, 9))
        y, alpha, _, d_src, d_dst = gg.block_restated(x0, ei, att_src, att_dst, gg.L, opt['time_step'], residual, kind == 'GAT_res_lap', non_lin,
                                                      torch.float64, up=up)
        assert (y - x_top).abs().max().item() <= 1e-12 and (alpha - alphas[-1].reshape(-1)).abs().max().item() <= 1e-12
        want_src, want_dst = (torch.stack([getattr(l, name).grad.reshape(-1) for l in layers]) for name in ('att_src', 'att_dst'))
        assert want_src.abs().max().item() > 0 and want_dst.abs().max().item() > 0
        assert (d_src - want_src).abs().max().item() <= 1e-12 and (d_dst - want_dst).abs().max().item() <= 1e-12


def test_alpha_order_is_the_looped_graphs():
    """`reference` hands alpha out in the target-CSR order of `MeshGraph.with_self_loops()`: every row sums to 1, the self-loop is the
    last entry of its row, and a node whose only in-edge is its self-loop has the weight 1."""
    b = gg.build('random-c8')
    g = b.looped
    rp = g.rowptr_t.long()
    a = gg.reference('random-c8')['alpha']
    assert a.shape == (g.num_edges,) and g.num_edges == int((b.ei[0] != b.ei[1]).sum()) + b.n
    rows = torch.zeros(b.n, dtype=torch.float64).index_add_(0, torch.repeat_interleave(torch.arange(b.n), rp[1:] - rp[:-1]), a)
    assert (rows - 1).abs().max().item() <= 1e-12
    assert torch.equal(g.col_t.long()[rp[1:] - 1], torch.arange(b.n))
    assert a[rp[17]].item() == 1.0 and int(rp[18] - rp[17]) == 1


@pytest.mark.parametrize("case_id", gg.IDS)
def test_case_is_what_it_claims(case_id):
    b = gg.build(case_id)
    c = b.case
    deg = gg.in_degrees(b.looped)
    rows = lib().gadapt_gat_plus_partial_rows(b.n, c.c)
    slots = 256 // gg.lanes_per_node(c.c)
    groups = -(-b.n // slots)
    per_blk = -(-groups // rows)
    print(f"{case_id}: C {c.c} N {b.n} E {b.looped.num_edges} rows {rows} groups {groups} per_blk {per_blk} "
          f"in-degree {int(deg.min())}..{int(deg.max())}")
    assert b.n == c.n == b.looped.num_nodes and b.ptr[-1] == b.n
    assert rows == c.rows and per_blk == c.per_blk and groups == c.n_blocks == -(-b.n * gg.lanes_per_node(c.c) // 256)
    assert (rows, per_blk, c.n_blocks) == gg.plan(b.n, c.c)
    assert (int(deg.min()), int(deg.max())) == c.deg
    assert b.looped.num_edges <= 2 ** 31 // 4 and b.n * c.c * 4 < 2 ** 32
    if c.lone is not None:
        assert int(deg[c.lone]) == 1
    else:
        assert int(deg.min()) >= 2


def test_the_table_reaches_every_path():
    """What the table is for, from the library's own plan: the reduce with 96 / 104 / 128 / 136 rows and at the cap, 104 rows at
    every lane split, one / two / three node groups per workgroup, workgroups left without a group, one block and 8 | 9 blocks."""
    rows = {cid: lib().gadapt_gat_plus_partial_rows(c.n, c.c) for cid, c in gg.CASES.items()}
    assert {96, 104, 128, 136, 1016, 1024} <= set(rows.values())
    assert {gg.CASES[cid].c for cid, r in rows.items() if r == 104} == {4, 8, 16, 32, 64, 128}
    assert {c.per_blk for c in gg.CASES.values()} == {1, 2, 3}
    for cid, busy in (('two-groups', 513), ('three-groups', 683), ('two-groups-c64', 576)):
        c = gg.CASES[cid]
        assert rows[cid] == 1024 and -(-c.n_blocks // c.per_blk) == busy              # the other workgroups write zero partials
    assert gg.CASES['cap-1024'].n + 1 == gg.CASES['two-groups'].n and gg.CASES['reduce-96'].n + 1 == gg.CASES['reduce-104'].n
    assert gg.CASES['reduce-128'].n + 1 == gg.CASES['reduce-136'].n
    assert (gg.CASES['tiny-c4'].n_blocks, gg.CASES['blocks-8'].n_blocks, gg.CASES['blocks-9'].n_blocks) == (1, 8, 9)
    # the shared-vector runs (`accumulate` in reduce_kernel): the four reduce shapes at C = 128 and two groups per workgroup
    assert [cid for cid, s in gg.RUNS if s == 1] == ['reduce-96', 'reduce-104', 'reduce-128', 'reduce-136', 'two-groups']


def test_rows_of_eight_and_nine_meet():
    """The unrolled path takes in-rows up to 8, the CSR loops the longer ones: the random graph has rows of exactly 8 and 9 and a row of
    more than 30 (node 11); on the union-jack meshes and in `mixed` rows of 9 sit in one 64-lane wave with shorter ones."""
    deg = gg.in_degrees(gg.build('random-c64').looped)
    assert int((deg == 8).sum()) > 0 and int((deg == 9).sum()) > 0 and int(deg[11]) >= 31 and int(deg.max()) == int(deg[11])
    for cid in ('union-jack-c8', 'union-jack-c64', 'mixed'):
        c = gg.CASES[cid]
        deg = gg.in_degrees(gg.build(cid).looped)
        per_wave = 64 // gg.lanes_per_node(c.c)
        pad = (-deg.numel()) % per_wave
        waves = torch.cat([deg, deg.new_full((pad,), 5)]).view(-1, per_wave)
        both = ((waves > 8).any(1) & (waves <= 8).any(1))
        assert int(both.sum()) > 0, cid
        # union-jack: corners 3 | 4, sides 4 | 6, interior 5 | 9; `mixed` adds the chain's 2 and the square meshes' 7
        assert set(deg.tolist()) == ({2, 3, 4, 5, 6, 7, 9} if cid == 'mixed' else {3, 4, 5, 6, 9})


def test_spread_case_spreads():
    """`spread` (att_src, att_dst x 8): in the last layer's attention one weight in seventeen lies below 2^-24 - entries that a fp32
    row sum starting from the largest weight no longer sees - and the smallest near 1e-13; the plain case on the same graph has no
    weight below 1e-4.  (At this factor no `exp` reaches fp32's underflow at e^-87: the widest row spans e^-30.)"""
    a = gg.reference('spread')['alpha']
    plain = gg.reference('reduce-104')['alpha']
    share = (a < 2.0 ** -24).double().mean().item()
    print(f"spread: min alpha {a.min().item():.2e}, share below 2^-24 {share:.3f}; plain: min alpha {plain.min().item():.2e}")
    assert share > 0.05 and a.min().item() < 1e-12
    assert plain.min().item() > 1e-4


@pytest.mark.parametrize("case_id,S", gg.RUNS, ids=gg.RUN_IDS)
def test_case_is_quiet(case_id, S):  # noqa: N803
    noise = gg.noise_of(case_id, S)
    r64 = gg.reference(case_id, S)
    print(f"{case_id} S={S}: fp32 restatement vs fp64: " + ", ".join(f"{q} {v:.2e}" for q, v in noise.items()))
    for q, v in noise.items():
        assert v < 0.5 * gg.FLOORS[q], (q, v)
        assert r64[q].abs().max().item() > 0 and bool(torch.isfinite(r64[q]).all())


def test_every_update_form_is_quiet():
    """The 28 (non_lin, residual, res_lap) forms of `test_every_update_form` on the random graph at C = 64."""
    worst = {q: 0.0 for q in gg.QUANTITIES}
    for non_lin in gg.NON_LINS:
        for residual in (True, False):
            for res_lap in (True, False):
                noise = gg.noise_of('random-c64', gg.L, residual=residual, res_lap=res_lap, non_lin=non_lin)
                for q, v in noise.items():
                    assert v < 0.5 * gg.FLOORS[q], (non_lin, residual, res_lap, q, v)
                    worst[q] = max(worst[q], v)
    print("28 forms, worst fp32 restatement vs fp64: " + ", ".join(f"{q} {v:.2e}" for q, v in worst.items()))


@pytest.mark.parametrize("route", list(gg.MODEL_ROUTES))
def test_model_route_case_is_quiet(route):
    """The cases of `test_model_route`: the fp32 oracle against its fp64 twin stays below 5e-5 on every parameter gradient, as run and
    over four other edge orders of the same batch (`helpers.edge_order_band`), and below 1e-5 on the coordinates - so the 1e-4 floor of
    `test_gpu_variants._model_parity` is the bound, on whatever host the oracle runs."""
    r = gg.MODEL_ROUTES[route]
    opt, ds, data, oracle = gg.model_case(route)
    tgt = data.x_phys
    assert data.x_comp.shape[0] == r.nodes and tgt.dim() == 2
    ref = oracle(data)
    F.mse_loss(ref, tgt).backward()
    o64, ref64 = oracle_fp64_twin(oracle, ds, opt, data, tgt)
    assert rel_err(ref, ref64)[0] < gg.COORD_TOL
    band = edge_order_band(oracle, o64, data, tgt, k=4)
    d32, d64 = dict(oracle.named_parameters()), dict(o64.named_parameters())
    names = [k for k in band if d32[k].grad is not None]
    assert len(names) == 2 * (1 if r.share else r.layers)
    for k in names:
        once = rel_err(d32[k].grad, d64[k].grad)[0]
        print(f"{route} {k}: fp32 oracle vs fp64 {once:.2e}, over four edge orders {band[k]:.2e}; "
              f"max |gradient| {d64[k].grad.abs().max().item():.1e}")
        assert once < gg.QUIET and band[k] < gg.QUIET, (k, once, band[k])
