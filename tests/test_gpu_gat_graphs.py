"""The fused GAT_plus block (`functional.gat_plus_block`, csrc/gadapt_gat.inc) against its fp64 restatement on the cases of
tests/gat_graphs.py: the smallest graphs at which each path of the backward's launch plan runs - `reduce_kernel` with 96 / 104 / 128 /
136 partial rows and 104 rows at every lane split, the cap of 1024 workgroups, two and three node groups per workgroup with workgroups
that get none, one block, 8 | 9 blocks - and union-jack meshes, mixed mesh sizes, 1-D chains, the random graph with its long rows,
widely spread scores.  tests/test_gat_graphs_host.py proves on the CPU, from the library's own `gadapt_gat_plus_partial_rows`, that
every case is what it claims, and that it is quiet (the fp32 restatement below half of each floor).

The rule is the project's own: `err <= max(floor, 1.5 x noise)`, `err` = the block against the fp64 restatement, `noise` = the fp32
restatement against fp64 (both `helpers.rel_err(...)[0]`), floor 1e-5 for x_L and alpha, 1e-4 for d x0, d att_src, d att_dst.  The
figures every test prints are on record in docs/measurements.md ("Fused GAT_plus block against fp64 at its launch-plan edges").
"""
import functools

import pytest
import torch

import gat_graphs as gg
import test_gpu_variants as variants
from helpers import oracle_fp64_twin, rel_err
from g_adaptivity_amd import MeshGraph
from g_adaptivity_amd import functional as Fn

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]          # the GAT route does not depend on graph.WIDE_MIN_NODES


@functools.lru_cache(maxsize=None)
def _looped(parts, dev):
    ei, n, _ = gg.graph_of(parts)
    return MeshGraph(ei, n, dev).with_self_loops()


def _run(looped, x0, up, att, dev, want_dx0=True, residual=True, res_lap=True, non_lin='tanh'):
    """{quantity: tensor} of one forward + backward of the block on (x_L * up).sum(); 'd x0' is None without `want_dx0`."""
    x = x0.to(dev).requires_grad_(want_dx0)
    s_, d_ = (t.to(dev).requires_grad_(True) for t in att)
    y, alpha = Fn.gat_plus_block(x, s_, d_, looped, gg.L, gg.DT, residual, res_lap, non_lin)
    (y * up.to(dev)).sum().backward()
    torch.cuda.synchronize()
    return dict(zip(gg.QUANTITIES, (y.detach(), alpha[-1].detach(), x.grad, s_.grad, d_.grad)))


def _rule(label, got, r64, noise):
    """err <= max(floor, 1.5 x noise) on the five quantities; every figure printed first."""
    bad = []
    for q in gg.QUANTITIES:
        assert got[q].shape == r64[q].shape and bool(torch.isfinite(got[q]).all()), (label, q)
        err, bound = rel_err(got[q], r64[q])[0], max(gg.FLOORS[q], 1.5 * noise[q])
        print(f"{label} | {q} | err {err:.2e} | noise {noise[q]:.2e} | bound {bound:.0e}")
        if not err <= bound:
            bad.append(f"{label} {q}: {err:.2e} against fp64 (fp32 restatement: {noise[q]:.2e}, bound {bound:.0e})")
    assert not bad, bad


@pytest.mark.parametrize("case_id,S", gg.RUNS, ids=gg.RUN_IDS)
def test_block_against_fp64(gpu_device, case_id, S):  # noqa: N803
    b = gg.build(case_id)
    looped = _looped(b.case.parts, gpu_device)
    assert looped.num_nodes == b.n and torch.equal(looped.eid_t.cpu(), b.looped.eid_t)
    got = _run(looped, b.x0, b.up, b.att[S], gpu_device)
    _rule(case_id if S == gg.L else case_id + '-shared', got, gg.reference(case_id, S), gg.noise_of(case_id, S))
    if b.case.lone is not None:                                          # a row of the self-loop alone: e^0 / (e^0 + 1e-16)
        rp = b.looped.rowptr_t
        assert int(rp[b.case.lone + 1] - rp[b.case.lone]) == 1 and got['alpha'][int(rp[b.case.lone])].item() == 1.0


def test_every_update_form(gpu_device):
    """All 28 (non_lin, residual, res_lap) forms of the update (`src/GNN.py:284-296`, 'GAT_res_lap' | 'GAT_lin') on the random graph at
    C = 64, under the same rule."""
    b = gg.build('random-c64')
    looped = _looped(b.case.parts, gpu_device)
    for non_lin in gg.NON_LINS:
        for residual in (True, False):
            for res_lap in (True, False):
                form = dict(residual=residual, res_lap=res_lap, non_lin=non_lin)
                got = _run(looped, b.x0, b.up, b.att[gg.L], gpu_device, **form)
                _rule(f"{non_lin} residual={int(residual)} res_lap={int(res_lap)}", got, gg.reference('random-c64', gg.L, **form),
                      gg.noise_of('random-c64', gg.L, **form))


@pytest.mark.parametrize("case_id", ['two-groups', 'mixed'])
def test_a_mesh_does_not_depend_on_its_batch(gpu_device, case_id):
    """Every member graph alone against its rows in the batch (the same x0 rows, `up` rows and vectors): x_L, alpha and d x0 bit for
    bit - every node's arithmetic is its own and rows are walked in the caller's edge order, wherever the node group falls in the
    workgroups' runs (`two-groups`: two groups per workgroup).  d att_* sums over the meshes and is not compared."""
    b = gg.build(case_id)
    whole = _run(_looped(b.case.parts, gpu_device), b.x0, b.up, b.att[gg.L], gpu_device)
    rp = b.looped.rowptr_t.long()
    for part, lo, hi in zip(b.case.parts, b.ptr[:-1], b.ptr[1:]):
        alone = _run(_looped((part,), gpu_device), b.x0[lo:hi], b.up[lo:hi], b.att[gg.L], gpu_device)
        assert alone['alpha'].shape[0] == int(rp[hi] - rp[lo])
        for q, rows in (('x_L', slice(lo, hi)), ('d x0', slice(lo, hi)), ('alpha', slice(int(rp[lo]), int(rp[hi])))):
            assert torch.equal(alone[q], whole[q][rows]), (case_id, part, lo, q, rel_err(alone[q], whole[q][rows]))


@pytest.mark.parametrize("case_id", ['reduce-136', 'two-groups'])
def test_parameter_partials_without_d_x0(gpu_device, case_id):
    """Layer 0's source pass without a d x0 to write (`bwd_s_kernel` with `dx == NULL`: the parameter partials only) gives the bits of
    the pass that writes it."""
    b = gg.build(case_id)
    looped = _looped(b.case.parts, gpu_device)
    for S in (gg.L, 1):  # noqa: N806
        with_dx, without = (_run(looped, b.x0, b.up, b.att[S], gpu_device, want_dx0=w) for w in (True, False))
        assert without['d x0'] is None and with_dx['d x0'] is not None
        for q in ('x_L', 'alpha', 'd att_src', 'd att_dst'):
            assert torch.equal(with_dx[q], without[q]), (case_id, S, q, rel_err(without[q], with_dx[q]))
        assert with_dx['d att_src'].abs().max().item() > 0


@pytest.mark.parametrize("case_id", ['two-groups', 'three-groups'])
def test_bit_reproducible(gpu_device, case_id):
    """Two runs, equal bits on all five outputs: the partial rows are summed in a fixed order."""
    b = gg.build(case_id)
    looped = _looped(b.case.parts, gpu_device)
    first, second = (_run(looped, b.x0, b.up, b.att[gg.L], gpu_device) for _ in range(2))
    for q in gg.QUANTITIES:
        assert torch.equal(first[q], second[q]), (case_id, q)


@pytest.mark.parametrize("route", list(gg.MODEL_ROUTES))
def test_model_route(gpu_device, route, monkeypatch):
    """Through `GNN.forward` (the `out_cols` slice and the `x_all` buffer the model passes) with `test_gpu_variants._model_parity`:
    36864 nodes at hidden 64 (two node groups per workgroup), mixed mesh sizes, 1-D meshes.  The cases are quiet
    (tests/test_gat_graphs_host.py): the bound is `_model_parity`'s 1e-4 floor."""
    r = gg.MODEL_ROUTES[route]
    case = gg.model_case(route)
    monkeypatch.setattr(variants, 'make_case', lambda *a, **k: case)     # the mixed batch and the [N,1] target of a 1-D one
    model, oracle, checked = variants._model_parity(gpu_device, r.dims, r.batch, r.hidden, r.layers, 'GAT_plus', seed=r.seed, non_lin='tanh',
                                                    share_conv=r.share)
    o64, _ = oracle_fp64_twin(oracle, case[1], case[0], case[2], case[2].x_phys)          # the figures `_model_parity` asserted on
    d32, d64, got = dict(oracle.named_parameters()), dict(o64.named_parameters()), dict(model.named_parameters())
    for name in checked:
        print(f"{route} | {name} | err {rel_err(got[name].grad, d64[name].grad)[0]:.2e} | noise {rel_err(d32[name].grad, d64[name].grad)[0]:.2e}")
    assert model._gat_plus_fusable() and case[2].x_comp.shape[0] == r.nodes
    if r.mixed:
        assert len(set(torch.bincount(case[2].batch).tolist())) > 1
    assert sorted(checked) == sorted(f'conv_layers.{l}.{v}' for l in range(1 if r.share else r.layers) for v in ('att_dst', 'att_src'))
    layer = model.conv_layers[0]
    assert layer.stored_alpha.shape[0] == layer.stored_ei.shape[1] and bool(torch.isfinite(layer.stored_alpha).all())
    assert torch.equal(layer.stored_ei[:, -r.nodes:].cpu(), torch.arange(r.nodes).repeat(2, 1))
