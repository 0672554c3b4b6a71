"""The narrow route against the fp64 oracle on the graphs of tests/narrow_graphs.py: ragged in- and out-rows (out-rows past the ELL-8
table take the CSR loops of `FusedNarrowSource::finish` and of `grand_bwd_source_narrow_kernel`), in-rows of 7, a fixed temperature,
mixed mesh sizes, the 512-row window, the eight-wave geometry on a ragged node count, 1-D meshes.  tests/test_narrow_graphs_host.py
proves on the CPU that every case is what it claims and that it is quiet (fp32 oracle within 5e-5 of fp64 on every gradient).

One test per case, four steps:
 1. autograd path against the oracle: coordinates within 1e-5 (fp32 oracle normwise and elementwise, fp64 normwise); every weight
    gradient `e64 <= max(1e-4, 1.5 x noise)`, `noise` = the fp32 oracle against fp64, one run (tests/test_gpu_parity.py's rule without
    the edge-order band: the cases are quiet); d lin_key.bias exactly 0;
 2. the debug switches (narrow / wide forward kernel, fused / paired backward) give bit-identical outputs and gradients, the paired
    backward makes `layers - 1` source launches and the fused one none, two identical runs agree bit for bit;
 3. the compact route (`MeshGraph.narrow_route` switched off): same output bits, gradients within 2e-6, and under the fp64 rule too;
 4. `FusedIteration` with `mse_loss` and `l1_loss`: output and flat gradient bit-identical to the autograd path's, the loss value
    within max(1e-6, 1.5 x the fp32 oracle's own deviation) of the fp64 oracle's, the packed slab rows equal to the live entries of
    the full-width slab.  Where the fused iteration does not apply (1-D: `x_comp` is [N]) the reason is asserted instead.

The figures every case prints are on record in docs/measurements.md ("The narrow route against fp64 on ragged, mixed and 1-D graphs").
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import narrow_graphs as ng
from helpers import hip_model_like, rel_err
from test_gpu_narrow_tail import LIVE, PACKED, ROW, _backward_args
from g_adaptivity_amd import graph as graph_mod
from g_adaptivity_amd import l1_loss, mse_loss, unit_gradient
from g_adaptivity_amd._native import current_stream, lib
from g_adaptivity_amd.optim import FlatAdam

NOT_DENSE = 'x_comp / target are not dense fp32 [N,dim] device tensors'


def _route(model, data):
    xc = data.x_comp if data.x_comp.dim() == 2 else data.x_comp.unsqueeze(-1)
    graph = model._graph(data, xc.shape[0], xc.device)
    o = model.opt
    return graph, model._route(data, graph, xc, data.f_tensor if o['gnn_inc_feat_f'] else None, data.uu_tensor if o['gnn_inc_feat_uu'] else None)


def _source_launches():
    tot, cnt = C.c_double(0.0), C.c_int(0)
    lib().gadapt_profile_read(2, C.byref(tot), C.byref(cnt))
    return cnt.value


def _grads(model):
    return {k: p.grad.clone() for k, p in model.conv_layers[0].named_parameters() if p.grad is not None}


def _run(model, data, tgt, narrow_forward=1, backward_fused=1):
    """model(data) + mse backward with the switches set; (output, conv gradients, source-pass launches)."""
    lib().gadapt_debug_set_narrow_forward(narrow_forward)
    lib().gadapt_debug_set_narrow_backward_fused(backward_fused)
    lib().gadapt_profile_reset(); lib().gadapt_profile_enable(1)
    try:
        model.zero_grad(set_to_none=True)
        out = model(data)
        F.mse_loss(out, tgt).backward()
        torch.cuda.synchronize()
        n_source = _source_launches()
    finally:
        lib().gadapt_profile_enable(0); lib().gadapt_profile_reset()
        lib().gadapt_debug_set_narrow_forward(1)
        lib().gadapt_debug_set_narrow_backward_fused(1)
    return out.detach().clone(), _grads(model), n_source


def _fp64_rule(case_id, what, grads, b):
    """e64 <= max(1e-4, 1.5 x noise) on the three weight gradients; every figure printed first."""
    bad = []
    for k in ng.PARAMETERS:
        e64, e32, noise = rel_err(grads[k], b.g64[k])[0], rel_err(grads[k], b.g32[k])[0], b.noise[k]
        bound = max(ng.GRAD_TOL, 1.5 * noise)
        print(f"{case_id} [{what}] {k}: e64 {e64:.2e} e32 {e32:.2e} noise {noise:.2e} bound {bound:.2e}")
        if not e64 <= bound:
            bad.append(f"{what} {k}.grad: {e64:.2e} vs fp64 (fp32 oracle: {noise:.2e})")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("case_id", ng.IDS)
def test_narrow_route_on_the_case(gpu_device, case_id, monkeypatch):
    import g_adaptivity_amd.functional as Fn
    from g_adaptivity_amd.training import FusedIteration
    b = ng.build(case_id)
    c, layers = b.case, b.case.layers
    monkeypatch.setattr(Fn, 'SMALL_MESH_FORWARD', False)
    monkeypatch.setattr(graph_mod, 'WIDE_MIN_NODES', 0)
    if c.half_max is not None:
        monkeypatch.setattr(graph_mod, 'WIDE_HALF_MAX_NODES', c.half_max)
    assert max(b.noise.values()) < ng.QUIET                              # (tests/test_narrow_graphs_host.py)
    model = hip_model_like(b.oracle, b.ds, b.opt, gpu_device).train()
    data, tgt = b.data.clone().to(gpu_device), b.tgt.to(gpu_device)
    graph, r = _route(model, data)
    assert r.narrow and graph.num_nodes == c.nodes
    assert (graph.wide_deg['s'] > 0) == (c.ell_s and not c.big) and (graph.wide_big_deg > 0) == c.big and (graph.wide_half_deg > 0) == c.half

    # ---- 1. the autograd path against the oracle
    out, g, n_source = _run(model, data, tgt)
    assert out.shape == b.ref.shape and not torch.isnan(out).any()
    norm, elem = rel_err(out, b.ref)
    norm64 = rel_err(out, b.ref64)[0]
    print(f"{case_id} coordinates: vs fp32 oracle normwise {norm:.2e} elementwise {elem:.2e}; vs fp64 normwise {norm64:.2e}")
    assert norm <= ng.COORD_TOL and elem <= ng.COORD_TOL and norm64 <= ng.COORD_TOL
    _fp64_rule(case_id, 'narrow', g, b)
    assert g['lin_key.bias'].abs().max().item() == 0.0                   # vanishes analytically (softmax shift invariance)
    assert n_source == 0                                                 # the default: every source pass inside a target pass

    # ---- 2. the switches: narrow / wide forward kernel x fused / paired backward, and a second identical run
    for nf, bf in ((1, 1), (0, 1), (1, 0), (0, 0)):
        out_s, g_s, n_s = _run(model, data, tgt, nf, bf)
        assert n_s == (0 if bf else layers - 1), (nf, bf, n_s)
        assert torch.equal(out_s, out), (nf, bf)
        assert set(g_s) == set(g)
        for k in g:
            assert torch.equal(g_s[k], g[k]), (nf, bf, k, rel_err(g_s[k], g[k]))

    # ---- 3. the compact route on the same graph
    with monkeypatch.context() as mp:
        mp.setattr(graph_mod.MeshGraph, 'narrow_route', lambda self, c_: False)
        assert not _route(model, data)[1].narrow and _route(model, data)[1].form == 'compact'
        out_c, g_c, _ = _run(model, data, tgt)
    assert torch.equal(out_c, out)
    assert set(g_c) == set(g)
    for k in g:
        e = rel_err(g[k], g_c[k])[0]
        print(f"{case_id} narrow vs compact route {k}: {e:.2e}")
        assert e <= 2e-6, (k, e)
    _fp64_rule(case_id, 'compact', g_c, b)                               # (the compact source pass on a graph without an ELL table of out-rows)
    assert _route(model, data)[1].narrow

    # ---- 4. the fused iteration, both native losses
    target_field = 'x_phys'
    optim = FlatAdam(model.parameters(), lr=0.0, capturable=True)
    if len(c.dims) == 1:                                                 # x_comp and the target are [N]: the autograd iteration trains these
        for loss_fn in (mse_loss, l1_loss):
            assert FusedIteration.eligible(model, optim, loss_fn, data, target_field) == NOT_DENSE
        return
    optim.zero_grad(); mse_loss(model(data), data.x_phys).backward(gradient=unit_gradient(gpu_device)); optim.step()   # lays the bucket out
    why = FusedIteration.eligible(model, optim, mse_loss, data, target_field)
    assert why is None, why
    live = LIVE.to(gpu_device)
    for name, loss_fn in (('mse', mse_loss), ('l1', l1_loss)):
        assert FusedIteration.eligible(model, optim, loss_fn, data, target_field) is None
        optim.zero_grad()
        out_a = model(data)
        loss_fn(out_a, data.x_phys).backward(gradient=unit_gradient(gpu_device))
        torch.cuda.synchronize()
        out_a, flat_a = out_a.detach().clone(), torch.cat([p.grad.reshape(-1) for p in optim.active]).clone()
        it = FusedIteration(model, optim, loss_fn, data, target_field)
        assert it.fwd.narrow and it.coeffs_in_forward == (not c.half)
        it.refresh_coeffs()
        for t in (it.slab, it.g_ws, it.dxd_ws, it.edge_ws, it.flat) + (tuple(it.coeffs) if it.coeffs_in_forward else ()):
            t.fill_(float('nan'))
        it.forward_backward()
        torch.cuda.synchronize()
        # (in-forward coefficients: on fewer than 64 steps of 256 nodes a coefficient launch inside the call, else the layer-0 launch)
        want_a, want_p0 = Fn.composite_coeffs(*[p.detach() for p in optim.active[:3]])
        assert torch.equal(it.coeffs[0].reshape(-1), want_a.reshape(-1)) and torch.equal(it.coeffs[1].reshape(-1), want_p0.reshape(-1))
        packed = it.slab.clone().view(it.slab_rows, PACKED)
        it.finish()                                                      # lr = 0: the parameters stay
        torch.cuda.synchronize()
        assert torch.equal(it.out, out_a) and torch.equal(it.out, out)
        assert not torch.isnan(it.flat).any() and torch.equal(it.flat, flat_a), (name, rel_err(it.flat, flat_a))
        if name == 'mse':                                                # the fused step's own gradient under the fp64 rule
            _fp64_rule(case_id, 'fused', {k: gk for k, (p, gk) in zip(ng.PARAMETERS, it.grads)}, b)
        assert it.flat[-64:].abs().max().item() == 0.0                   # d lin_key.bias
        l32, l64 = b.losses[name]
        dev32, got = abs(l32 - l64) / abs(l64), abs(it.loss.item() - l64) / abs(l64)
        print(f"{case_id} {name}_loss: fused {it.loss.item():.9e} fp64 {l64:.9e}: {got:.2e} (fp32 oracle: {dev32:.2e})")
        assert got <= max(1e-6, 1.5 * dev32), (name, got, dev32)
        # the packed slab rows against the full-width slab of the same backward, with either form of the backward
        rows = it.slab_rows
        assert packed.shape == (rows, PACKED) and rows == lib().gadapt_backward_slab_rows(it.n, 64)
        for fused in (1, 0):
            full = torch.full((rows, ROW), float('nan'), device=gpu_device)
            again = torch.full((rows, PACKED), float('nan'), device=gpu_device)
            lib().gadapt_debug_set_narrow_backward_fused(fused)
            try:
                it.fwd(*it._in, current_stream(it.device))
                assert lib().gadapt_block_backward_narrow(*_backward_args(it, full)) == 0
                assert lib().gadapt_block_backward_narrow_packed(*_backward_args(it, again)) == 0
                torch.cuda.synchronize()
            finally:
                lib().gadapt_debug_set_narrow_backward_fused(1)
            assert not torch.isnan(full).any()
            assert torch.equal(again, packed) and torch.equal(packed[:, :20], full[:, live]) and (packed[:, 20:] == 0).all()
            rest = torch.ones(ROW, dtype=torch.bool, device=gpu_device)
            rest[live] = False
            assert (full[:, rest] == 0).all()
