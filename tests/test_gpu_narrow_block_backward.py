"""The narrow route's backward layers below the top in one launch (`grand_bwd_narrow_block_kernel`, DESIGN.md section 5;
`gadapt_block_backward_narrow_packed_block`) against the launches it replaces (`gadapt_block_backward_narrow_packed` /
`..._packed_below_top`), in one process.  Every stage runs the fused kernel's statements on the same operands and the slab rows are
summed in the same order, so everything is compared as int32 patterns with `torch.equal`.

C-ABI level, driven through the harness of test_gpu_narrow_top_in_forward.py.  Per case: both `top_done` values (the top layer's target
pass in the forward launch, or as the first launch of the backward); the switch on / off / on again; two consecutive steps each from the
same state; every work buffer and the slab NaN-poisoned before each step.  In a step, the forward runs once; from its state
  the reference call    leaves the slab (all 32 entries of every row, rows without nodes included) and the work buffers;
  the new entry point   runs from the same state twice: equal bits both times (no race on the LDS buffers), the slab equal to the
                        reference's, and everything include/gadapt_hip.h says it does not write still as the forward left it (poison,
                        or what T_{L-1} wrote); at a group boundary (6 layers) the g rows and pairs the next launch reads are the
                        reference's (its dxd rows are not comparable: the reference overwrites them in place one launch later - they
                        are checked through the slab rows the second group computes from them);
  the tail              flat gradient, parameters, both moments, step count and loss, equal across the switch positions."""
import ctypes

import pytest
import torch

import narrow_graphs as ng
from helpers import hip_model_like
from test_gpu_narrow_top_in_forward import C_, NAN, Harness, _patch, _same, _square
from g_adaptivity_amd import mse_loss
from g_adaptivity_amd._native import current_stream, lib, ptr


def _bits(t):
    return t.contiguous().view(torch.int32)


def _eq(a, b):
    return torch.equal(_bits(a), _bits(b))


def _run(h, block_on, top_in_fwd, steps=2):
    """`steps` consecutive steps from the saved state; per step the report, the slab and what the tail leaves."""
    fw, n, e, L, st = h.fwd, h.n, h.e, h.L, current_stream(h.dev)
    ws = (h.g_ws, h.dxd_ws, h.edge_ws, h.slab)
    ran = ctypes.c_int(-1)
    tiles_rows = min(2 * -(-n // 512), h.rows)
    out = []
    lib().gadapt_debug_set_narrow_top_in_forward(top_in_fwd)
    lib().gadapt_debug_set_narrow_backward_block(block_on)
    try:
        h.restore()
        for _ in range(steps):
            for t in (fw.x_all, fw.x_top4, fw.alpha, fw.seed) + ws:
                t.fill_(NAN)
            fw.partials.zero_()
            n_part = fw(*h._in, st)
            torch.cuda.synchronize()
            top_done = 1 if fw.top_ran else 0
            assert top_done == top_in_fwd
            before = [t.clone() for t in ws]
            # ---- the launches it replaces
            h.bw[-1] = st
            ref_fn = lib().gadapt_block_backward_narrow_packed_below_top if top_done else lib().gadapt_block_backward_narrow_packed
            assert ref_fn(*h.bw) == 0
            torch.cuda.synchronize()
            ref = [t.clone() for t in ws]
            assert not torch.isnan(ref[3]).any()
            # ---- the new entry point, twice from the same state
            got = []
            for _rep in range(2):
                for t, b in zip(ws, before):
                    t.copy_(b)
                ran.value = -1
                assert lib().gadapt_block_backward_narrow_packed_block(*h.bw, top_done, ctypes.addressof(ran)) == 0
                torch.cuda.synchronize()
                got.append([t.clone() for t in ws])
            assert all(_eq(a, b) for a, b in zip(got[0], got[1])), 'two runs from the same state differ'
            g_ws, dxd, edge, slab = got[0]
            assert _eq(slab, ref[3]), ('slab', (_bits(slab) != _bits(ref[3])).nonzero()[:8].tolist())
            s = dict(ran=ran.value, slab=slab)
            if ran.value:
                dflat, bflat = dxd.view(-1), before[1].view(-1)
                if top_done:                                           # the block launches write slab entries 0..19 of the tiles' rows only
                    assert _eq(slab[tiles_rows:], before[3][tiles_rows:]) and _eq(slab[:, 20:], before[3][:, 20:])
                    assert _eq(dflat[:4 * n], bflat[:4 * n]) and _eq(edge, before[2])
                assert (slab[tiles_rows:] == 0).all() and (slab[:, 20:] == 0).all()
                if L <= 4:
                    assert torch.isnan(g_ws).all() and torch.isnan(dflat[4 * n:]).all()
                else:                                                  # 6 layers: 3 + 2, one boundary
                    assert L == 6
                    assert _eq(g_ws[0].view(-1)[:4 * n], ref[0][0].view(-1)[:4 * n]) and not torch.isnan(g_ws[0].view(-1)[:4 * n]).any()
                    assert torch.isnan(g_ws[0].view(-1)[4 * n:]).all() and torch.isnan(g_ws[1]).all()
                    assert _eq(dflat[4 * n:4 * n + 2 * e], ref[1].view(-1)[4 * n:4 * n + 2 * e])      # the pairs of the second edge buffer
                    assert not torch.isnan(dflat[4 * n + 2 * e:8 * n + 2 * e]).any() and torch.isnan(dflat[8 * n + 2 * e:]).all()
            else:                                                      # exactly the old launches
                assert all(_eq(a, b) for a, b in zip(got[0], ref))
            if h.optim is not None:
                o = h.optim
                h.flat.fill_(NAN)
                args = [ptr(h.slab), h.rows, ptr(h.scratch), ptr(o.bucket), ptr(h.flat), ptr(o.exp_avg), ptr(o.exp_avg_sq), 1e-3, 0.9,
                        0.999, 1e-8, 0.0, ptr(o._dev_state), 1.0, None if fw.in_forward else ptr(fw.coeffs[0]),
                        None if fw.in_forward else ptr(fw.coeffs[1]), ptr(fw.partials), n_part, ptr(h.loss), n * h.d, C_, st]
                assert lib().gadapt_step_tail_narrow(*args) == 0
                torch.cuda.synchronize()
                s['flat'], s['param'], s['m'], s['v'] = h.flat.clone(), o.bucket.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone()
                s['state'], s['loss'] = o._dev_state.clone(), h.loss.clone()
                assert not torch.isnan(s['flat']).any() and s['flat'].abs().max().item() > 0
            out.append(s)
    finally:
        lib().gadapt_debug_set_narrow_top_in_forward(1)
        lib().gadapt_debug_set_narrow_backward_block(1)
        h.restore()
    return out


def _check(h, expect_ran, top_values=(1, 0), steps=2):
    for top in top_values:
        on, off, again = _run(h, 1, top, steps), _run(h, 0, top, steps), _run(h, 1, top, steps)
        for k in range(steps):
            a, b, c = on[k], off[k], again[k]
            assert (a['ran'], b['ran'], c['ran']) == (int(expect_ran), 0, int(expect_ran)), (top, k, a['ran'], b['ran'], c['ran'])
            _same(a, c, ('two runs with the switch on', top, k))
            _same(a, b, ('switch on against off', top, k))
        if h.optim is not None:
            assert not torch.equal(on[0]['param'], on[1]['param'])           # the second step ran on other weights


# (mesh side, batch, layers, loss): 16 x 16 b1 - one tile, every range clamped at both ends; 23 x 23 b7 - 3703 nodes, a ragged last tile
# and a partial wave; 32 x 32 b3 - halo 32; 64 x 64 b2 - halo 64, interior tiles; 2 layers (no block launch, reported), 3 (two stages),
# 6 (3 + 2 stages: a group boundary through global memory); l1 loss
SHAPES = [(16, 1, 4, 'mse'), (23, 7, 4, 'mse'), (32, 3, 4, 'mse'), (64, 2, 4, 'mse'), (23, 7, 2, 'mse'), (23, 7, 3, 'mse'), (23, 7, 6, 'mse'),
          (64, 2, 3, 'l1'), (64, 2, 6, 'mse'), (23, 7, 4, 'l1'), (16, 1, 6, 'l1')]
SHAPE_IDS = ['16x16-b1-one-tile', '23x23-b7-ragged', '32x32-b3-halo-32', '64x64-b2-halo-64', '23x23-b7-2-layers-old-launches',
             '23x23-b7-3-layers', '23x23-b7-6-layers-two-groups', '64x64-b2-3-layers-l1', '64x64-b2-6-layers-two-groups', '23x23-b7-l1',
             '16x16-b1-6-layers-l1']


@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("mesh_n,batch,layers,loss", SHAPES, ids=SHAPE_IDS)
def test_layers_below_the_top_in_one_launch(gpu_device, mesh_n, batch, layers, loss, monkeypatch):
    model, optim, data = _square(gpu_device, mesh_n, batch, layers, monkeypatch)
    h = Harness(model, data, l1=(loss == 'l1'), optim=optim)
    assert h.graph.narrow_block_halo_source == (64 if mesh_n == 64 else 32)
    assert (mesh_n, batch) != (16, 1) or -(-h.n // 512) == 1
    assert (mesh_n, batch) != (23, 7) or (h.n == 3703 and h.n % 512 % 64 != 0)
    _check(h, expect_ran=layers >= 3)


@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("case_id", ng.IDS)
def test_graphs_of_the_narrow_route(gpu_device, case_id, monkeypatch):
    """Ragged rows, self-loops, mixed mesh sizes, 1-D meshes: the block launch runs where the out-edges have a halo and no row of either
    table is longer than 8; every other graph reports the old launches.  Equal either way."""
    b = ng.build(case_id)
    c = b.case
    _patch(monkeypatch, c.half_max)
    model = hip_model_like(b.oracle, b.ds, b.opt, gpu_device).train()
    data = b.data.clone().to(gpu_device)
    h = Harness(model, data)
    g = h.graph
    assert not (c.big and g.narrow_block_halo_source)
    out_rows = int((g.rowptr_s[1:] - g.rowptr_s[:-1]).max())
    assert not g.narrow_block_halo_source or out_rows <= 8
    expect = g.narrow_block_halo_source in (32, 64) and g.max_in_degree <= 8 and h.L >= 3 and h.e > 0
    _check(h, expect_ran=expect, top_values=(0,) if c.big else (1, 0))


@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("mesh_n,batch", [(23, 7), (64, 2)], ids=['23x23-b7', '64x64-b2'])
def test_fused_iteration_three_steps(gpu_device, mesh_n, batch, monkeypatch):
    """`FusedIteration` calls the new entry point: parameters, moments, step count, flat gradient, loss and output after three steps are
    equal with the switch on and off."""
    from g_adaptivity_amd.training import FusedIteration
    model, optim, data = _square(gpu_device, mesh_n, batch, 4, monkeypatch)
    assert FusedIteration.eligible(model, optim, mse_loss, data, 'x_phys') is None
    it = FusedIteration(model, optim, mse_loss, data, 'x_phys')
    assert it.fwd.narrow
    saved = [t.clone() for t in (optim.bucket, optim.exp_avg, optim.exp_avg_sq, optim._dev_state)]
    got = {}
    for on in (1, 0):
        for t, s in zip((optim.bucket, optim.exp_avg, optim.exp_avg_sq, optim._dev_state), saved):
            t.copy_(s)
        it.refresh_coeffs()
        lib().gadapt_debug_set_narrow_backward_block(on)
        try:
            for _ in range(3):
                for t in (it.slab, it.g_ws, it.dxd_ws, it.edge_ws, it.flat):
                    t.fill_(NAN)
                it.run()
                assert it.fwd.top_ran and it.block_ran.value == on
            torch.cuda.synchronize()
        finally:
            lib().gadapt_debug_set_narrow_backward_block(1)
        got[on] = [t.clone() for t in (optim.bucket, optim.exp_avg, optim.exp_avg_sq, optim._dev_state, it.flat, it.loss, it.out)]
    for t, s in zip((optim.bucket, optim.exp_avg, optim.exp_avg_sq, optim._dev_state), saved):
        t.copy_(s)
    optim.step_count -= 6
    assert got[1][3].tolist()[0] == saved[3].tolist()[0] + 3
    assert not torch.equal(got[1][0], saved[0]) and not torch.isnan(got[1][0]).any()
    for a, b, name in zip(got[1], got[0], ('param', 'exp_avg', 'exp_avg_sq', 'state', 'flat', 'loss', 'out')):
        assert torch.equal(a, b), name
