"""The top layer's backward target pass inside the block forward launch (`wide::fwd_narrow_block_kernel<., ., TOP>`, DESIGN.md section 5;
`gadapt_block_forward_loss_narrow_top` + `gadapt_block_backward_narrow_packed_below_top`) against the launch it replaces
(`gadapt_debug_set_narrow_top_in_forward(0)`: `grand_bwd_target_narrow_kernel` as the first launch of the backward), in one process.
The fused lane runs that kernel's statements on operands its forward still holds, so everything is compared with `torch.equal`.

C-ABI level, per case, switch on / off / on again, two consecutive steps each from the same state, on NaN-poisoned buffers:
  after the forward call   every [N,4] slot, alpha, the head rows, the seed, the loss partials, the coefficients; and - where the top
                           pass ran in it - dxd, the {alpha dt, ds} pairs in the buffer the next launch reads, and every row of the packed
                           slab (32 entries; rows without nodes zero) against what `grand_bwd_target_narrow_kernel` ALONE leaves: the
                           top two layers as a block with one conv per layer (`gadapt_block_backward_narrow`, a_stride != 0), where each
                           layer has a slab of its own and nothing below the top layer writes dxd or pairs;
  after the backward call  dxd, both edge buffers, the gradient work buffers, every slab row;
  after the tail           the flat gradient, the parameters, both moments, the step count, the loss.
Ineligible cases (no registered halo, more than 131072 nodes) must report that the old launches ran, and still be equal."""
import pytest
import torch

import narrow_graphs as ng
from helpers import hip_model_like
from test_gpu_narrow_tail import LIVE, PACKED, ROW
from g_adaptivity_amd import GNN, MeshDataset, collate, hot_path_opt, mse_loss, unit_gradient
from g_adaptivity_amd import graph as graph_mod
from g_adaptivity_amd.functional import BlockForwardCall
from g_adaptivity_amd.optim import FlatAdam
from g_adaptivity_amd._native import current_stream, lib, ptr

C_ = 64
NAN = float('nan')


def _patch(monkeypatch, half_max=None):
    import g_adaptivity_amd.functional as Fn_mod
    monkeypatch.setattr(Fn_mod, 'SMALL_MESH_FORWARD', False)
    monkeypatch.setattr(graph_mod, 'WIDE_MIN_NODES', 0)
    if half_max is not None:
        monkeypatch.setattr(graph_mod, 'WIDE_HALF_MAX_NODES', half_max)


def _square(gpu_device, mesh_n, batch, layers, monkeypatch):
    """A square-mesh batch, its model and a FlatAdam whose bucket is laid out (lr 1e-3: the steps move the weights)."""
    _patch(monkeypatch)
    opt = hot_path_opt(mesh_dims=[mesh_n, mesh_n], hidden_dim=64, num_layers=layers, lr=1e-3, device=str(gpu_device), show_mesh_evol_plots='False')
    ds = MeshDataset([mesh_n, mesh_n], batch, seed=11)
    data = collate(ds.samples).to(gpu_device)
    torch.manual_seed(12)
    model = GNN(ds, opt).to(gpu_device).train()
    optim = FlatAdam(model.parameters(), lr=0.0, capturable=True)
    optim.zero_grad(); mse_loss(model(data), data.x_phys).backward(gradient=unit_gradient(gpu_device)); optim.step()   # lays the bucket out
    optim.param_groups[0]['lr'] = 1e-3
    return model, optim, data


class Harness:
    """One fused step of the narrow route straight over the C-ABI: the forward call given the backward's buffers, the backward entry
    point that its report selects, and (`optim` given) the one-launch tail.  `d_loss`: loss columns, where fewer than the model's."""

    def __init__(self, model, data, l1=False, optim=None, d_loss=None):
        dev = data.x_comp.device
        xc = data.x_comp if data.x_comp.dim() == 2 else data.x_comp.unsqueeze(-1)
        o = model.opt
        self.graph = g = model._graph(data, xc.shape[0], dev)
        f, uu = (data.f_tensor if o['gnn_inc_feat_f'] else None), (data.uu_tensor if o['gnn_inc_feat_uu'] else None)
        tgt = ng.target_of(data).contiguous()
        self.n, self.e, self.L = g.num_nodes, g.num_edges, int(o['num_layers'])
        self.fwd = fw = BlockForwardCall(model, g, tgt, l1, None, store=False, narrow=True)
        assert g.narrow_route(C_)
        f32 = dict(device=dev, dtype=torch.float32)
        n, e = self.n, max(self.e, 1)
        self.g_ws, self.dxd_ws, self.edge_ws = torch.empty(2, n, C_, **f32), torch.empty(n, C_, **f32), torch.empty(e, 2, **f32)
        self.rows = lib().gadapt_backward_slab_rows(n, C_)
        self.slab = torch.empty(self.rows, PACKED, **f32)
        fw.with_backward_buffers(self.dxd_ws, self.edge_ws, self.slab)
        self.d = fw.d
        if d_loss is not None and d_loss != fw.d:                           # fewer loss columns than coordinates
            self.d = d_loss
            self.tgt_d, self.seed_d = tgt[:, :d_loss].contiguous(), torch.empty(n, d_loss, **f32)
            fw.args[13], fw.args[14], fw.args[16] = ptr(self.tgt_d), d_loss, ptr(self.seed_d)
            fw.seed = self.seed_d
        self._in = (ptr(xc), ptr(f), ptr(uu))
        self.dev, self.optim = dev, optim
        a, p0 = fw.coeffs
        self.bw = [g.c_ref, ptr(fw.x_all), 4, ptr(fw.alpha), ptr(fw.seed), self.d, self.L, ptr(a), 0, ptr(p0), 0, ptr(fw.lp), ptr(self.g_ws),
                   ptr(self.dxd_ws), ptr(self.edge_ws), ptr(self.slab), None, 0, None, C_, None]
        # the reference of the top pass alone: the top two layers as a block with one conv per layer, on buffers of its own
        self.r_g, self.r_dxd, self.r_edge = torch.empty_like(self.g_ws), torch.empty_like(self.dxd_ws), torch.empty_like(self.edge_ws)
        self.r_slab = torch.empty(2, self.rows, ROW, **f32)
        self.r_a, self.r_p0 = torch.empty(2, C_, C_, **f32), torch.empty(2, C_, **f32)
        if optim is not None:
            self.flat, self.loss = torch.empty(2 * C_ * C_ + 2 * C_, **f32), torch.zeros((), **f32)
            self.scratch = torch.empty(32 * ROW, **f32)
            self.saved = [t.clone() for t in (optim.bucket, optim.exp_avg, optim.exp_avg_sq, optim._dev_state)]

    def restore(self):
        o = self.optim
        if o is not None:
            for t, s in zip((o.bucket, o.exp_avg, o.exp_avg_sq, o._dev_state), self.saved):
                t.copy_(s)
        if not self.fwd.in_forward:
            self.fwd.compute_coeffs(current_stream(self.dev))

    def top_alone(self):
        """dxd, pairs and packed slab rows as `grand_bwd_target_narrow_kernel` alone leaves them for the forward state now in the buffers."""
        fw, L, n = self.fwd, self.L, self.n
        a, p0 = fw.coeffs
        self.r_a.copy_(a.reshape(1, C_, C_).expand(2, C_, C_)); self.r_p0.copy_(p0.reshape(1, C_).expand(2, C_))
        for t in (self.r_g, self.r_dxd, self.r_edge, self.r_slab):
            t.fill_(NAN)
        args = [self.graph.c_ref, fw.x_all.data_ptr() + 4 * (L - 2) * n * C_, 4, fw.alpha.data_ptr() + 4 * (L - 2) * fw.alpha.shape[1],
                ptr(fw.seed), self.d, 2, ptr(self.r_a), C_ * C_, ptr(self.r_p0), C_, fw.lp.data_ptr() + 4 * 2 * (L - 2), ptr(self.r_g), ptr(self.r_dxd),
                ptr(self.r_edge), ptr(self.r_slab), None, 0, None, C_, current_stream(self.dev)]
        assert lib().gadapt_block_backward_narrow(*args) == 0
        torch.cuda.synchronize()
        top = self.r_slab[1]
        rest = torch.ones(ROW, dtype=torch.bool, device=self.dev)
        rest[LIVE.to(self.dev)] = False
        assert not torch.isnan(top).any() and (top[:, rest] == 0).all()
        packed = torch.zeros(self.rows, PACKED, device=self.dev)
        packed[:, :20] = top[:, LIVE.to(self.dev)]
        return dict(dxd=self.r_dxd.view(-1)[:4 * n].clone(), pairs=self.r_edge.view(-1)[:2 * self.e].clone(), slab=packed)

    def run(self, on, steps=2):
        """`steps` consecutive steps from the saved state with the switch `on`; per step what each call leaves, and whether the top pass
        ran in the forward."""
        fw, n, e, L, st = self.fwd, self.n, self.e, self.L, current_stream(self.dev)
        lib().gadapt_debug_set_narrow_top_in_forward(on)
        out = []
        try:
            self.restore()
            for _ in range(steps):
                for t in (fw.x_all, fw.x_top4, fw.alpha, fw.seed, self.g_ws, self.dxd_ws, self.edge_ws, self.slab):
                    t.fill_(NAN)
                fw.partials.zero_()
                n_part = fw(*self._in, st)
                torch.cuda.synchronize()
                assert 0 < n_part <= lib().gadapt_loss_partials_max()
                ran = fw.top_ran
                s = dict(ran=ran, n_part=n_part)
                s['slots'] = fw.x_all.view(L, -1)[:, :4 * n].clone()
                s['alpha'], s['top'], s['seed'], s['partials'] = fw.alpha[:, :e].clone(), fw.x_top4.clone(), fw.seed.clone(), fw.partials[:n_part].clone()
                s['a'], s['p0'] = fw.coeffs[0].clone(), fw.coeffs[1].clone()
                if ran:
                    s['f_dxd'], s['f_pairs'], s['f_slab'] = self.dxd_ws.view(-1)[:4 * n].clone(), self.edge_ws.view(-1)[:2 * e].clone(), self.slab.clone()
                    assert torch.isnan(self.dxd_ws.view(-1)[4 * n:]).all() and torch.isnan(self.g_ws).all()      # nothing else was touched
                else:
                    assert torch.isnan(self.dxd_ws).all() and torch.isnan(self.edge_ws).all() and torch.isnan(self.slab).all()
                    s['alone'] = self.top_alone()
                self.bw[-1] = st
                fn = lib().gadapt_block_backward_narrow_packed_below_top if ran else lib().gadapt_block_backward_narrow_packed
                assert fn(*self.bw) == 0
                torch.cuda.synchronize()
                s['b_slab'], s['b_dxd'], s['b_edge'], s['b_g'] = self.slab.clone(), self.dxd_ws.clone(), self.edge_ws.clone(), self.g_ws.clone()
                assert not torch.isnan(s['b_slab']).any()
                if self.optim is not None:
                    o = self.optim
                    self.flat.fill_(NAN)
                    args = [ptr(self.slab), self.rows, ptr(self.scratch), ptr(o.bucket), ptr(self.flat), ptr(o.exp_avg), ptr(o.exp_avg_sq), 1e-3, 0.9,
                            0.999, 1e-8, 0.0, ptr(o._dev_state), 1.0, None if fw.in_forward else ptr(fw.coeffs[0]),
                            None if fw.in_forward else ptr(fw.coeffs[1]), ptr(fw.partials), n_part, ptr(self.loss), n * self.d, C_, st]
                    assert lib().gadapt_step_tail_narrow(*args) == 0
                    torch.cuda.synchronize()
                    s['flat'], s['param'], s['m'], s['v'] = self.flat.clone(), o.bucket.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone()
                    s['state'], s['loss'] = o._dev_state.clone(), self.loss.clone()
                    assert not torch.isnan(s['flat']).any() and s['flat'].abs().max().item() > 0
                out.append(s)
        finally:
            lib().gadapt_debug_set_narrow_top_in_forward(1)
            self.restore()
        return out


def _same(x, y, what):
    def eq(a, b):                                                       # (bitwise: buffers may hold NaN poison in parts no launch writes)
        return a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    bad = [k for k in x if k in y and torch.is_tensor(x[k]) and not eq(x[k], y[k])]
    assert not bad, (what, bad)


def _check(h, expect_ran, steps=2):
    """on / off / on: the reports, then every stored value."""
    rows, busy = h.rows, -(-h.n // 256)
    on, off, again = h.run(1, steps), h.run(0, steps), h.run(1, steps)
    for k in range(steps):
        a, b, c = on[k], off[k], again[k]
        assert a['ran'] == c['ran'] == expect_ran and not b['ran'], (k, a['ran'], b['ran'])
        assert a['n_part'] == b['n_part']
        for key in ('slots', 'alpha', 'top', 'seed'):
            assert not torch.isnan(a[key]).any(), key
        _same(a, c, ('two runs with the switch on', k))
        _same(a, b, ('switch on against off', k))
        if expect_ran:
            alone = b['alone']
            assert torch.equal(a['f_dxd'], alone['dxd']) and not torch.isnan(a['f_dxd']).any(), k
            assert torch.equal(a['f_pairs'], alone['pairs']) and not torch.isnan(a['f_pairs']).any(), k
            assert not torch.isnan(a['f_slab']).any()
            assert torch.equal(a['f_slab'], alone['slab']), (k, (a['f_slab'] != alone['slab']).nonzero()[:8].tolist())
            assert (a['f_slab'][:, 20:] == 0).all() and (a['f_slab'][busy:] == 0).all()
            assert (a['f_slab'][:busy, :20].abs().amax(dim=1) > 0).all()
    if h.optim is not None:
        before = int(h.saved[3][0])                                      # (the step that laid the bucket out counted too)
        assert [int(s['state'][0]) - before for s in on] == list(range(1, steps + 1))
        assert not torch.equal(on[0]['param'], on[1]['param'])           # the second step ran on other weights


# (mesh side, batch, layers, loss, loss columns): 16 x 16 b1 - one tile, 8 slab rows of which 7 are empty; 23 x 23 b7 - ragged, last
# tile and last row with nodes partly filled; 32 x 32 b3 - halo 32; 64 x 64 b2 - fewer than 64 tiles, coefficients given; 64 x 64 b16 -
# 64 tiles, in-kernel coefficients; 2, 3 and 6 layers (6: two groups, the second carries the pass); l1 loss; one loss column
SHAPES = [(16, 1, 4, 'mse', 2), (23, 7, 4, 'mse', 2), (32, 3, 4, 'mse', 2), (64, 2, 4, 'mse', 2), (64, 16, 4, 'mse', 2),
          (23, 7, 2, 'mse', 2), (23, 7, 3, 'mse', 2), (23, 7, 6, 'mse', 2), (23, 7, 4, 'l1', 2), (23, 7, 4, 'mse', 1), (23, 7, 2, 'l1', 1)]
SHAPE_IDS = ['16x16-b1-one-tile', '23x23-b7-ragged', '32x32-b3-halo-32', '64x64-b2-coefficients-given', '64x64-b16-in-kernel-coefficients',
             '23x23-b7-2-layers', '23x23-b7-3-layers', '23x23-b7-6-layers-two-groups', '23x23-b7-l1', '23x23-b7-one-loss-column',
             '23x23-b7-2-layers-l1-one-loss-column']


@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("mesh_n,batch,layers,loss,d_loss", SHAPES, ids=SHAPE_IDS)
def test_step_with_the_top_pass_in_the_forward_launch(gpu_device, mesh_n, batch, layers, loss, d_loss, monkeypatch):
    model, optim, data = _square(gpu_device, mesh_n, batch, layers, monkeypatch)
    h = Harness(model, data, l1=(loss == 'l1'), optim=optim, d_loss=d_loss)
    halo = lib().gadapt_narrow_block_halo(h.graph.c_ref, C_)
    assert halo == (64 if mesh_n == 64 else 32)
    tiles = -(-h.n // 512)
    assert (mesh_n, batch) != (64, 16) or (tiles == 128 and h.fwd.in_forward)   # the layer-0 launch computes A itself: a4 from its sums
    assert (mesh_n, batch) != (64, 2) or tiles == 16                            # ... and here from the coefficient launch's A
    assert (mesh_n, batch) != (16, 1) or (tiles == 1 and h.rows == 8)
    _check(h, expect_ran=True)


@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("case_id", ng.IDS)
def test_graphs_of_the_narrow_route(gpu_device, case_id, monkeypatch):
    """Ragged rows (in-rows of 0 .. 8), self-loops, mixed mesh sizes, 1-D meshes (one coordinate, one loss column): the pass runs in the
    forward wherever the block launch does; the 512-row window has no halo and keeps the old launches.  Equal either way."""
    b = ng.build(case_id)
    c = b.case
    _patch(monkeypatch, c.half_max)
    model = hip_model_like(b.oracle, b.ds, b.opt, gpu_device).train()
    data = b.data.clone().to(gpu_device)
    h = Harness(model, data)
    assert h.n == c.nodes
    halo = lib().gadapt_narrow_block_halo(h.graph.c_ref, C_)
    assert (halo == 0) == c.big
    _check(h, expect_ran=not c.big)


@pytest.mark.gpu
@pytest.mark.one_dispatch
def test_switch_and_missing_buffers_keep_the_old_launches(gpu_device, monkeypatch):
    model, optim, data = _square(gpu_device, 23, 7, 3, monkeypatch)
    h = Harness(model, data, optim=optim)
    st = current_stream(h.dev)
    for k in (18, 19, 20):                                              # dxd_ws, edge_ws, slab
        args = list(h.fwd.args)
        args[2], args[4], args[5], args[-1] = *h._in, st
        args[k] = None
        h.dxd_ws.fill_(NAN); h.edge_ws.fill_(NAN); h.slab.fill_(NAN)
        assert lib().gadapt_block_forward_loss_narrow_top(*args) > 0
        torch.cuda.synchronize()
        assert not h.fwd.top_ran
        assert torch.isnan(h.dxd_ws).all() and torch.isnan(h.edge_ws).all() and torch.isnan(h.slab).all()
    args = list(h.fwd.args)
    args[2], args[4], args[5], args[-1] = *h._in, st
    args[21] = None                                                      # nowhere to report
    assert lib().gadapt_block_forward_loss_narrow_top(*args) == -1 and b'top' in lib().gadapt_last_error()


@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("mesh_n,batch", [(23, 7), (64, 2)], ids=['23x23-b7', '64x64-b2'])
def test_fused_iteration_three_steps(gpu_device, mesh_n, batch, monkeypatch):
    """`FusedIteration` takes the new calls: parameters, moments and step count after three steps are equal with the switch on and off."""
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
        lib().gadapt_debug_set_narrow_top_in_forward(on)
        try:
            for _ in range(3):
                for t in (it.slab, it.g_ws, it.dxd_ws, it.edge_ws, it.flat):
                    t.fill_(NAN)
                it.run()
                assert it.fwd.top_ran == bool(on)
            torch.cuda.synchronize()
        finally:
            lib().gadapt_debug_set_narrow_top_in_forward(1)
        got[on] = [t.clone() for t in (optim.bucket, optim.exp_avg, optim.exp_avg_sq, optim._dev_state, it.flat, it.loss, it.out)]
    for t, s in zip((optim.bucket, optim.exp_avg, optim.exp_avg_sq, optim._dev_state), saved):
        t.copy_(s)
    optim.step_count -= 6
    assert got[1][3].tolist()[0] == saved[3].tolist()[0] + 3
    assert not torch.equal(got[1][0], saved[0]) and not torch.isnan(got[1][0]).any()
    for a, b, name in zip(got[1], got[0], ('param', 'exp_avg', 'exp_avg_sq', 'state', 'flat', 'loss', 'out')):
        assert torch.equal(a, b), name
