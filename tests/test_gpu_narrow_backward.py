"""The narrow route's backward: `grand_bwd_target_fused_narrow_kernel` - the source pass of each layer inside the
target pass of the layer below, the default - against the pair of launches per layer (`gadapt_debug_set_narrow_backward_fused(0)`), in
one process and from identical parameters, through `FusedIteration.forward_backward()`.  The arithmetic and its order are the same, so
everything is bit-identical: the slab rows after the backward, the flat gradient after `finish()`, `out` and `loss`.  The fused launches
read one layer's {alpha dt, ds} pairs while they scatter the next layer's into a second buffer; a race there would show as slabs that
differ between two runs on the same inputs."""
import ctypes as C

import pytest
import torch

from g_adaptivity_amd import GNN, MeshDataset, collate, hot_path_opt, mse_loss, unit_gradient
from g_adaptivity_amd import graph as graph_mod
from g_adaptivity_amd.optim import FlatAdam
from g_adaptivity_amd._native import lib

# (mesh side, batch, layers).  23x23 b7: N = 3703 is no multiple of 256 (a partial last workgroup), boundary rows of low degree.
# 64x64 b32: N = 512 x 256, every workgroup of the capped grid full, one node per lane; b33: the smallest batch past the cap - lanes take
# a second grid-stride step.  2 layers: the only fused launch is the layer-0 form and its source half reads the compact top gradient.
# 3 layers: one ping-pong of the edge buffers.
CASES = [(23, 7, 4), (64, 3, 4), (64, 32, 4), (64, 33, 4), (23, 7, 2), (23, 7, 3)]
IDS = ['23x23-b7-ragged', '64x64-b3', '64x64-b32-full-grid', '64x64-b33-two-grid-stride-steps', '23x23-b7-2-layers', '23x23-b7-3-layers']


def _setup(gpu_device, mesh_n, batch, layers, monkeypatch):
    import g_adaptivity_amd.functional as Fn_mod
    from g_adaptivity_amd.training import FusedIteration
    monkeypatch.setattr(Fn_mod, 'SMALL_MESH_FORWARD', False)
    monkeypatch.setattr(graph_mod, 'WIDE_MIN_NODES', 0)
    opt = hot_path_opt(mesh_dims=[mesh_n, mesh_n], hidden_dim=64, num_layers=layers, lr=0.0, device=str(gpu_device), show_mesh_evol_plots='False')
    ds = MeshDataset([mesh_n, mesh_n], batch, seed=11)
    data = collate(ds.samples).to(gpu_device)
    torch.manual_seed(12)
    model = GNN(ds, opt).to(gpu_device).train()
    optim = FlatAdam(model.parameters(), lr=0.0, capturable=True)
    optim.zero_grad(); mse_loss(model(data), data.x_phys).backward(gradient=unit_gradient(gpu_device)); optim.step()   # lays the bucket out
    assert FusedIteration.eligible(model, optim, mse_loss, data, 'x_phys') is None
    it = FusedIteration(model, optim, mse_loss, data, 'x_phys')
    assert it.fwd.narrow, "the case must take the narrow route"
    it.refresh_coeffs()
    return model, optim, it


def _source_launches():
    tot, cnt = C.c_double(0.0), C.c_int(0)
    lib().gadapt_profile_read(2, C.byref(tot), C.byref(cnt))
    return cnt.value


def _step(it, optim, fused):
    """One forward + backward + tail with the switch set, on poisoned work buffers and from the same optimizer state; returns what the
    step leaves (lr = 0: the parameters stay) and the number of source-pass launches it made."""
    state = (optim.exp_avg.clone(), optim.exp_avg_sq.clone(), optim._dev_state.clone(), optim.step_count)
    lib().gadapt_debug_set_narrow_backward_fused(fused)
    lib().gadapt_profile_reset(); lib().gadapt_profile_enable(1)
    try:
        for t in (it.slab, it.g_ws, it.dxd_ws, it.edge_ws, it.flat):
            t.fill_(float('nan'))
        it.forward_backward()
        torch.cuda.synchronize()
        n_source = _source_launches()
        slab = it.slab.clone()
        it.finish()
        torch.cuda.synchronize()
    finally:
        lib().gadapt_profile_enable(0); lib().gadapt_profile_reset()
        lib().gadapt_debug_set_narrow_backward_fused(1)
    rec = dict(slab=slab, flat=it.flat.clone(), out=it.out.clone(), loss=it.loss.clone(), n_source=n_source)
    optim.exp_avg.copy_(state[0]); optim.exp_avg_sq.copy_(state[1]); optim._dev_state.copy_(state[2]); optim.step_count = state[3]
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize("mesh_n,batch,layers", CASES, ids=IDS)
def test_fused_narrow_backward_equals_the_pair(gpu_device, mesh_n, batch, layers, monkeypatch):
    model, optim, it = _setup(gpu_device, mesh_n, batch, layers, monkeypatch)
    n, e = it.n, it.graph.num_edges
    assert 2 * e <= 60 * n, "the second edge buffer must fit the tail of dxd_ws, or the pairs run and the case checks nothing"
    # the grid of every target-pass launch is the slab row count: one node per lane up to 512 workgroups, a second step beyond
    assert (it.slab_rows * 256 < n) == ((mesh_n, batch) == (64, 33))
    if (mesh_n, batch) == (64, 32):
        assert it.slab_rows * 256 == n
    new, new2, old = _step(it, optim, 1), _step(it, optim, 1), _step(it, optim, 0)
    # the switch selects the launches: L-1 source passes per backward with the pairs, none fused
    assert new['n_source'] == 0 and new2['n_source'] == 0 and old['n_source'] == layers - 1
    for k in ('slab', 'flat', 'out'):
        assert not torch.isnan(new[k]).any(), k
    # no race on the edge buffers: the same inputs give the same bits
    assert torch.equal(new['slab'], new2['slab']) and torch.equal(new['flat'], new2['flat'])
    for k in ('slab', 'flat', 'out', 'loss'):
        assert torch.equal(new[k], old[k]), (k, (new[k] - old[k]).abs().max().item())
    assert new['flat'].abs().max().item() > 0
