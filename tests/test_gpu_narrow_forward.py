"""The narrow route's forward layers: `wide::fwd_narrow_kernel` (one node per lane on the [N,4] rows, the default)
against `wide::fwd_kernel<XC = true>` (`gadapt_debug_set_narrow_forward(0)`), in one process.  Every stored value is bit-identical: the
[N,4] layer slots, alpha, the layer-0 input rows, the head rows, the loss derivative and the composite coefficients the layer-0 launch
computes; the loss value agrees to rounding (its partial sums are grouped by wave, and the waves differ)."""
import pytest
import torch
import torch.nn.functional as F

from g_adaptivity_amd import GNN, MeshDataset, collate, hot_path_opt, mse_loss, unit_gradient
from g_adaptivity_amd import graph as graph_mod
from g_adaptivity_amd.optim import FlatAdam
from g_adaptivity_amd._native import lib

# (mesh side, batch, weight scale, layer 0 computes the coefficients): only batches on 256-node steps take them from the weights
CASES = [(64, 32, 1.0, True), (23, 7, 1.0, False), (32, 32, 1.0, False), (128, 2, 1.0, True), (64, 16, 4.0, True)]
IDS = ['64x64-b32-several-steps', '23x23-b7-ragged', '32x32-b32-four-wave-geometry', '128x128-b2-big-window', '64x64-b16-rebase']


def _setup(gpu_device, mesh_n, batch, scale, monkeypatch):
    import g_adaptivity_amd.functional as Fn_mod
    from g_adaptivity_amd.training import FusedIteration
    monkeypatch.setattr(Fn_mod, 'SMALL_MESH_FORWARD', False)
    monkeypatch.setattr(graph_mod, 'WIDE_MIN_NODES', 0)
    opt = hot_path_opt(mesh_dims=[mesh_n, mesh_n], hidden_dim=64, num_layers=4, lr=0.0, device=str(gpu_device), show_mesh_evol_plots='False')
    ds = MeshDataset([mesh_n, mesh_n], batch, seed=11)
    data = collate(ds.samples).to(gpu_device)
    torch.manual_seed(12)
    model = GNN(ds, opt).to(gpu_device).train()
    with torch.no_grad():                                           # scale > 1: scores spread far enough for the softmax to re-base
        model.conv_layers[0].lin_query.weight.mul_(scale)
        model.conv_layers[0].lin_key.weight.mul_(scale)
    optim = FlatAdam(model.parameters(), lr=0.0, capturable=True)
    optim.zero_grad(); mse_loss(model(data), data.x_phys).backward(gradient=unit_gradient(gpu_device)); optim.step()   # lays the bucket out
    assert FusedIteration.eligible(model, optim, mse_loss, data, 'x_phys') is None
    it = FusedIteration(model, optim, mse_loss, data, 'x_phys')
    assert it.fwd.narrow, "the case must take the narrow route"
    it.refresh_coeffs()
    return model, data, it


def _forward_once(it, on):
    """One `gadapt_block_forward_loss_narrow` call on poisoned buffers; returns every value it stores."""
    f = it.fwd
    n, L = f.n, f.L
    lib().gadapt_debug_set_narrow_forward(on)
    try:
        f.x_all.fill_(float('nan')); f.x_top4.fill_(float('nan')); f.alpha.fill_(float('nan')); f.seed.fill_(float('nan'))
        f.partials.zero_()
        if f.in_forward:                                            # outputs of the layer-0 launch
            f.coeffs[0].fill_(float('nan')); f.coeffs[1].fill_(float('nan'))
        n_part = f(*it._in, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        lib().gadapt_debug_set_narrow_forward(1)
    assert 0 < n_part <= lib().gadapt_loss_partials_max()
    slots = f.x_all.view(L, -1)[:, :4 * n].reshape(L, n, 4).clone()    # slot l: the [N,4] rows at its start (slot 0: the layer-0 input)
    return dict(slots=slots, top=f.x_top4.clone(), alpha=f.alpha[:, :it.graph.num_edges].clone(), seed=f.seed.clone(),
                a=f.coeffs[0].clone(), p0=f.coeffs[1].clone(), loss=f.partials[:n_part].double().sum().item(), in_forward=f.in_forward)


@pytest.mark.gpu
@pytest.mark.parametrize("mesh_n,batch,scale,computes", CASES, ids=IDS)
def test_narrow_forward_equals_wide_forward(gpu_device, mesh_n, batch, scale, computes, monkeypatch):
    model, data, it = _setup(gpu_device, mesh_n, batch, scale, monkeypatch)
    new, old = _forward_once(it, 1), _forward_once(it, 0)
    assert not torch.isnan(new['slots']).any() and not torch.isnan(new['alpha']).any() and not torch.isnan(new['seed']).any()
    for k in ('slots', 'top', 'alpha', 'seed', 'a', 'p0'):
        assert torch.equal(new[k], old[k]), k
    assert abs(new['loss'] - old['loss']) <= 1e-6 * abs(old['loss']), (new['loss'], old['loss'])
    assert new['in_forward'] == computes
    if scale > 1.0:
        # the case is what it claims: many rows whose first weight is at most e^-16 of another one (the softmax re-based in layer 0)
        rp = it.graph.rowptr_t.long()
        a0 = new['alpha'][0]
        first = a0[rp[:-1][rp[1:] > rp[:-1]]]
        assert (first < 1.2e-7).sum().item() > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("mesh_n,batch,scale,computes", [CASES[0], CASES[2], CASES[3], CASES[4]], ids=[IDS[0], IDS[2], IDS[3], IDS[4]])
def test_narrow_forward_autograd_path(gpu_device, mesh_n, batch, scale, computes, monkeypatch):
    """`model(data)` on the narrow route (gadapt_block_forward_narrow, coefficients given) and its backward: output and every weight
    gradient bit-identical with either forward kernel."""
    model, data, _ = _setup(gpu_device, mesh_n, batch, scale, monkeypatch)

    def run(on):
        lib().gadapt_debug_set_narrow_forward(on)
        try:
            model.zero_grad()
            out = model(data)
            F.mse_loss(out, data.x_phys).backward()
            torch.cuda.synchronize()
        finally:
            lib().gadapt_debug_set_narrow_forward(1)
        return out.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    (o1, g1), (o0, g0) = run(1), run(0)
    assert torch.equal(o1, o0)
    assert set(g1) == set(g0) and g1
    for k in g1:
        assert torch.equal(g1[k], g0[k]), k
