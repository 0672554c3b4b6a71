"""The narrow route's forward as groups of up to four layers in ONE launch (`wide::fwd_narrow_block_kernel`, DESIGN.md section 5: a
workgroup owns 512 nodes and recomputes the layers below on a halo) against one `wide::fwd_narrow_kernel` launch per layer
(`gadapt_debug_set_narrow_forward(2)`), in one process.  Both run the same per-node statements on the same aligned 32-node groups, so
every stored value is bit-identical: the [N,4] layer slots, alpha, the layer-0 input rows, the head rows, the loss derivative and the
composite coefficients; the loss value agrees to rounding (its partial sums are grouped by wave, and the waves differ).  Every case
asserts through `gadapt_narrow_block_halo` that the default choice really took the block launch (or, on an ineligible graph, did not)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import narrow_graphs as ng
from helpers import hip_model_like
from g_adaptivity_amd import GNN, MeshDataset, collate, hot_path_opt, mse_loss, unit_gradient
from g_adaptivity_amd import graph as graph_mod
from g_adaptivity_amd.optim import FlatAdam
from g_adaptivity_amd._native import lib

# (mesh side, batch, weight scale, layers, halo)
CASES = [(64, 8, 1.0, 4, 64), (64, 16, 4.0, 4, 64), (23, 7, 1.0, 4, 32), (16, 1, 1.0, 4, 32), (32, 3, 1.0, 4, 32),
         (23, 7, 1.0, 2, 32), (23, 7, 1.0, 3, 32), (23, 7, 1.0, 6, 32)]
IDS = ['64x64-b8-64-tiles', '64x64-b16-rebase', '23x23-b7-ragged-last-tile', '16x16-b1-one-clipped-tile', '32x32-b3-halo-32',
       '23x23-b7-2-layers', '23x23-b7-3-layers', '23x23-b7-6-layers-two-groups']


def _setup(gpu_device, mesh_n, batch, scale, layers, monkeypatch):
    import g_adaptivity_amd.functional as Fn_mod
    from g_adaptivity_amd.training import FusedIteration
    monkeypatch.setattr(Fn_mod, 'SMALL_MESH_FORWARD', False)
    monkeypatch.setattr(graph_mod, 'WIDE_MIN_NODES', 0)
    opt = hot_path_opt(mesh_dims=[mesh_n, mesh_n], hidden_dim=64, num_layers=layers, lr=0.0, device=str(gpu_device), show_mesh_evol_plots='False')
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


def _block_halo(graph):
    """What the default forward choice runs this graph with: the halo of the block launch, 0 = one launch per layer."""
    return lib().gadapt_narrow_block_halo(graph.c_ref, 64)


def _host_halo(graph):
    rowptr, col = graph._cpu_csr_t
    h = C.c_int32(-1)
    assert lib().gadapt_narrow_block_halo_host(rowptr.data_ptr(), col.data_ptr(), graph.num_nodes, C.addressof(h)) == 0
    return h.value


def _forward_once(it, mode):
    """One `gadapt_block_forward_loss_narrow` call on poisoned buffers; returns every value it stores."""
    f = it.fwd
    n, L = f.n, f.L
    lib().gadapt_debug_set_narrow_forward(mode)
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
                a=f.coeffs[0].clone(), p0=f.coeffs[1].clone(), loss=f.partials[:n_part].double().sum().item(), n_part=n_part)


STORED = ('slots', 'top', 'alpha', 'seed', 'a', 'p0')


@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("mesh_n,batch,scale,layers,halo", CASES, ids=IDS)
def test_block_launch_equals_per_layer_launches(gpu_device, mesh_n, batch, scale, layers, halo, monkeypatch):
    model, data, it = _setup(gpu_device, mesh_n, batch, scale, layers, monkeypatch)
    assert _block_halo(it.graph) == halo == it.graph.narrow_block_halo == _host_halo(it.graph)
    lib().gadapt_debug_set_narrow_forward(2)
    try:
        assert _block_halo(it.graph) == 0                               # the forced per-layer choice
    finally:
        lib().gadapt_debug_set_narrow_forward(1)
    new, old, again = _forward_once(it, 1), _forward_once(it, 2), _forward_once(it, 1)
    tiles, steps = (it.fwd.n + 511) // 512, (it.fwd.n + 255) // 256
    assert new['n_part'] == 8 * tiles and old['n_part'] == 4 * steps   # one partial per wave: the launch that ended the block
    for k in STORED:
        assert not torch.isnan(new[k]).any(), k
        assert torch.equal(new[k], old[k]), k
        assert torch.equal(new[k], again[k]), k                         # two block runs on freshly poisoned buffers
    assert abs(new['loss'] - old['loss']) <= 1e-6 * abs(old['loss']), (new['loss'], old['loss'])
    assert new['loss'] == again['loss']
    if scale > 1.0:
        # the case is what it claims: many rows whose first weight is at most e^-16 of another one (the softmax re-based in layer 0)
        rp = it.graph.rowptr_t.long()
        a0 = new['alpha'][0]
        first = a0[rp[:-1][rp[1:] > rp[:-1]]]
        assert (first < 1.2e-7).sum().item() > 1000


def _autograd(model, data, tgt, mode):
    lib().gadapt_debug_set_narrow_forward(mode)
    try:
        model.zero_grad(set_to_none=True)
        out = model(data)
        F.mse_loss(out, tgt).backward()
        torch.cuda.synchronize()
    finally:
        lib().gadapt_debug_set_narrow_forward(1)
    return out.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("mesh_n,batch,scale,layers,halo", [CASES[0], CASES[2], CASES[7]], ids=[IDS[0], IDS[2], IDS[7]])
def test_autograd_and_evaluation_paths(gpu_device, mesh_n, batch, scale, layers, halo, monkeypatch):
    """`model(data)` plus backward (gadapt_block_forward_narrow, coefficients given) and the evaluation forward without a target or an
    attention buffer (`GraphedForward`: gadapt_block_forward_loss_narrow with target = NULL): output and every weight gradient
    bit-identical with either choice."""
    from g_adaptivity_amd.inference import GraphedForward
    model, data, it = _setup(gpu_device, mesh_n, batch, scale, layers, monkeypatch)
    assert _block_halo(it.graph) == halo
    (o1, g1), (o2, g2) = _autograd(model, data, data.x_phys, 1), _autograd(model, data, data.x_phys, 2)
    assert not torch.isnan(o1).any() and torch.equal(o1, o2)
    assert set(g1) == set(g2) and g1
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    model.eval()
    gf = GraphedForward(model, data)
    assert gf.issued
    outs = []
    for mode in (1, 2):
        lib().gadapt_debug_set_narrow_forward(mode)
        try:
            gf.out.fill_(float('nan'))
            outs.append(gf(data).clone())
        finally:
            lib().gadapt_debug_set_narrow_forward(1)
    assert not torch.isnan(outs[0]).any() and torch.equal(outs[0], outs[1])


@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("case_id", ng.IDS)
def test_graphs_of_the_narrow_route(gpu_device, case_id, monkeypatch):
    """Ragged rows, mixed mesh sizes, 1-D meshes, the 512-row window: equal where the graph is eligible; where it is not, the query is 0
    and the default choice runs the per-layer launches."""
    import g_adaptivity_amd.functional as Fn
    b = ng.build(case_id)
    c = b.case
    monkeypatch.setattr(Fn, 'SMALL_MESH_FORWARD', False)
    monkeypatch.setattr(graph_mod, 'WIDE_MIN_NODES', 0)
    if c.half_max is not None:
        monkeypatch.setattr(graph_mod, 'WIDE_HALF_MAX_NODES', c.half_max)
    model = hip_model_like(b.oracle, b.ds, b.opt, gpu_device).train()
    data, tgt = b.data.clone().to(gpu_device), b.tgt.to(gpu_device)
    xc = data.x_comp if data.x_comp.dim() == 2 else data.x_comp.unsqueeze(-1)
    graph = model._graph(data, xc.shape[0], xc.device)
    assert graph.narrow_route(64) and graph.num_nodes == c.nodes
    want = _host_halo(graph)
    rp, cl = (t.tolist() for t in graph._cpu_csr_t)
    brute = next((h for h in (32, 64) if all(32 * (i // 32) - h <= j < 32 * (i // 32) + 32 + h
                                             for i in range(c.nodes) for j in cl[rp[i]:rp[i + 1]])), 0)
    assert _block_halo(graph) == want == brute
    assert (want == 0) == c.big                                          # meshes 65 and 100 nodes wide: neighbours up to 101 nodes away
    (o1, g1), (o2, g2) = _autograd(model, data, tgt, 1), _autograd(model, data, tgt, 2)
    assert not torch.isnan(o1).any() and torch.equal(o1, o2)
    assert set(g1) == set(g2) and g1
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
