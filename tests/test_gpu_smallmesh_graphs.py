"""The one-launch small-mesh pair (csrc/gadapt_smallmesh.inc) against the fp64 oracle on the batches of tests/smallmesh_graphs.py:
meshes of different sizes in one launch, both forms of the backward's alpha load, hidden 32 in all its instantiations, one mesh,
per-layer convs, in-rows of 0 / 1 / 12+ and out-rows of 0 / 12+, an edgeless trailing mesh, a mesh of long rows only, the size
limits.  tests/test_smallmesh_graphs_host.py proves on the CPU that every case is what it claims - the instantiation it selects
included - and that it is quiet (fp32 oracle within 5e-5 of fp64 on every gradient).

 1. training through the pair (profile ids 9 / 10 ran once, 0 / 1 not at all; `limit-over`: the other way round): coordinates within 1e-5
    (fp32 oracle normwise and elementwise, fp64 normwise); every conv-parameter gradient of every distinct conv
    `e64 <= max(1e-4, 1.5 x noise)`, `noise` = the fp32 oracle against fp64; d lin_key.bias exactly 0; the attention of every layer in
    the caller's edge order within 1e-5 of the fp64 oracle's;
 2. the evaluation forward (`eval()`, `no_grad`) of every case, `full-1024` included: the same coordinate bounds; rows of nodes without
    in-edges against (1 - dt)^L x of fp64;
 3. batch independence, bitwise: every mesh of the `mixed-*` cases and of `ragged-13` run alone through the C-ABI - where it selects the
    batch's instantiation its output rows, alpha, x_all rows and slab row ARE the batch's; the gradient assembled from the lone slab
    rows is held under the fp64 rule either way; two runs on NaN-poisoned buffers store the same bits and leave no NaN;
 4. `FusedIteration` with `mse_loss` and `l1_loss`: on the pair, output and flat gradient bit-identical to the autograd path's, both
    gradients under the fp64 rule (the l1 one with the l1 noise), the loss within max(1e-6, 1.5 x the fp32 oracle's own deviation) of
    fp64, one loss partial per wave of the claimed forward; where it does not apply, the documented reason;
 5. `mesh_eptr = NULL` (the C-ABI allows it, Python never passes it): forward and backward store the same bits as with the offsets.

The figures every case prints are on record in docs/measurements.md ("The small-mesh pair against fp64 at its launch edges").
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import smallmesh_graphs as sg
from helpers import hip_model_like, rel_err
from g_adaptivity_amd import l1_loss, mse_loss, unit_gradient
from g_adaptivity_amd._native import check, current_stream, lib, ptr
from g_adaptivity_amd.functional import bucket_cuts
from g_adaptivity_amd.graph import MeshGraph
from g_adaptivity_amd.optim import FlatAdam

NAN = float('nan')


def _launches(kernel_id):
    tot, cnt = C.c_double(0.0), C.c_int(0)
    lib().gadapt_profile_read(kernel_id, C.byref(tot), C.byref(cnt))
    return cnt.value


def _take_every_size(monkeypatch):
    """Every size the kernels take, not only where the pair is the faster one (as tests/test_gpu_smallmesh.py does)."""
    import g_adaptivity_amd.functional as Fn
    monkeypatch.setattr(Fn, 'small_forward_policy', lambda c, max_nodes: True)
    monkeypatch.setattr(Fn, 'small_training_policy', lambda c, max_nodes: True)


def _profiled(fn):
    """fn() with the launch counters on: (its result, {profile id: launches})."""
    lib().gadapt_profile_reset(); lib().gadapt_profile_enable(1)
    try:
        res = fn()
        torch.cuda.synchronize()
        counts = {k: _launches(k) for k in (9, 10, 0, 1)}
    finally:
        lib().gadapt_profile_enable(0); lib().gadapt_profile_reset()
    return res, counts


def _watch_attention(model, monkeypatch):
    """{'graph', 'alpha'} of the model's next forward: the [L,E] attention in target-CSR order that it publishes (a weight-shared conv
    is ONE module: its `stored_alpha` shows the last layer only)."""
    seen, publish = {}, model._publish_attention

    def spy(graph, alpha):
        seen.update(graph=graph, alpha=alpha.detach().clone())
        return publish(graph, alpha)
    monkeypatch.setattr(model, '_publish_attention', spy)
    return seen


def _coordinates(case_id, what, out, b):
    assert out.shape == b.ref.shape and not torch.isnan(out).any()
    norm, elem = rel_err(out, b.ref)
    norm64 = rel_err(out, b.ref64)[0]
    print(f"{case_id} [{what}] coordinates: vs fp32 oracle normwise {norm:.2e} elementwise {elem:.2e}; vs fp64 normwise {norm64:.2e}")
    assert norm <= sg.COORD_TOL and elem <= sg.COORD_TOL and norm64 <= sg.COORD_TOL


def _attention(case_id, what, seen, b, bound=sg.COORD_TOL):
    """Every layer's attention, brought to the caller's edge order, against the fp64 oracle's."""
    graph, alpha = seen['graph'], seen['alpha']
    assert alpha.shape[0] == b.case.layers and torch.equal(graph.edge_index.cpu(), b.edge_index)
    worst = 0.0
    for l in range(b.case.layers):
        got = graph.alpha_to_edge_order(alpha[l][:graph.num_edges])
        assert not torch.isnan(got).any()
        worst = max(worst, rel_err(got, b.alpha64[l])[0])
    print(f"{case_id} [{what}] attention vs fp64, worst layer: {worst:.2e} (fp32 oracle: {b.alpha_noise:.2e})")
    assert worst <= bound


def _fp64_rule(case_id, what, grads, g64, noise):
    """e64 <= max(1e-4, 1.5 x noise) on the three weight gradients of every distinct conv; every figure printed first."""
    bad = []
    assert len(grads) == len(g64) == len(noise)
    for k, (g, ref, nz) in enumerate(zip(grads, g64, noise)):
        for name in sg.PARAMETERS:
            e64, bound = rel_err(g[name], ref[name])[0], max(sg.GRAD_TOL, 1.5 * nz[name])
            print(f"{case_id} [{what}] conv {k} {name}: e64 {e64:.2e} noise {nz[name]:.2e} bound {bound:.2e}")
            if not e64 <= bound:
                bad.append(f"{what} conv {k} {name}.grad: {e64:.2e} vs fp64 (fp32 oracle: {nz[name]:.2e})")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("case_id", sg.TRAINED)
def test_pair_against_fp64(gpu_device, case_id, monkeypatch):
    _take_every_size(monkeypatch)
    b = sg.build(case_id)
    c = b.case
    model = hip_model_like(b.oracle, b.ds, b.opt, gpu_device).train()
    data, tgt = b.data.clone().to(gpu_device), b.tgt.to(gpu_device)
    seen = _watch_attention(model, monkeypatch)

    def step():
        model.zero_grad(set_to_none=True)
        out = model(data)
        F.mse_loss(out, tgt).backward()
        return out.detach().clone()
    out, n = _profiled(step)
    if c.bwd is not None:
        assert n == {9: 1, 10: 1, 0: 0, 1: 0}, f"the one-launch pair did not run: {n}"
    else:                                                                # the backward does not fit the LDS: the per-layer kernels train it
        assert n[9] == 0 and n[10] == 0 and n[0] == c.layers and n[1] > 0, n
    _coordinates(case_id, 'train', out, b)
    convs = sg.distinct_convs(model)
    grads = [{k: dict(cv.named_parameters())[k].grad for k in sg.PARAMETERS} for cv in convs]
    _fp64_rule(case_id, 'pair' if c.bwd is not None else 'per-layer', grads, b.g64, b.noise)
    for cv in convs:
        assert cv.lin_key.bias.grad.abs().max().item() == 0.0            # vanishes analytically (softmax shift invariance)
    _attention(case_id, 'train', seen, b)
    last = convs[-1].stored_alpha                                        # [E,1], the caller's edge order: the top layer's
    assert last.shape == (b.edge_index.shape[1], 1) and rel_err(last.reshape(-1), b.alpha64[-1])[0] <= sg.COORD_TOL


@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("case_id", sg.IDS)
def test_evaluation_forward_against_fp64(gpu_device, case_id, monkeypatch):
    _take_every_size(monkeypatch)
    b = sg.build(case_id)
    c = b.case
    model = hip_model_like(b.oracle, b.ds, b.opt, gpu_device).eval()
    data = b.data.clone().to(gpu_device)
    seen = _watch_attention(model, monkeypatch)

    def run():
        with torch.no_grad():
            return model(data).clone()
    out, n = _profiled(run)
    assert n == {9: 1, 10: 0, 0: 0, 1: 0}, f"the evaluation forward of a small-mesh batch must be the one-launch kernel: {n}"
    _coordinates(case_id, 'eval', out, b)
    # (not asked of the training test, whose bound is 1e-5 flat: on `full-1024`, evaluated only, the fp32 ORACLE's attention is 6.5e-5 off)
    _attention(case_id, 'eval', seen, b, bound=max(sg.COORD_TOL, 1.5 * b.alpha_noise))
    g = seen['graph']
    empty = torch.nonzero(g.rowptr_t[1:] == g.rowptr_t[:-1]).reshape(-1).cpu()
    assert (empty.numel() > 0) == (c.deg_t[0] == 0)
    if empty.numel():                                                    # no in-edge: x + dt (0 - x) in every layer
        want = (1.0 - b.opt['time_step']) ** c.layers * b.data.x_comp[empty].double()
        norm, elem = rel_err(out[empty.to(gpu_device)], want)
        print(f"{case_id} [eval] {empty.numel()} rows without in-edges vs fp64: normwise {norm:.2e} elementwise {elem:.2e}")
        assert norm <= sg.COORD_TOL and elem <= sg.COORD_TOL


# ------------------------------------------------------------------------------------------------ the C-ABI, called directly
def _plan(model, data):
    """(graph, the model's one-launch plan for a TRAINING step of the batch, its node fields, its stacked conv weights)."""
    o = model.opt
    xc = data.x_comp if data.x_comp.dim() == 2 else data.x_comp.unsqueeze(-1)
    f, uu = (data.f_tensor if o['gnn_inc_feat_f'] else None), (data.uu_tensor if o['gnn_inc_feat_uu'] else None)
    graph = model._graph(data, xc.shape[0], xc.device)
    with torch.enable_grad():
        r = model._route(data, graph, xc, f, uu)
    assert r.form == 'small' and r.small['train']
    w = tuple(t.contiguous() for t in model._stacked(detach=True))
    return graph, r.small, (xc.contiguous(), f, uu), w


def _forward(graph, part, fields, plan, w, layers, eptr=True):
    """gadapt_small_forward keeping x_all and alpha, on NaN-poisoned buffers: (out [N,dim], alpha [L,E], x_all [L,N,C])."""
    import g_adaptivity_amd.functional as Fn
    xc, f, uu = fields
    n, dim = xc.shape
    S, c = w[0].shape[0], w[0].shape[1]
    dev = xc.device
    out = torch.full((n, dim), NAN, device=dev)
    alpha = torch.full((layers, max(graph.num_edges, 1)), NAN, device=dev)
    x_all = torch.full((layers, n, c), NAN, device=dev)
    args = Fn._small_args(graph, part, ptr(xc), dim, ptr(f), ptr(uu), plan['enc_w'], w[0], w[1], w[2], S, plan['lp'], layers, out, dim, alpha, x_all)
    if not eptr:
        assert args[2] is not None
        args[2] = None                                                   # mesh_eptr: the kernels take the edge offsets from rowptr
    check(lib().gadapt_small_forward(*args, c, current_stream(dev)), 'gadapt_small_forward')
    return out, alpha[:, :graph.num_edges], x_all


def _backward(graph, part, x_all, alpha, g_top, plan, w, layers, eptr=True):
    """gadapt_small_backward on a NaN-poisoned slab: [S, n_meshes, C*C + C]."""
    mesh_ptr, n_meshes, max_nodes, max_edges = part
    S, c = w[0].shape[0], w[0].shape[1]
    dev = g_top.device
    slab = torch.full((S, n_meshes, c * c + c), NAN, device=dev)
    alpha = alpha.contiguous() if alpha.shape[1] else torch.zeros(layers, 1, device=dev)
    check(lib().gadapt_small_backward(graph.c_ref, ptr(mesh_ptr[0]), ptr(mesh_ptr[1]) if eptr else None, n_meshes, max_nodes, max_edges, ptr(x_all),
                                      ptr(alpha), ptr(g_top), g_top.shape[1], ptr(w[0]), ptr(w[1]), ptr(w[2]), c * c if S > 1 else 0,
                                      c if S > 1 else 0, ptr(plan['lp']), layers, ptr(slab), c, current_stream(dev)), 'gadapt_small_backward')
    return slab


def _gradients(slab, w, layers):
    """The conv-parameter gradients of a slab, as `functional._SmallMeshBlock.backward` makes them: per distinct conv
    {parameter: gradient}."""
    S, n_meshes, row = slab.shape
    c, dev, st = w[0].shape[1], slab.device, current_stream(slab.device)
    flat = torch.empty(S * (2 * c * c + 2 * c), device=dev)
    cuts = bucket_cuts(c, S)
    d_wq, d_wk = flat[cuts[0]:cuts[1]].view(S, c, c), flat[cuts[2]:cuts[3]].view(S, c, c)
    d_bq, d_bk = flat[cuts[1]:cuts[2]].view(S, c), flat[cuts[3]:cuts[4]].view(S, c)
    scratch = torch.empty(32 * row, device=dev)
    slab = slab.contiguous()
    for s_ in range(S):
        check(lib().gadapt_slab_reduce_coeffs_backward(ptr(slab[s_]), n_meshes, ptr(scratch), ptr(w[0][s_]), ptr(w[1][s_]), ptr(w[2][s_]), ptr(d_wq[s_]),
                                                       ptr(d_bq[s_]), ptr(d_wk[s_]), ptr(d_bk[s_]), c, st, None, layers, 0, None),
              'gadapt_slab_reduce_coeffs_backward')
    torch.cuda.synchronize()
    return [{'lin_query.weight': d_wq[s_].clone(), 'lin_query.bias': d_bq[s_].clone(), 'lin_key.weight': d_wk[s_].clone()} for s_ in range(S)]


def _batched(b, model, data, eptr=True):
    graph, plan, fields, w = _plan(model, data)
    L = b.case.layers
    out, alpha, x_all = _forward(graph, plan['part'], fields, plan, w, L, eptr)
    g_top = (2.0 / out.numel() * (out - b.tgt.to(out.device))).contiguous()       # d mse_loss / d out
    slab = _backward(graph, plan['part'], x_all, alpha, g_top, plan, w, L, eptr)
    torch.cuda.synchronize()
    return SimpleRun(graph, plan, fields, w, out, alpha, x_all, g_top, slab)


class SimpleRun:
    def __init__(self, graph, plan, fields, w, out, alpha, x_all, g_top, slab):
        self.graph, self.plan, self.fields, self.w = graph, plan, fields, w
        self.out, self.alpha, self.x_all, self.g_top, self.slab = out, alpha, x_all, g_top, slab

    def stored(self):
        return (self.out, self.alpha, self.x_all, self.slab)


def _same_bits(a, b):
    for x, y in zip(a.stored(), b.stored()):
        assert x.shape == y.shape and not torch.isnan(x).any() and torch.equal(x, y)


@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("case_id", sg.LONE)
def test_batch_independence(gpu_device, case_id, monkeypatch):
    _take_every_size(monkeypatch)
    b = sg.build(case_id)
    c, L = b.case, b.case.layers
    model = hip_model_like(b.oracle, b.ds, b.opt, gpu_device).train()
    data = b.data.clone().to(gpu_device)
    run = _batched(b, model, data)
    _same_bits(run, _batched(b, model, data))                            # two runs on poisoned buffers: the same bits, no NaN left
    _coordinates(case_id, 'C-ABI', run.out, b)
    _fp64_rule(case_id, 'C-ABI batch', _gradients(run.slab, run.w, L), b.g64, b.noise)
    mesh_ptr = run.plan['part'][0].cpu()
    ei = run.graph.edge_index.cpu()
    rows = []
    for m, same in enumerate(c.lone):
        n0, n1, e0, e1 = int(mesh_ptr[0][m]), int(mesh_ptr[0][m + 1]), int(mesh_ptr[1][m]), int(mesh_ptr[1][m + 1])
        sel = (ei[1] >= n0) & (ei[1] < n1)
        assert int(sel.sum()) == e1 - e0 and bool(((ei[0][sel] >= n0) & (ei[0][sel] < n1)).all())
        g_m = MeshGraph((ei[:, sel] - n0).contiguous(), n1 - n0, gpu_device)      # (stable CSR build: the batch's edge order inside every row)
        part = g_m.mesh_partition(None)
        assert part[1:] == (1, n1 - n0, e1 - e0)
        fields = tuple(None if t is None else t[n0:n1].contiguous() for t in run.fields)
        out, alpha, x_all = _forward(g_m, part, fields, run.plan, run.w, L)
        slab = _backward(g_m, part, x_all, alpha, run.g_top[n0:n1].contiguous(), run.plan, run.w, L)
        torch.cuda.synchronize()
        assert not any(torch.isnan(t).any() for t in (out, alpha, x_all, slab))
        rows.append(slab)
        if same:                                                         # the batch's instantiation: the batch's bits
            assert torch.equal(out, run.out[n0:n1]) and torch.equal(alpha, run.alpha[:, e0:e1]) and torch.equal(x_all, run.x_all[:, n0:n1])
            assert torch.equal(slab[:, 0], run.slab[:, m]), (m, rel_err(slab[:, 0], run.slab[:, m]))
        else:                                                            # another instantiation: held against fp64 like the batch
            norm64 = rel_err(out, b.ref64[n0:n1])[0]
            worst = max(rel_err(g_m.alpha_to_edge_order(alpha[l]), b.alpha64[l][sel])[0] for l in range(L))
            print(f"{case_id} mesh {m} alone ({n1 - n0} nodes): coordinates vs fp64 {norm64:.2e}, attention vs fp64 {worst:.2e}")
            assert norm64 <= sg.COORD_TOL and worst <= sg.COORD_TOL
    # the gradient of the batch from the slab rows of its meshes run alone
    _fp64_rule(case_id, 'C-ABI lone meshes', _gradients(torch.cat(rows, dim=1), run.w, L), b.g64, b.noise)


@pytest.mark.gpu
@pytest.mark.one_dispatch
def test_edge_offsets_from_rowptr(gpu_device, monkeypatch):
    """`mesh_eptr = NULL`: the kernels read a mesh's first in-edge from rowptr_t[n0] (and rowptr_s[n0] in the backward) - one more
    dependent load, the same values."""
    _take_every_size(monkeypatch)
    b = sg.build('mixed-8-13-23')
    model = hip_model_like(b.oracle, b.ds, b.opt, gpu_device).train()
    data = b.data.clone().to(gpu_device)
    with_offsets, without = _batched(b, model, data, eptr=True), _batched(b, model, data, eptr=False)
    _same_bits(with_offsets, without)
    _coordinates('mixed-8-13-23', 'mesh_eptr = NULL', without.out, b)


@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("case_id", [k for k in sg.IDS if sg.CASES[k].fused is not None])
def test_fused_iteration(gpu_device, case_id, monkeypatch):
    from g_adaptivity_amd.training import FusedIteration
    _take_every_size(monkeypatch)
    b = sg.build(case_id)
    c = b.case
    model = hip_model_like(b.oracle, b.ds, b.opt, gpu_device).train()
    data = b.data.clone().to(gpu_device)
    optim = FlatAdam(model.parameters(), lr=0.0, capturable=True)
    if c.fused != 'small':                                               # 1-D (x_comp is [N]) and per-layer convs: the autograd iteration trains these
        for loss_fn in (mse_loss, l1_loss):
            assert FusedIteration.eligible(model, optim, loss_fn, data, 'x_phys') == c.fused
        return
    optim.zero_grad(); mse_loss(model(data), data.x_phys).backward(gradient=unit_gradient(gpu_device)); optim.step()   # lays the bucket out
    for name, loss_fn, g64, noise in (('mse', mse_loss, b.g64, b.noise), ('l1', l1_loss, b.l1_g64, b.l1_noise)):
        why = FusedIteration.eligible(model, optim, loss_fn, data, 'x_phys')
        assert why is None, why
        optim.zero_grad()
        out_a = model(data)
        loss_fn(out_a, data.x_phys).backward(gradient=unit_gradient(gpu_device))
        torch.cuda.synchronize()
        out_a, flat_a = out_a.detach().clone(), torch.cat([p.grad.reshape(-1) for p in optim.active]).clone()
        it = FusedIteration(model, optim, loss_fn, data, 'x_phys')
        assert it.small is not None                                      # the one-launch pair, not the per-layer kernels
        for t in (it.slab, it.flat, it.out, it.fwd.x_all, it.fwd.alpha, it.fwd.seed):
            t.fill_(NAN)
        _, n = _profiled(it.forward_backward)
        assert n == {9: 1, 10: 1, 0: 0, 1: 0}, n
        assert it.n_part == c.batch * c.fwd[1] // 64                     # one loss partial per wave of the claimed forward
        it.finish()                                                      # lr = 0: the parameters stay
        torch.cuda.synchronize()
        _coordinates(case_id, f'fused {name}', it.out, b)
        assert torch.equal(it.out, out_a)
        assert not torch.isnan(it.flat).any() and torch.equal(it.flat, flat_a), (name, rel_err(it.flat, flat_a))
        _fp64_rule(case_id, f'fused {name}', [{k: gk for k, (p, gk) in zip(sg.PARAMETERS, it.grads)}], g64, noise)
        assert it.flat[-c.hidden:].abs().max().item() == 0.0             # d lin_key.bias
        l32, l64 = b.losses[name]
        dev32, got = abs(l32 - l64) / abs(l64), abs(it.loss.item() - l64) / abs(l64)
        print(f"{case_id} {name}_loss: fused {it.loss.item():.9e} fp64 {l64:.9e}: {got:.2e} (fp32 oracle: {dev32:.2e})")
        assert got <= max(1e-6, 1.5 * dev32), (name, got, dev32)
