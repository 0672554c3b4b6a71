"""The narrow route's step tail spread over row-owning workgroups (`step_tail_narrow_spread_kernel`, csrc/gadapt_tail_plan.h, DESIGN.md
section 5) against the one-workgroup `step_tail_narrow_kernel` (`gadapt_debug_set_narrow_tail_spread(0)`), in one process.  Both add the
slab rows in the same order, run the same chain-rule expressions and the same Adam arithmetic, so everything is compared with
`torch.equal` from cloned state: the flat gradient, the parameters, both moments, the step count and the loss."""
import os

import pytest
import torch

from g_adaptivity_amd import GNN, MeshDataset, collate, hot_path_opt, mse_loss, unit_gradient
from g_adaptivity_amd import graph as graph_mod
from g_adaptivity_amd.optim import FlatAdam
from g_adaptivity_amd._native import lib, ptr

C_ = 64
PACKED = 32                 # packed slab row
NPAR = 2 * C_ * C_ + 2 * C_
DEFAULT = 0 if os.environ.get('GADAPT_NARROW_TAIL_SPREAD', '1')[:1] == '0' else 1     # what the library starts with
KEYS = ('grad', 'param', 'm', 'v', 'state', 'loss')


class _switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        lib().gadapt_debug_set_narrow_tail_spread(self.on)

    def __exit__(self, *exc):
        lib().gadapt_debug_set_narrow_tail_spread(DEFAULT)


def _inputs(gpu_device, n_rows, n_loss, seed):
    gen = torch.Generator(device='cpu').manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(gpu_device)
    slab = rnd(n_rows, PACKED)
    slab[:, 20:] = 0
    state0 = dict(param=0.1 * rnd(NPAR), m=0.01 * rnd(NPAR), v=(0.01 * rnd(NPAR)) ** 2)
    partials = rnd(n_loss).abs() if n_loss else None
    return slab, state0, partials


def _steps(gpu_device, on, slab, state0, partials, weight_decay, moments, steps, sync_each=True):
    """`steps` calls of gadapt_step_tail_narrow in a row from cloned state, every buffer the call writes NaN-poisoned first; what each
    call leaves (sync_each) or what the last one leaves behind one synchronisation at the end."""
    param, m, v = state0['param'].clone(), state0['m'].clone(), state0['v'].clone()
    state = torch.zeros(2, dtype=torch.int32, device=gpu_device)
    grad, loss = torch.full((NPAR,), float('nan'), device=gpu_device), torch.full((), float('nan'), device=gpu_device)
    scratch = torch.empty(8, device=gpu_device)
    args = [ptr(slab), slab.shape[0], ptr(scratch), ptr(param), ptr(grad), ptr(m) if moments else None, ptr(v) if moments else None,
            1e-3, 0.9, 0.999, 1e-8, weight_decay, ptr(state), 1.0, None, None, ptr(partials), 0 if partials is None else partials.numel(),
            ptr(loss), 4 * 1234, C_, None]
    snap = lambda: dict(grad=grad.clone(), param=param.clone(), m=m.clone(), v=v.clone(), state=state.clone(), loss=loss.clone())
    out = []
    with _switch(on):
        for _ in range(steps):
            if sync_each:
                grad.fill_(float('nan')); loss.fill_(float('nan'))
            assert lib().gadapt_step_tail_narrow(*args) == 0
            if sync_each:
                torch.cuda.synchronize()
                out.append(snap())
        torch.cuda.synchronize()
    return out if sync_each else [snap()]


def _same(want, got, what):
    for k in KEYS:
        if k == 'loss' and torch.isnan(want[k]):                # no loss partials: the loss is not written, the poison stays
            assert torch.isnan(got[k]), what
            continue
        assert not torch.isnan(got[k].float()).any(), (what, k)
        assert torch.equal(want[k], got[k]), (what, k, (want[k].float() - got[k].float()).abs().max().item())


# n_rows (8 chunks of per = ceil(n_rows / 8) rows): one row and seven empty chunks; fewer rows than chunks; one row per chunk; per = 2
# with empty chunks; per = 32 with the last chunk one short; exactly one full 32-row group per chunk; per = 33, one leftover row; one full
# group plus leftovers (per = 38); two full groups per chunk (the headline); 1024: per = 128, the loop over groups (euler20)
@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("n_rows", [1, 7, 8, 9, 255, 256, 257, 300, 512, 1024])
def test_spread_tail_is_the_one_workgroup_tail(gpu_device, n_rows):
    for n_loss in (0, 7, 256, 2048):
        slab, state0, partials = _inputs(gpu_device, n_rows, n_loss, 1000 * n_rows + n_loss)
        for weight_decay in (0.0, 1e-2):
            for moments in (True, False):
                what = (n_rows, n_loss, weight_decay, moments)
                want = _steps(gpu_device, 0, slab, state0, partials, weight_decay, moments, 3)
                got = _steps(gpu_device, 1, slab, state0, partials, weight_decay, moments, 3)
                for k, (w, g) in enumerate(zip(want, got)):
                    _same(w, g, what + (k,))
                    if moments:
                        assert g['state'].tolist() == [k + 1, 0], what
                        assert not torch.equal(g['param'], state0['param'])
                    else:                                            # gradient only: nothing but the flat gradient and the loss is written
                        assert g['state'].tolist() == [0, 0], what
                        assert all(torch.equal(g[x], state0[x]) for x in ('param', 'm', 'v')), what
                assert want[0]['grad'].abs().max().item() > 0


# Fifty calls issued back to back, one synchronisation at the end: a workgroup that read the step count late, or lost it, would leave
# other parameters than fifty calls of the one-workgroup kernel, or another count
@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("n_rows,n_loss", [(512, 256), (300, 0)])
def test_fifty_calls_back_to_back(gpu_device, n_rows, n_loss):
    slab, state0, partials = _inputs(gpu_device, n_rows, n_loss, 77 + n_rows)
    want, = _steps(gpu_device, 0, slab, state0, partials, 1e-2, True, 50, sync_each=False)
    got, = _steps(gpu_device, 1, slab, state0, partials, 1e-2, True, 50, sync_each=False)
    assert got['state'].tolist() == [50, 0] and want['state'].tolist() == [50, 0]
    _same(want, got, (n_rows, n_loss))


@pytest.mark.gpu
@pytest.mark.one_dispatch
def test_switch_off_on_off_reproduces(gpu_device):
    slab, state0, partials = _inputs(gpu_device, 300, 256, 5)
    runs = [_steps(gpu_device, on, slab, state0, partials, 1e-2, True, 2) for on in (0, 1, 0)]
    for k in range(2):
        _same(runs[0][k], runs[1][k], ('off-on', k))
        _same(runs[0][k], runs[2][k], ('off-off', k))


def _fused_run(gpu_device, mesh_n, batch, on, monkeypatch):
    import g_adaptivity_amd.functional as Fn_mod
    from g_adaptivity_amd.training import FusedIteration
    monkeypatch.setattr(Fn_mod, 'SMALL_MESH_FORWARD', False)
    monkeypatch.setattr(graph_mod, 'WIDE_MIN_NODES', 0)
    opt = hot_path_opt(mesh_dims=[mesh_n, mesh_n], hidden_dim=64, num_layers=4, lr=1e-3, device=str(gpu_device), show_mesh_evol_plots='False')
    ds = MeshDataset([mesh_n, mesh_n], batch, seed=11)
    data = collate(ds.samples).to(gpu_device)
    torch.manual_seed(12)
    model = GNN(ds, opt).to(gpu_device).train()
    optim = FlatAdam(model.parameters(), lr=1e-3, weight_decay=1e-2, capturable=True)
    optim.zero_grad(); mse_loss(model(data), data.x_phys).backward(gradient=unit_gradient(gpu_device)); optim.step()   # lays the bucket out
    assert FusedIteration.eligible(model, optim, mse_loss, data, 'x_phys') is None
    it = FusedIteration(model, optim, mse_loss, data, 'x_phys')
    assert it.fwd.narrow, "the case must take the narrow route"
    it.refresh_coeffs()
    out = []
    with _switch(on):
        for _ in range(3):
            it.run()
            torch.cuda.synchronize()
            out.append(dict(out=it.out.clone(), loss=it.loss.clone(), flat=it.flat.clone(), bucket=optim.bucket.clone(),
                            m=optim.exp_avg.clone(), v=optim.exp_avg_sq.clone(), state=optim._dev_state.clone()))
    return out


@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("mesh_n,batch", [(16, 1), (64, 2)], ids=['16x16-b1', '64x64-b2'])
def test_fused_iteration_is_the_same_either_way(gpu_device, mesh_n, batch, monkeypatch):
    want = _fused_run(gpu_device, mesh_n, batch, 0, monkeypatch)
    got = _fused_run(gpu_device, mesh_n, batch, 1, monkeypatch)
    for k, (w, g) in enumerate(zip(want, got)):
        for key in w:
            assert not torch.isnan(g[key].float()).any(), (k, key)
            assert torch.equal(w[key], g[key]), (k, key)
    assert want[2]['state'].tolist()[1] == 0 and got[2]['state'].tolist() == want[2]['state'].tolist()
    assert not torch.equal(got[0]['bucket'], got[2]['bucket'])
