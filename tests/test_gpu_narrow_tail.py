"""The narrow route's packed slab and its one-launch tail.

`gadapt_block_backward_narrow_packed` writes slab rows of 32 floats - the 20 weight-gradient partials a target-pass workgroup owes
(entry 4 o + c = dA[o][c], entry 16 + o = dp0[o]; o, c < 4) and 12 zeros - where `gadapt_block_backward_narrow` writes rows of
64 * 64 + 64 floats that are zero outside those 20; `gadapt_step_tail_narrow` is `gadapt_step_tail` (two launches) over such rows in one
launch.  The full-width path is the oracle, and everything is compared with `torch.equal`: the sums, their order and the Adam
arithmetic are the same."""
import pytest
import torch

from g_adaptivity_amd import GNN, MeshDataset, collate, hot_path_opt, mse_loss, unit_gradient
from g_adaptivity_amd import graph as graph_mod
from g_adaptivity_amd.optim import FlatAdam
from g_adaptivity_amd._native import current_stream, lib, ptr

C_ = 64
ROW = C_ * C_ + C_          # full-width slab row: dA then dp0
PACKED = 32                 # packed slab row
NPAR = 2 * C_ * C_ + 2 * C_
BADARG = -1
# position of the 20 live entries of a full-width row, in packed order
LIVE = torch.tensor([o * C_ + c for o in range(4) for c in range(4)] + [C_ * C_ + o for o in range(4)])


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


def _backward_args(it, slab):
    """The backward's argument list of the iteration (`FusedIteration._plans`) with another slab."""
    args = list(it._bw[1])
    args[15] = ptr(slab)
    args[-1] = current_stream(it.device)
    return args


# The grid of a target-pass launch - the slab row count - is one workgroup per 64-node tile, rounded up to 8 and capped at 512, and each
# workgroup takes 256 nodes per grid-stride step.  23x23 b7, 2 layers: 64 rows, 15 workgroups with nodes (the last one ragged), 49
# that flush an all-zero row.  64x64 b3: 192 rows, 48 with nodes.  64x64 b33, 3 layers: 512 rows, lanes take two grid-stride steps.
@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("mesh_n,batch,layers,rows,busy", [(23, 7, 2, 64, 15), (64, 3, 4, 192, 48), (64, 33, 3, 512, 512)],
                         ids=['23x23-b7-2-layers-ragged', '64x64-b3-4-layers', '64x64-b33-3-layers-two-grid-stride-steps'])
@pytest.mark.parametrize("fused", [1, 0], ids=['fused', 'pairs'])
def test_packed_slab_holds_the_live_entries_of_the_full_slab(gpu_device, mesh_n, batch, layers, rows, busy, fused, monkeypatch):
    model, optim, it = _setup(gpu_device, mesh_n, batch, layers, monkeypatch)
    assert it.slab_rows == rows == lib().gadapt_backward_slab_rows(it.n, C_) and min(rows, -(-it.n // 256)) == busy
    assert it.slab.numel() == rows * PACKED == lib().gadapt_narrow_slab_floats(it.n)
    full = torch.full((rows, ROW), float('nan'), device=gpu_device)
    packed = torch.full((rows, PACKED), float('nan'), device=gpu_device)
    lib().gadapt_debug_set_narrow_backward_fused(fused)
    try:
        it.fwd(*it._in, current_stream(it.device))
        assert lib().gadapt_block_backward_narrow(*_backward_args(it, full)) == 0
        assert lib().gadapt_block_backward_narrow_packed(*_backward_args(it, packed)) == 0
        torch.cuda.synchronize()
    finally:
        lib().gadapt_debug_set_narrow_backward_fused(1)
    assert not torch.isnan(full).any() and not torch.isnan(packed).any()
    live = LIVE.to(gpu_device)
    assert torch.equal(packed[:, :20], full[:, live])
    assert (packed[:busy, :20].abs().amax(dim=1) > 0).all() and (packed[busy:] == 0).all()
    assert (packed[:, 20:] == 0).all()
    rest = torch.ones(ROW, dtype=torch.bool, device=gpu_device)
    rest[live] = False
    assert (full[:, rest] == 0).all()


def _tail_args(slab, n_rows, scratch, param, grad, m, v, state, wd, partials, loss, loss_count):
    return [ptr(slab), n_rows, ptr(scratch), ptr(param), ptr(grad), ptr(m), ptr(v), 1e-3, 0.9, 0.999, 1e-8, wd, ptr(state), 1.0,
            None, None, ptr(partials), 0 if partials is None else partials.numel(), ptr(loss), loss_count, C_, None]


# n_rows: fewer rows than chunks; a chunk of one row; per = 2; per = 9; one 32-group plus leftovers (per = 38); two full groups (per = 64)
@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("n_rows", [1, 3, 15, 65, 300, 512])
@pytest.mark.parametrize("n_loss", [7, 256, 2048])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_narrow_tail_is_the_two_launch_tail(gpu_device, n_rows, n_loss, weight_decay):
    gen = torch.Generator(device='cpu').manual_seed(1000 * n_rows + n_loss)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(gpu_device)
    packed = rnd(n_rows, PACKED)
    packed[:, 20:] = 0
    full = torch.zeros(n_rows, ROW, device=gpu_device)
    full[:, LIVE.to(gpu_device)] = packed[:, :20]
    param0, m0, v0 = 0.1 * rnd(NPAR), 0.01 * rnd(NPAR), (0.01 * rnd(NPAR)) ** 2
    partials = rnd(n_loss).abs()
    scratch = torch.empty(32 * ROW, device=gpu_device)
    loss_count = 4 * 1234

    def run(fn, slab, moments):
        """Two steps in a row from cloned state; what each step leaves."""
        param, m, v = param0.clone(), m0.clone(), v0.clone()
        state = torch.zeros(2, dtype=torch.int32, device=gpu_device)
        grad, loss = torch.full((NPAR,), float('nan'), device=gpu_device), torch.full((), float('nan'), device=gpu_device)
        out = []
        for _ in range(2):
            args = _tail_args(slab, n_rows, scratch, param, grad, m if moments else None, v if moments else None, state, weight_decay,
                              partials, loss, loss_count)
            assert fn(*args) == 0
            torch.cuda.synchronize()
            out.append(dict(grad=grad.clone(), param=param.clone(), m=m.clone(), v=v.clone(), state=state.clone(), loss=loss.clone()))
        return out

    for moments in (True, False):
        want = run(lib().gadapt_step_tail, full, moments)
        got = run(lib().gadapt_step_tail_narrow, packed, moments)
        for step, (w, g) in enumerate(zip(want, got)):
            for k in w:
                assert not torch.isnan(g[k].float()).any(), (moments, step, k)
                assert torch.equal(w[k], g[k]), (moments, step, k, (w[k].float() - g[k].float()).abs().max().item())
            if moments:
                assert g['state'].tolist() == [step + 1, 0]
                assert not torch.equal(g['param'], param0)
            else:                                                        # gradient only: nothing but the flat gradient and the loss is written
                assert g['state'].tolist() == [0, 0]
                assert torch.equal(g['param'], param0) and torch.equal(g['m'], m0) and torch.equal(g['v'], v0)
        assert want[0]['grad'].abs().max().item() > 0


@pytest.mark.gpu
@pytest.mark.one_dispatch
def test_bad_arguments_are_refused(gpu_device, monkeypatch):
    z = lambda n, **kw: torch.zeros(n, device=gpu_device, **kw)
    slab, scratch, param, grad, m, v = z(4 * PACKED), z(32 * ROW), z(NPAR), z(NPAR), z(NPAR), z(NPAR)
    state, partials, loss = z(2, dtype=torch.int32), z(8), z(1)
    good = _tail_args(slab, 4, scratch, param, grad, m, v, state, 0.0, partials, loss, 100)
    fn = lib().gadapt_step_tail_narrow

    def refused(**change):
        args = list(good)
        for k, val in change.items():
            args[int(k[1:])] = val
        return fn(*args) == BADARG

    assert refused(a20=32) and refused(a20=128)                           # hidden != 64
    assert refused(a1=0) and refused(a1=-3)                               # n_rows <= 0
    assert refused(a0=None) and refused(a2=None)                          # a missing slab or scratch
    assert refused(a12=None)                                              # moments given without state
    assert refused(a5=None) and refused(a3=None) and refused(a4=None)     # one moment only; no parameters; no gradient
    assert b'step_tail_narrow' in lib().gadapt_last_error()
    torch.cuda.synchronize()
    for t in (param, grad, m, v, loss):
        assert (t == 0).all()                                             # nothing was launched
    assert state.tolist() == [0, 0]
    # the packed backward takes one shared conv only
    model, optim, it = _setup(gpu_device, 23, 7, 2, monkeypatch)
    it.fwd(*it._in, current_stream(it.device))
    it.slab.fill_(float('nan'))
    for a_stride, p0_stride in ((C_ * C_, 0), (0, C_), (C_ * C_, C_)):
        args = _backward_args(it, it.slab)
        args[8], args[10] = a_stride, p0_stride
        assert lib().gadapt_block_backward_narrow_packed(*args) == BADARG
    assert b'packed' in lib().gadapt_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(it.slab).all()                                     # nothing was launched
    assert lib().gadapt_narrow_slab_floats(0) < 0
