"""loss_type='pde_loss' as a captured training step (`GraphedTrainStep` over `fem.PdeBatch`) against the eager loop on a twin
model: parameters, Adam moments and losses bit for bit, with new fields AND new Gaussians (in other counts per mesh) every
step.  7 x 7 meshes, batch 2, a 17 x 17 lattice, hidden 8, 2 layers."""
import pytest
import torch

from g_adaptivity_amd import GNN, GraphedTrainStep, MeshDataset, collate, hot_path_opt, l1_loss, mse_loss
from g_adaptivity_amd.fem import PdeBatch
from g_adaptivity_amd.optim import FlatAdam

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
N, NLAT = 7, 17
COUNTS = [(2, 2), (1, 3), (3, 1)]                            # Gaussians per mesh of the three batches


def _opt(**kw):
    return hot_path_opt(mesh_dims=[N, N], hidden_dim=8, num_layers=2, time_step=0.1, loss_type='pde_loss', eval_quad_points=NLAT,
                        device=str(DEV), **kw)


@pytest.fixture(scope='module')
def datasets():
    """One 7 x 7 dataset per Gaussian count, all over the same mesh."""
    return {k: MeshDataset([N, N], 4, seed=20 + k, num_gauss=k, pde_loss_fields=True, eval_quad_points=NLAT) for k in (1, 2, 3)}


@pytest.fixture(scope='module')
def batches(datasets):
    """Three batches of one topology: other fields, other Gaussians, other counts per mesh."""
    out = []
    for step, counts in enumerate(COUNTS):
        out.append(collate([datasets[k].samples[step + i] for i, k in enumerate(counts)]))
    assert [[len(p['centers']) for p in b.pde_params] for b in out] == [list(c) for c in COUNTS]
    return out


def _twin(ds, opt, seed=0):
    torch.manual_seed(seed)
    a = GNN(ds, opt).to(DEV).train()
    b = GNN(ds, opt).to(DEV).train()
    b.load_state_dict(a.state_dict())
    return a, b


def _state(model, optim):
    return [p.detach().clone() for p in model.parameters()] + [optim.exp_avg.clone(), optim.exp_avg_sq.clone()]


def _run(model, loss_fn, batches, captured, **kw):
    optim = FlatAdam(model.parameters(), lr=1e-2, capturable=True)
    step = GraphedTrainStep(model, optim, loss_fn=loss_fn, **kw)
    losses = []
    for b in batches:
        d = b.clone().to(DEV)
        losses.append((step(d) if captured else step.eager(d)).clone())
    torch.cuda.synchronize()
    return step, _state(model, optim), losses


def test_cached_tail_is_the_uncached_tail(datasets, batches):
    model, _ = _twin(datasets[2], _opt())
    res = []
    for cached in (False, True):
        d = batches[1].clone().to(DEV)
        if cached:
            d._pde_batch = PdeBatch.from_data(model, d)
        model.zero_grad()
        coeffs, x_phys, sol = model(d)
        l1_loss(sol.view(-1, 1), d.u_true_fine_tensor.view(-1, 1)).backward()
        res.append([coeffs.detach(), x_phys.detach(), sol.detach()] + [p.grad.clone() for p in model.parameters() if p.grad is not None])
    assert len(res[0]) == len(res[1]) > 3 and res[0][2].abs().max() > 0
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize('loss_fn', [mse_loss, l1_loss], ids=['mse', 'l1'])
def test_captured_step_is_the_eager_loop(datasets, batches, loss_fn):
    ma, mb = _twin(datasets[2], _opt())
    step, got, got_losses = _run(ma, loss_fn, batches, captured=True)
    _, want, want_losses = _run(mb, loss_fn, batches, captured=False)
    assert len(step._captured) == 1 and step.fused_reason is not None and 'pde_loss' in step.fused_reason
    assert step.target_field == 'u_true_fine_tensor'
    for k, (a, b) in enumerate(zip(got_losses, want_losses)):
        assert torch.equal(a, b), (k, a.item(), b.item())
    assert len({l.item() for l in got_losses}) == 3                              # three different batches
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_mixed_size_batch_in_one_step():
    from g_adaptivity_amd import Mixed_DataLoader, MixedMeshDataset
    ds = MixedMeshDataset([5, N], 2, seed=3, pde_loss_fields=True, eval_quad_points=NLAT)
    opt = _opt(data_type='randg_mix')
    batch = next(iter(Mixed_DataLoader(ds, batch_size=2, shuffle=False, follow_batch=[], exclude_keys=['pde_params'])))
    assert not hasattr(batch, 'pde_params') and batch.x_comp.shape[0] == 25 + N * N
    ma, mb = _twin(ds, opt)
    _, got, got_losses = _run(ma, l1_loss, [batch], captured=True)
    _, want, want_losses = _run(mb, l1_loss, [batch], captured=False)
    assert torch.equal(got_losses[0], want_losses[0])
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_wave_adjoint_step_is_the_lane_step(datasets, batches):
    ma, _ = _twin(datasets[2], _opt(fem_adjoint='wave'))
    mb, _ = _twin(datasets[2], _opt())
    step, got, got_losses = _run(ma, l1_loss, batches, captured=True)
    _, want, want_losses = _run(mb, l1_loss, batches, captured=True)
    assert next(iter(step._captured.values())).static._pde_batch.adjoint == 'wave'
    for a, b in zip(got + got_losses, want + want_losses):
        assert torch.equal(a, b)


def test_refusals_capture_nothing(datasets, batches):
    model, _ = _twin(datasets[2], _opt())
    optim = FlatAdam(model.parameters(), lr=1e-2, capturable=True)
    step = GraphedTrainStep(model, optim, loss_fn=l1_loss)
    bare = batches[0].clone().to(DEV)
    del bare.__dict__['pde_params']                                              # what DeviceMeshLoader yields
    with pytest.raises(ValueError, match='must carry its Gaussians'):
        step(bare)
    assert not step._captured
    tight = GraphedTrainStep(model, optim, loss_fn=l1_loss, max_gauss=1)
    with pytest.raises(ValueError, match=r'4 Gaussians in the batch, room for 2\b'):
        tight(batches[1].clone().to(DEV))
    assert not tight._captured

    ds1 = MeshDataset([11], 2)
    m1 = GNN(ds1, hot_path_opt(mesh_dims=[11], hidden_dim=8, num_layers=2, device=str(DEV))).to(DEV).train()
    m1.opt['loss_type'] = 'pde_loss'                                             # (the constructor refuses a 1-D pde_loss model itself)
    with pytest.raises(NotImplementedError, match='1-D'):
        GraphedTrainStep(m1, FlatAdam(m1.parameters(), capturable=True))
