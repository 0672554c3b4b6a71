"""1-D loss_type='pde_loss' (opt['pde_loss_1d']) as a captured training step (`GraphedTrainStep` over `fem1d.Pde1dBatch`): four steps
over changing batches with changing Gaussian counts per mesh.  The captured 'split' tail against the eager loop on a twin model:
parameters, Adam moments and losses bit for bit.  The captured 'fused' tail (gadapt_fem_poisson1d_loss) against 'split':
parameters and moments bit for bit; its losses, summed in another order, against tests/fem1d_restatement.py in fp64 with the
fp32 run as the noise (rel <= max(1e-5, 1.5 x noise)).  5 nodes, batch 2, 33 evaluation points, hidden 8, 2 layers.

Why 5 nodes.  A loss value is a sum over d = sol - u_true, and sol is stored in fp32: rounding sol alone (2^-24 |sol| per point)
moves mean(d^2) by up to 2 x 2^-24 |sol| / |d| of itself, whatever computes it.  For that to lie under the rule's floor of 1e-5
the case needs |d| / |sol| >= 1.2e-2.  On 15 nodes the FEM error of these Gaussians (scales 0.1 .. 0.5) is smaller than that
(measured: 3.3e-3 at the third step, where the bound is 3.7e-5 and both the three-launch and the one-launch loss stood at
1.1e-5 of the fp64 value, the fp32 restatement at 5.5e-6); on 5 nodes (h^2 twelve times larger) it is not.  The test asserts the
ratio, so a case that cannot tell a wrong loss from a rounded one fails as such."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fem1d_restatement as R  # noqa: E402

from g_adaptivity_amd import GNN, GraphedTrainStep, MeshDataset, collate, hot_path_opt, l1_loss, mse_loss  # noqa: E402
from g_adaptivity_amd.fem1d import Pde1dBatch  # noqa: E402
from g_adaptivity_amd.optim import FlatAdam  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
N, P = 5, 33
COUNTS = [(2, 2), (1, 3), (3, 1), (2, 3)]                    # Gaussians per mesh of the four batches
QUAD = {'load_quad_points': 101, 'stiff_quad_points': 3}


def _opt(**kw):
    return hot_path_opt(mesh_dims=[N], hidden_dim=8, num_layers=2, time_step=0.1, loss_type='pde_loss', pde_loss_1d=True,
                        eval_quad_points=P, device=str(DEV), **kw)


@pytest.fixture(scope='module')
def datasets():
    """One 5-node dataset per Gaussian count, all over the same mesh."""
    return {k: MeshDataset([N], 5, seed=30 + k, num_gauss=k, pde_loss_fields=True, eval_quad_points=P) for k in (1, 2, 3)}


@pytest.fixture(scope='module')
def batches(datasets):
    out = [collate([datasets[k].samples[step + i] for i, k in enumerate(counts)]) for step, counts in enumerate(COUNTS)]
    assert [[len(p['centers']) for p in b.pde_params] for b in out] == [list(c) for c in COUNTS]
    assert all(b.u_true_fine_tensor.shape == (2 * P,) for b in out)
    return out


def _twin(ds, opt, seed=0):
    torch.manual_seed(seed)
    a = GNN(ds, dict(opt)).to(DEV).train()
    b = GNN(ds, dict(opt)).to(DEV).train()
    b.load_state_dict(a.state_dict())
    return a, b


def _state(model, optim):
    return [p.detach().clone() for p in model.parameters()] + [optim.exp_avg.clone(), optim.exp_avg_sq.clone()]


def _run(model, loss_fn, batches, captured, keep_x=None, **kw):
    optim = FlatAdam(model.parameters(), lr=1e-2, capturable=True)
    step = GraphedTrainStep(model, optim, loss_fn=loss_fn, **kw)
    losses = []
    for b in batches:
        d = b.clone().to(DEV)
        if keep_x is not None:                                   # the mesh this step's loss is taken on
            with torch.no_grad():
                keep_x.append(model(d)[1].detach().cpu())
        losses.append((step(d) if captured else step.eager(d)).clone())
    torch.cuda.synchronize()
    return step, _state(model, optim), losses


def _cs(p, dtype):
    return ([torch.tensor(float(c[0]), dtype=dtype) for c in p['centers']], [torch.tensor(float(s[0]), dtype=dtype) for s in p['scales']])


def _restated_loss(x, batch, kind, dt):
    pts = torch.linspace(0, 1, P).to(dt)
    sols = [R.poisson(x[b * N:(b + 1) * N].to(dt), *_cs(batch.pde_params[b], dt), QUAD, pts)[1] for b in range(2)]
    d = torch.cat(sols) - batch.u_true_fine_tensor.to(dt)
    return (d.abs().mean() if kind == 'l1' else (d * d).mean()).double(), (d.norm() / torch.cat(sols).norm()).item()


@pytest.mark.parametrize('kind', ['l1', 'mse'])
def test_captured_split_is_the_eager_loop_and_fused_is_split(datasets, batches, kind):
    loss_fn = {'l1': l1_loss, 'mse': mse_loss}[kind]
    ma, mb = _twin(datasets[2], _opt())
    mc, _ = _twin(datasets[2], _opt(fem1d_tail='fused'))
    xs = []
    step, got, got_losses = _run(ma, loss_fn, batches, captured=True)
    _, want, want_losses = _run(mb, loss_fn, batches, captured=False, keep_x=xs)
    fstep, fused, fused_losses = _run(mc, loss_fn, batches, captured=True)
    assert len(step._captured) == 1 and step.fused_reason is not None and 'pde_loss' in step.fused_reason
    assert step.target_field == 'u_true_fine_tensor' and step.tail == 'split' and fstep.tail == 'fused'
    pb, fpb = (next(iter(s._captured.values())).static._pde_batch for s in (step, fstep))
    assert isinstance(pb, Pde1dBatch) and pb.fused is None and fpb.fused == ('u_true_fine_tensor', kind)
    assert pb.gptr.tolist() == [0, 2, 5] and pb.cap == 16                       # the last batch's Gaussians, room for 2 x 8
    for k, (a, b) in enumerate(zip(got_losses, want_losses)):
        assert torch.equal(a, b), (k, a.item(), b.item())
    assert len({l.item() for l in got_losses}) == 4                              # four different batches
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    for a, b in zip(fused, got):
        assert torch.equal(a, b)
    for k, (x, batch) in enumerate(zip(xs, batches)):
        (f64, ratio), (f32, _) = _restated_loss(x, batch, kind, torch.float64), _restated_loss(x, batch, kind, torch.float32)
        assert ratio >= 1.2e-2, (k, ratio, 'the case is ill-conditioned for a floor of 1e-5 on the loss value (see above)')
        noise = ((f32 - f64).abs() / f64.abs()).item()
        for tag, l in (('fused', fused_losses[k]), ('split', got_losses[k])):
            err = ((l.double().cpu() - f64).abs() / f64.abs()).item()
            print(f"step {k} {kind} {tag}: loss vs fp64 {err:.3e}, fp32 restatement vs fp64 {noise:.3e}, |d| / |sol| {ratio:.2e}")
            assert err <= max(1e-5, 1.5 * noise), (k, tag, err, noise)


def test_refusals_capture_nothing(datasets, batches):
    for tail in ('split', 'fused'):
        model, _ = _twin(datasets[2], _opt(fem1d_tail=tail))
        optim = FlatAdam(model.parameters(), lr=1e-2, capturable=True)
        step = GraphedTrainStep(model, optim, loss_fn=l1_loss)
        bare = batches[0].clone().to(DEV)
        del bare.__dict__['pde_params']                                          # what DeviceMeshLoader yields
        with pytest.raises(ValueError, match='must carry its Gaussians'):
            step(bare)
        assert not step._captured
        tight = GraphedTrainStep(model, optim, loss_fn=l1_loss, max_gauss=1)
        with pytest.raises(ValueError, match=r'4 Gaussians in the batch, room for 2\b'):
            tight(batches[1].clone().to(DEV))
        assert not tight._captured
    with pytest.raises(ValueError, match="'fused'.*l1_loss or mse_loss"):
        GraphedTrainStep(model, optim, loss_fn=torch.nn.functional.l1_loss)
    assert not step._captured
