"""The global CNN features on the HIP kernels (`features.global_cnn`, `GlobalFeatureExtractorCNN(kernel='hip')`) on the MI355X.

The yardstick is the fp64 restatement of tests/cnn_restatement.py (equal to the oracle's `_GlobalCNN` in fp64 to 1e-12:
tests/test_cnn_host.py).  ONE bar for the features and each of the eight parameter gradients of every case:

    max |hip - fp64| / max |fp64|  <=  max(4 x noise, 1e-6)

`noise` is the fp32 restatement's own distance from fp64 (the factor 4 is the M2N 'slow' suite's); the floor 1e-6 is where fp32
convolutions sit on these shapes: a tap-by-tap fp32 restatement measured 6e-8 to 1.1e-7 (features) and 1.3e-7 to 3.6e-7 (gradients)
from fp64 on the CPU, torch's own fp32 convolution 6e-8 to 1.6e-6.  Every comparison is printed before it is asserted and recorded in
build/cnn_parity.json (docs/measurements.md has the table)."""
import copy

import pytest
import torch
import torch.nn.functional as F

from cnn_cases import CASES, FLOOR, NAMES, PAST, _module, _record, _run, bar, params_of, reference, rel
from g_adaptivity_amd import GNN, MeshDataset, _native as nv, hot_path_opt
from helpers import hip_model_like, make_case, oracle_fp64_twin, rel_err

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]
COORD_TOL, GRAD_TOL = 1e-5, 1e-4


@pytest.mark.parametrize('name', list(CASES))
def test_features_and_gradients_against_fp64(gpu_device, name):
    ref = reference(name)
    m, u, d_feat = _module(name, gpu_device)
    got = _run(m, u, d_feat)
    again = _run(m, u, d_feat)
    with torch.no_grad():
        plain = m(u)                                                    # no workspace: the same launch without the activation stores
    torch.cuda.synchronize()
    rows, bad = {}, []
    for label, g, want, noise in zip(NAMES, got, [ref['feat']] + ref['grads'], ref['noise']):
        e = rel(g, want)
        rows[label] = {'error': e, 'noise': noise, 'bar': bar(noise), 'margin': bar(noise) / max(e, 1e-300)}
        print(f"{name} {label}: error {e:.2e}, noise {noise:.2e}, bar {bar(noise):.2e}")
        if not e <= bar(noise):
            bad.append((label, e, bar(noise)))
    _record('cases', name, rows)
    assert not bad, bad
    for label, a, b in zip(NAMES, got, again):                          # fixed-order sums, no atomics: the same bits on a second run
        assert torch.equal(a, b), label
    assert torch.equal(plain, got[0])


@pytest.mark.parametrize('name', ['2d-5x5-m8-scaled', '2d-23x23-m8', '2d-5x5-m64', '1d-21-m16'])
def test_a_mesh_does_not_see_its_batch(gpu_device, name):
    """Mesh 0's feature row: the same bits alone and in a batch of 3, when the batch maximum is the same (mesh 0 holds it)."""
    m, u, _ = _module(name, gpu_device)
    u3 = torch.cat([u, u.flip(0)])[:3].clone()
    u3.reshape(3, -1)[0, 1] = 2.0 * u3.abs().max()
    with torch.no_grad():
        alone, three = m(u3[:1].clone()), m(u3)
    assert torch.equal(alone[0], three[0])
    assert not torch.equal(three[0], three[1])


def test_layer_activations_entry_by_entry(gpu_device):
    """The saved activations of the 3 x 3 case against the restatement, every entry of every layer: after the pool a wrong corner tap
    is a small change of a mean, here it is a wrong number.  [4][B, C_l, n0 n1], layer after layer."""
    name = '2d-3x3-m8'
    dim, n0, n1, mid, out, B = CASES[name]
    ref = reference(name)
    m, u, _ = _module(name, gpu_device)
    lib = nv.lib()
    ps = [p.detach().contiguous() for p in params_of(m)]
    acts = torch.full((lib.gadapt_cnn_workspace_floats(B, dim, n0, n1, mid, out),), float('nan'), device=gpu_device)
    feat = torch.empty(B, out, device=gpu_device)
    umax = u.abs().amax()
    nv.check(lib.gadapt_cnn_forward(nv.ptr(u), nv.ptr(umax), B, dim, n0, n1, mid, out, *[nv.ptr(p) for p in ps], nv.ptr(feat), nv.ptr(acts),
                                    nv.current_stream(gpu_device)), 'gadapt_cnn_forward')
    torch.cuda.synchronize()
    at = 0
    for l, want in enumerate(ref['acts']):
        got = acts[at:at + want.numel()].reshape(want.shape).cpu().double()
        at += want.numel()
        worst = ((got - want).abs().max() / want.abs().max()).item()
        print(f"{name} layer {l + 1} activations: worst entry {worst:.2e} of max |A|")
        assert worst <= FLOOR, (l, worst)
    assert at == acts.numel()
    assert rel(feat, ref['feat']) <= bar(ref['noise'][0])


@pytest.mark.parametrize('name', ['2d-4x7-m8-o3', '2d-16x16-m16', '1d-21-m16'])
def test_hip_and_torch_modules_agree(gpu_device, name):
    """Two modules with one state_dict, kernel='hip' and kernel='torch' (MIOpen): the features and the eight gradients within the
    bar of the case.  (One non-square case with out = 3, one at a backward limit, the 1-D layout.)"""
    ref = reference(name)
    hip, u, d_feat = _module(name, gpu_device, 'hip')
    tor, _, _ = _module(name, gpu_device, 'torch')
    a, b = _run(hip, u, d_feat), _run(tor, u, d_feat)
    torch.cuda.synchronize()
    bad = []
    for label, x, y, noise in zip(NAMES, a, b, ref['noise']):
        e = rel(x, y)
        print(f"{name} {label}: hip vs torch {e:.2e}, bar {bar(noise):.2e}; torch vs fp64 {rel(y, ([ref['feat']] + ref['grads'])[NAMES.index(label)]):.2e}")
        if not e <= bar(noise):
            bad.append((label, e, bar(noise)))
    assert not bad, bad


@pytest.mark.parametrize('name', list(PAST))
def test_past_the_limit(gpu_device, name):
    """One size past a backward limit: 'hip' refuses before a launch and names the limit, 'auto' returns what 'torch' returns."""
    hip, u, d_feat = _module(name, gpu_device, 'hip')
    with pytest.raises(nv.NativeError, match='65536-byte budget'):
        hip(u)
    auto, _, _ = _module(name, gpu_device, 'auto')
    tor, _, _ = _module(name, gpu_device, 'torch')
    assert torch.equal(auto(u), tor(u))
    auto(u).backward(d_feat)                                            # and trains through torch's backward
    assert all(p.grad is not None for p in auto.parameters())


# (the two 7 x 7 rows: one mesh in the extractors' backward.  At hidden 4 the extractors have mid = 4 < out = 8, and the encoder keeps the
# first four input columns only, none of them a feature: the 16 extractor gradients are exactly zero in the oracle, and must be here)
MODEL_CASES = {'9x9-C16-b3': ((9, 9), 3, 16), '1d-21-C16-b3': ((21,), 3, 16), '7x7-C8-b1': ((7, 7), 1, 8), '7x7-C4-b1': ((7, 7), 1, 4)}
GLOB = dict(gnn_inc_glob_feat_f=True, gnn_inc_glob_feat_uu=True, glob_feat_kernel='hip')


@pytest.mark.parametrize('case', list(MODEL_CASES))
def test_model_parity_with_hip_features(gpu_device, case):
    """The whole model with both extractors on the HIP kernels against the fp64 oracle: the rule of
    test_gpu_parity.py::test_global_cnn_features_parity, the 16 extractor tensors counted."""
    mesh_dims, batch, hidden = MODEL_CASES[case]
    opt, ds, data, oracle = make_case(mesh_dims, batch, hidden, 2, 'GRAND_plus', **GLOB)
    model = hip_model_like(oracle, ds, opt, gpu_device)
    assert model.global_feature_extractor_cnn_f.kernel == 'hip'
    tgt = data.x_phys if data.x_phys.dim() == 2 else data.x_phys.unsqueeze(-1)
    ref = oracle(data)
    F.mse_loss(ref, tgt).backward()
    o64, ref64 = oracle_fp64_twin(oracle, ds, opt, data, tgt)
    out = model(data.clone().to(gpu_device))
    F.mse_loss(out, tgt.to(gpu_device)).backward()
    torch.cuda.synchronize()
    norm, elem = rel_err(out, ref)
    print(f"{case} x_phys: normwise {norm:.2e} elementwise {elem:.2e}; vs fp64 {rel_err(out, ref64)[0]:.2e}")
    assert norm <= COORD_TOL and elem <= COORD_TOL and rel_err(out, ref64)[0] <= COORD_TOL
    checked, bad, rows = 0, [], {}
    d32, d64 = dict(oracle.named_parameters()), dict(o64.named_parameters())
    for name, ph in model.named_parameters():
        p32, p64 = d32[name], d64[name]
        if p64.grad is None:
            assert ph.grad is None, name
            continue
        if name.endswith('lin_key.bias'):
            continue                                                    # analytically zero; the oracle's is rounding noise
        e64, noise = rel_err(ph.grad, p64.grad)[0], rel_err(p32.grad, p64.grad)[0]
        rows[name] = {'error': e64, 'noise': noise}
        print(f"{case} {name}.grad: {e64:.2e} (fp32 oracle: {noise:.2e})")
        if not e64 <= max(GRAD_TOL, 1.5 * noise):
            bad.append((name, e64, noise))
        checked += name.startswith('global_feature_extractor')
    _record('models', case, rows)
    assert not bad, bad
    assert checked == 16                                                # 2 extractors x 4 convs x (weight, bias)


def test_graphed_replay_equals_the_eager_loop(gpu_device):
    """The 1-D model with both extractors on the HIP kernels: three captured-and-replayed training steps leave the parameters of three
    eager steps, bit for bit - nothing in the route reads the device on the host, and every sum has a fixed order."""
    from g_adaptivity_amd import DeviceMeshLoader, GraphedTrainStep
    from g_adaptivity_amd.optim import FlatAdam
    opt = hot_path_opt(mesh_dims=[21], hidden_dim=16, num_layers=2, device=str(gpu_device), lr=1e-3, **GLOB)
    ds = MeshDataset([21], 3, seed=3)
    torch.manual_seed(0)
    base = GNN(ds, opt).to(gpu_device).train()
    state = copy.deepcopy(base.state_dict())
    res = []
    for graphed in (False, True):
        m = GNN(ds, opt).to(gpu_device).train(); m.load_state_dict(copy.deepcopy(state))
        o = FlatAdam(m.parameters(), lr=opt['lr'], capturable=True)
        step = GraphedTrainStep(m, o, loss_fn=lambda out, t: F.mse_loss(out, t.reshape(out.shape)))     # 1-D: x_phys is [N]
        for _ in range(3):
            for d in DeviceMeshLoader(ds, batch_size=3, shuffle=False, device=gpu_device):
                (step if graphed else step.eager)(d)
        torch.cuda.synchronize()
        if graphed:
            assert len(step._captured) == 1
        res.append({n: p.detach().clone() for n, p in m.named_parameters()})
    moved = 0
    for n, p0 in base.named_parameters():
        assert torch.equal(res[0][n], res[1][n]), n
        moved += int(n.startswith('global_feature_extractor') and not torch.equal(res[0][n], p0))
    assert moved == 16
