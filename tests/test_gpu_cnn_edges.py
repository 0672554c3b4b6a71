"""The global CNN kernels (`csrc/gadapt_cnn.inc`) at their channel, batch, LDS and layout edges, on the MI355X: what the rows of
tests/cnn_cases.py cannot show through `test_gpu_cnn.py::test_features_and_gradients_against_fp64` alone.

The rule is that file's and nothing looser: max |hip - fp64| / max |fp64| <= max(4 x noise, 1e-6) against the fp64 restatement, the
saved activations entry by entry under the floor 1e-6, and `torch.equal` wherever two calls of the kernels must give the same bits.
Every comparison is printed before it is asserted and recorded in build/cnn_parity.json."""
import pytest
import torch
import torch.nn as nn

from cnn_cases import CASES, FLOOR, FORWARD_ONLY, NAMES, PAST_FORWARD, _module, _record, _run, bar, params_of, reference, rel, run_restatement
from g_adaptivity_amd import _native as nv

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]


def _judge(section, name, got, want, noise, labels=NAMES):
    """Prints and records error / noise / bar of every tensor; returns the ones past their bar."""
    rows, bad = {}, []
    for label, g, w, n in zip(labels, got, want, noise):
        e = rel(g, w)
        rows[label] = {'error': e, 'noise': n, 'bar': bar(n), 'margin': bar(n) / max(e, 1e-300)}
        print(f"{name} {label}: error {e:.2e}, noise {n:.2e}, bar {bar(n):.2e}")
        if not e <= bar(n):
            bad.append((label, e, bar(n)))
    _record(section, name, rows)
    return bad


def _same_bits(name, what, a, b, labels=NAMES):
    """Nine tensors (or fewer) of two runs, bit for bit."""
    assert len(a) == len(b)
    for label, x, y in zip(labels, a, b):
        same = torch.equal(x, y)
        print(f"{name} {what} {label}: {'the same bits' if same else f'DIFFERENT, {rel(x, y):.2e} apart'}")
        assert same, (what, label)


ACTIVATION_ROWS = {'2d-6x5-m3-o5': None, '2d-5x5-m4-o8': None, '2d-9x1-m8': None, '1d-21-m16-b1': None, '2d-3x3-m8-b65': [0, 63, 64]}


@pytest.mark.parametrize('name', list(ACTIVATION_ROWS))
def test_layer_activations_entry_by_entry(gpu_device, name):
    """The saved activations against the restatement, every entry of every layer ([4][B, C_l, n0 n1], layer after layer; C_4 = out):
    after the pool a wrong channel or a transposed stride is a small change of a mean, here it is a wrong number.  The workspace is
    NaN before the launch, so an entry nobody wrote shows too."""
    dim, n0, n1, mid, out, B = CASES[name]
    meshes = ACTIVATION_ROWS[name] or list(range(B))
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
    assert not torch.isnan(acts).any()
    at, rows = 0, {}
    for l, want in enumerate(ref['acts']):
        assert want.shape == (B, out if l == 3 else mid, n0 * n1)
        got = acts[at:at + want.numel()].reshape(want.shape).cpu().double()
        at += want.numel()
        worst = ((got[meshes] - want[meshes]).abs().max() / want.abs().max()).item()
        rows[f'layer {l + 1}'] = {'error': worst, 'bar': FLOOR}
        print(f"{name} layer {l + 1} activations: worst entry {worst:.2e} of max |A|")
    _record('activations', name, rows)
    assert all(r['error'] <= FLOOR for r in rows.values()), rows
    assert at == acts.numel()
    assert rel(feat, ref['feat']) <= bar(ref['noise'][0])


@pytest.mark.parametrize('name', list(FORWARD_ONLY))
def test_forward_only_images(gpu_device, name):
    """Past the backward limit, within the forward's: taken under `no_grad` and with frozen parameters (no workspace, two LDS images),
    by 'hip' and by 'auto' alike; with trainable parameters under grad 'auto' hands the image to torch."""
    ref = reference(name)
    hip, u, _ = _module(name, gpu_device, 'hip')
    auto, _, _ = _module(name, gpu_device, 'auto')
    tor, _, _ = _module(name, gpu_device, 'torch')
    with torch.no_grad():
        first, second, chosen = hip(u), hip(u), auto(u)
    torch.cuda.synchronize()
    bad = _judge('forward_only', name, [first], [ref['feat']], ref['noise'])
    assert not bad, bad
    _same_bits(name, 'second call', [first], [second])
    _same_bits(name, "'auto' under no_grad", [first], [chosen])
    trained = auto(u)                                                   # grad on, trainable: the backward would not fit
    assert trained.requires_grad and torch.equal(trained, tor(u))
    for p in hip.parameters():
        p.requires_grad_(False)
    frozen = hip(u)                                                     # grad mode on, nothing to train: the same path
    _same_bits(name, 'frozen parameters', [first], [frozen])
    assert not frozen.requires_grad


@pytest.mark.parametrize('name', list(PAST_FORWARD))
def test_past_the_forward_limit(gpu_device, name):
    hip, u, _ = _module(name, gpu_device, 'hip')
    auto, _, _ = _module(name, gpu_device, 'auto')
    tor, _, _ = _module(name, gpu_device, 'torch')
    with torch.no_grad():
        with pytest.raises(nv.NativeError, match='the forward of a 30 x 30 image'):
            hip(u)
        assert torch.equal(auto(u), tor(u))


def test_frozen_first_layer(gpu_device):
    """`convs.0` frozen: the six other gradients keep their bits, the frozen two stay None."""
    name = '2d-5x5-m5-o8'
    m, u, d_feat = _module(name, gpu_device)
    full = _run(m, u, d_feat)
    m.convs[0].requires_grad_(False)
    m.zero_grad(set_to_none=True)
    feat = m(u)
    feat.backward(d_feat)
    torch.cuda.synchronize()
    assert m.convs[0].weight.grad is None and m.convs[0].bias.grad is None
    _same_bits(name, 'convs.0 frozen', [full[0]] + full[3:], [feat.detach()] + [p.grad for p in params_of(m)[2:]], NAMES[:1] + NAMES[3:])
    assert len(full[3:]) == 6


def test_a_mesh_does_not_see_its_batch_beyond_mesh_2(gpu_device):
    """Mesh 64 of 65: its feature row has the same bits alone and in the batch when the batch maximum is the same (mesh 64 holds it), and
    so has mesh 0's when mesh 0 holds it; the gradients of mesh 64 run alone (one mesh: no partials, no reduce) against the fp64
    restatement of that single mesh."""
    name = '2d-3x3-m8-b65'
    dim = CASES[name][0]
    m, u, d_feat = _module(name, gpu_device)
    top = 2.0 * u.abs().max()
    last, first = u.clone(), u.clone()
    last.reshape(65, -1)[64, 1] = top
    first.reshape(65, -1)[0, 1] = top
    with torch.no_grad():
        batch, alone = m(last), m(last[64:].clone())
        batch0, alone0 = m(first), m(first[:1].clone())
    _same_bits(name, 'mesh 64 alone / in the batch', [alone[0]], [batch[64]])
    _same_bits(name, 'mesh 0 alone / in the batch', [alone0[0]], [batch0[0]])
    assert not torch.equal(batch[64], batch[63]) and not torch.equal(batch[64], batch0[64])
    one, seed = last[64:].clone(), d_feat[64:].clone()
    got = _run(m, one, seed)
    torch.cuda.synchronize()
    ps = [p.detach().cpu() for p in params_of(m)]
    f64, g64, _ = run_restatement(one.cpu(), ps, seed.cpu(), dim, torch.float64)
    f32, g32, _ = run_restatement(one.cpu(), ps, seed.cpu(), dim, torch.float32)
    noise = [rel(f32, f64)] + [rel(a, b) for a, b in zip(g32, g64)]
    bad = _judge('isolation', name + '/mesh-64-alone', got, [f64] + g64, noise)
    assert not bad, bad


def _layout_case(gpu_device):
    m, u, d_feat = _module('2d-4x7-m8-o3', gpu_device)
    return m, u, d_feat, _run(m, u, d_feat)


def test_field_layouts(gpu_device):
    """The field as `field_to_grid` hands it over (a transposed, flipped 7 x 4 base), as a slice of a larger batch, and as one mesh
    expanded to three: the bits of the contiguous call, features and all eight gradients."""
    name = '2d-4x7-m8-o3'
    m, u, d_feat, want = _layout_case(gpu_device)
    base = u.flip(2).transpose(2, 3).contiguous()                       # [B, 1, 7, 4]
    grid = base.transpose(2, 3).flip(2)
    assert grid.shape == u.shape and torch.equal(grid, u)
    print(f"{name} transposed and flipped: strides {grid.stride()}, contiguous {grid.is_contiguous()}")
    _same_bits(name, 'transpose(2, 3).flip(2) of a 7 x 4 base', want, _run(m, grid, d_feat))
    turned = base.transpose(2, 3)                                       # the transposed view itself, no copy behind it
    assert not turned.is_contiguous()
    _same_bits(name, 'transposed view', _run(m, turned.contiguous(), d_feat), _run(m, turned, d_feat))
    big = torch.cat([torch.full_like(u[:1], 100.0), u, torch.full_like(u, -100.0)])
    part = big[1:3]
    assert part.storage_offset() == u[0].numel() and torch.equal(part, u)
    _same_bits(name, 'slice of a larger batch', want, _run(m, part, d_feat))
    three = u[1:2].expand(3, -1, -1, -1)
    assert three.stride(0) == 0
    seed3 = torch.cat([d_feat, d_feat[:1] * 0.5])
    _same_bits(name, 'expanded mesh', _run(m, u[1:2].repeat(3, 1, 1, 1), seed3), _run(m, three, seed3))


def test_upstream_gradient_layouts(gpu_device):
    """`feat.sum().backward()` hands an expanded, zero-stride d_feat; a transposed-storage d_feat has the strides (1, B)."""
    name = '2d-4x7-m8-o3'
    m, u, d_feat, want = _layout_case(gpu_device)
    ones = _run(m, u, torch.ones_like(d_feat))
    m.zero_grad(set_to_none=True)
    feat = m(u)
    feat.sum().backward()
    _same_bits(name, 'feat.sum().backward()', ones, [feat.detach()] + [p.grad for p in params_of(m)])
    turned = d_feat.t().contiguous().t()
    assert turned.stride() == (1, d_feat.shape[0]) and torch.equal(turned, d_feat)
    _same_bits(name, 'transposed-storage d_feat', want, _run(m, u, turned))


def test_parameter_on_non_contiguous_storage(gpu_device):
    name = '2d-4x7-m8-o3'
    m, u, d_feat, want = _layout_case(gpu_device)
    w = m.convs[1].weight.detach()
    m.convs[1].weight = nn.Parameter(w.permute(3, 2, 1, 0).contiguous().permute(3, 2, 1, 0))
    held = m.convs[1].weight
    assert not held.is_contiguous() and torch.equal(held, w)
    got = _run(m, u, d_feat)
    assert held.grad.shape == held.shape == w.shape
    _same_bits(name, 'convs.1.weight on permuted storage', want, got)


@pytest.mark.parametrize('name', ['2d-5x5-m4-o8', '2d-6x5-m3-o5', '2d-5x5-m8-b1', '1d-101-m16'])
def test_hip_and_torch_modules_agree(gpu_device, name):
    """Two modules with one state_dict, kernel='hip' and kernel='torch' (MIOpen): the features and the eight gradients within the
    bar of the case.  (out > mid, a tail group with n0 > n1, one mesh, the fine 1-D size.)"""
    ref = reference(name)
    hip, u, d_feat = _module(name, gpu_device, 'hip')
    tor, _, _ = _module(name, gpu_device, 'torch')
    a, b = _run(hip, u, d_feat), _run(tor, u, d_feat)
    torch.cuda.synchronize()
    for label, y, want in zip(NAMES, b, [ref['feat']] + ref['grads']):
        print(f"{name} {label}: torch vs fp64 {rel(y, want):.2e}")
    bad = _judge('hip_vs_torch', name, a, b, ref['noise'])
    assert not bad, bad
