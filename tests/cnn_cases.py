"""The cases of the global CNN features on the HIP kernels (`features.global_cnn`), with the claim each row exists for, and the
shared fp64 yardstick of each (computed once per session, never changed).

A case is (dim, n0, n1, mid, out, B); 1-D is n0 = 1.  Inputs are fixed-seed `randn` images (optionally scaled per mesh), the weights
are the modules' own initialisation under a fixed seed, the upstream gradient is `randn`.  About half the activations are negative on
these inputs, so both SELU branches run; no gradient vanishes.

Conditions every row of CASES meets, proven on the fp64 restatement alone in tests/test_cnn_host.py (nothing a kernel computes enters a
case or a bar): each of the eight fp64 gradients has max|g| >= 1e-3; in every layer of four or more channels the share of negative
activations before the pool lies in [0.05, 0.95]; in narrower layers both SELU branches occur somewhere in the network.  The seeds as
they stand meet them on every row, so no row carries a seed offset."""
import functools
import json
import os

import torch

from cnn_restatement import restatement
from g_adaptivity_amd.features import GlobalFeatureExtractorCNN

CASES = {
    # every pixel touches the zero border; 9 pixels in a 64-lane wave
    '2d-3x3-m8': (2, 3, 3, 8, 8, 2),
    # non-square (a transposed stride shows) and an output width that is no multiple of the 4 channels of a wave's unit
    '2d-4x7-m8-o3': (2, 4, 7, 8, 3, 2),
    # meshes scaled 1 : 10 : 0.1 - the normalisation is by the BATCH maximum; per-mesh offsets into u, feat and the workspace
    '2d-5x5-m8-scaled': (2, 5, 5, 8, 8, 3),
    # exactly 64 and 256 pixels: full units, no dead lane
    '2d-8x8-m8': (2, 8, 8, 8, 8, 2),
    '2d-16x16-m8': (2, 16, 16, 8, 8, 2),
    # 529 pixels: more than one pass per lane, a last unit of 17 live lanes; the backward limit at 8 channels
    '2d-23x23-m8': (2, 23, 23, 8, 8, 2),
    # wider channels at their backward limit (16 x 16 at 16) or near it (9 x 9 at 32; the limit is 11 x 11)
    '2d-16x16-m16': (2, 16, 16, 16, 8, 2),
    '2d-9x9-m32': (2, 9, 9, 32, 8, 2),
    # the widest supported hidden size: 36 864 weight-gradient entries per layer over a 1024-thread workgroup
    '2d-5x5-m64': (2, 5, 5, 64, 8, 2),
    # Conv1d weight layout [out, in, 3]; the Burgers size
    '1d-3-m8': (1, 1, 3, 8, 8, 3),
    '1d-21-m16': (1, 1, 21, 16, 8, 3),
    # one mesh: the backward writes its gradients straight to d_params, there is no partials buffer and no reduce launch
    '2d-5x5-m8-b1': (2, 5, 5, 8, 8, 1),
    '1d-21-m16-b1': (1, 1, 21, 16, 8, 1),
    # out > mid: the LDS image is sized by out, the top layer's activations sit at 3 B mid P + mesh out P, and the backward's G / N swap
    # leaves out - mid stale planes behind; one group each, then more than one group each
    '2d-5x5-m4-o8': (2, 5, 5, 4, 8, 2),
    '2d-5x5-m12-o16': (2, 5, 5, 12, 16, 2),
    # n0 > n1; mid 3 is one tail group only (three live channels, one clamped); out 5 > mid is a full group and a tail of one
    '2d-6x5-m3-o5': (2, 6, 5, 3, 5, 2),
    # n0 > n1; mid 6 is one full group and a tail of two; out 2 a tail group alone
    '2d-7x4-m6-o2': (2, 7, 4, 6, 2, 2),
    # mid 5: a tail of one channel in the three mid-wide forward layers and in the ci groups of the backward's transposed convolution
    '2d-5x5-m5-o8': (2, 5, 5, 5, 8, 2),
    # one channel everywhere: every lane group is clamped to channel 0; and two channels
    '2d-3x3-m1-o1': (2, 3, 3, 1, 1, 2),
    '2d-3x3-m2-o1': (2, 3, 3, 2, 1, 2),
    # dim 2 with a single row (every pixel touches the top and the bottom border), a single column (w2 = 3: every tap but those of the
    # centre column reads the border) and a single pixel (u / max is +-1, the pool divides by 1)
    '2d-1x9-m8': (2, 1, 9, 8, 8, 2),
    '2d-9x1-m8': (2, 9, 1, 8, 8, 2),
    '2d-1x1-m8': (2, 1, 1, 8, 8, 2),
    # 66 pixels, a wave and two lanes, in both orientations
    '2d-2x33-m8': (2, 2, 33, 8, 8, 2),
    '2d-33x2-m8': (2, 33, 2, 8, 8, 2),
    # the backward limits at mid 32 (65 380 bytes) and at mid 64 (62 404 bytes)
    '2d-11x11-m32': (2, 11, 11, 32, 8, 2),
    '2d-7x7-m64': (2, 7, 7, 64, 8, 2),
    # the smallest 1-D images: no interior pixel
    '1d-1-m8': (1, 1, 1, 8, 8, 2),
    '1d-2-m8': (1, 1, 2, 8, 8, 2),
    # exactly one wave of pixels, and one pixel more
    '1d-64-m8': (1, 1, 64, 8, 8, 2),
    '1d-65-m8': (1, 1, 65, 8, 8, 2),
    # the workload's fine 1-D size
    '1d-101-m16': (1, 1, 101, 16, 8, 2),
    # the 1-D backward limits: 65 400 bytes at mid 8, 65 532 at mid 16 (four under the budget)
    '1d-222-m8': (1, 1, 222, 8, 8, 2),
    '1d-111-m16': (1, 1, 111, 16, 8, 2),
    # mesh indices past one wave's worth in every per-mesh offset (u, feat, workspace, partials); a 65-term serial reduce
    '2d-3x3-m8-b65': (2, 3, 3, 8, 8, 65),
    # the batch maximum of |u| sits on a NEGATIVE entry (one pixel of mesh 0 is -3 max|u|): the scale is max|u|, not max u
    '2d-5x5-m8-negmax': (2, 5, 5, 8, 8, 2),
}
SCALES = {'2d-5x5-m8-scaled': (1.0, 10.0, 0.1)}
# SCALES' sibling: (mesh, pixel, factor) - that pixel of that mesh is set to factor x max|u| of the drawn batch
PLANTS = {'2d-5x5-m8-negmax': (0, 7, -3.0)}
# one size past each backward limit: refused before a launch under 'hip', taken by torch under 'auto'
PAST = {'2d-24x24-m8': (2, 24, 24, 8, 8, 2), '2d-17x17-m16': (2, 17, 17, 16, 8, 2), '1d-223-m8': (1, 1, 223, 8, 8, 2),
        '1d-112-m16': (1, 1, 112, 16, 8, 2), '2d-12x12-m32': (2, 12, 12, 32, 8, 2), '2d-8x8-m64': (2, 8, 8, 64, 8, 2)}
# past the backward limit, within the forward's: taken under no_grad or with frozen parameters only (29 x 29: 64 868 bytes, the limit)
FORWARD_ONLY = {'2d-24x24-m8': (2, 24, 24, 8, 8, 2), '2d-29x29-m8': (2, 29, 29, 8, 8, 2)}
# one size past the forward limit (69 136 bytes): refused under no_grad too
PAST_FORWARD = {'2d-30x30-m8': (2, 30, 30, 8, 8, 2)}
ALL = {**CASES, **PAST, **FORWARD_ONLY, **PAST_FORWARD}
# the largest 2-D square image whose backward fits 65 536 bytes of LDS, per mid (out = 8); the longest 1-D image; the largest forward
BACKWARD_LIMITS = {8: 23, 16: 16, 32: 11, 64: 7}
BACKWARD_LIMITS_1D = {8: 222, 16: 111}
FORWARD_LIMITS = {8: 29}
NAMES = ['feat'] + [f'convs.{k}.{t}' for k in range(4) for t in ('weight', 'bias')]
FLOOR = 1e-6                  # the floor of the bar max(4 x noise, FLOOR): tests/test_gpu_cnn.py


def make_inputs(name, case=None):
    """(u [B, 1, (n0,) n1] fp32, module (kernel='torch', CPU), d_feat [B, out] fp32): the same for every test of the case."""
    dim, n0, n1, mid, out, B = case or ALL[name]
    gen = torch.Generator().manual_seed(1234 + 17 * n0 + 31 * n1 + mid + out + dim)
    u = torch.randn((B, 1, n1) if dim == 1 else (B, 1, n0, n1), generator=gen)
    for b, s in enumerate(SCALES.get(name, ())):
        u[b] *= s
    if name in PLANTS:
        mesh, pixel, factor = PLANTS[name]
        u[mesh].view(-1)[pixel] = factor * u.abs().max()
    d_feat = torch.randn(B, out, generator=gen)
    torch.manual_seed(4321 + mid + out + dim)
    return u, GlobalFeatureExtractorCNN(1, mid, out, dim=dim), d_feat


def params_of(module):
    return [t for conv in module.convs for t in (conv.weight, conv.bias)]


def run_restatement(u, params, d_feat, dim, dtype):
    """feat, the eight parameter gradients under the seed d_feat, and the four layers' activations, all in `dtype` on the CPU."""
    ps = [p.detach().to(dtype).requires_grad_(True) for p in params]
    feat, acts = restatement(u.to(dtype), ps, dim)
    grads = torch.autograd.grad(feat, ps, grad_outputs=d_feat.to(dtype))
    return feat.detach(), [g.detach() for g in grads], [a.detach() for a in acts]


def rel(a, b):
    """max |a - b| / max |b|"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@functools.lru_cache(maxsize=None)
def reference(name):
    """The yardstick of a case: the fp64 restatement and `noise`, the fp32 restatement's distance from it (feat first, then the eight
    gradients)."""
    dim = ALL[name][0]
    u, module, d_feat = make_inputs(name)
    f64, g64, a64 = run_restatement(u, params_of(module), d_feat, dim, torch.float64)
    f32, g32, _ = run_restatement(u, params_of(module), d_feat, dim, torch.float32)
    noise = [rel(f32, f64)] + [rel(a, b) for a, b in zip(g32, g64)]
    return {'u': u, 'module': module, 'd_feat': d_feat, 'feat': f64, 'grads': g64, 'acts': a64, 'noise': noise}


def bar(noise):
    return max(4.0 * noise, FLOOR)


_LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'build', 'cnn_parity.json')


def _record(section, name, rows):
    os.makedirs(os.path.dirname(_LOG), exist_ok=True)
    try:
        log = json.load(open(_LOG))
    except Exception:
        log = {'rule': 'max|hip - fp64| / max|fp64| <= max(4 * noise, 1e-6); noise = fp32 restatement vs fp64'}
    log.setdefault(section, {})[name] = rows
    json.dump(log, open(_LOG, 'w'), indent=1)


def _module(name, dev, kernel='hip', case=None):
    u, cpu, d_feat = make_inputs(name, case)
    dim, _, _, mid, out, _ = case or ALL[name]
    m = GlobalFeatureExtractorCNN(1, mid, out, dim=dim, kernel=kernel).to(dev)
    m.load_state_dict(cpu.state_dict())
    return m, u.to(dev), d_feat.to(dev)


def _run(m, u, d_feat):
    m.zero_grad(set_to_none=True)
    feat = m(u)
    feat.backward(d_feat)
    return [feat.detach().clone()] + [p.grad.detach().clone() for p in params_of(m)]
