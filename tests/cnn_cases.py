"""The cases of the global CNN features on the HIP kernels (`features.global_cnn`), with the claim each row exists for, and the
shared fp64 yardstick of each (computed once per session, never changed).

A case is (dim, n0, n1, mid, out, B); 1-D is n0 = 1.  Inputs are fixed-seed `randn` images (optionally scaled per mesh), the weights
are the modules' own initialisation under a fixed seed, the upstream gradient is `randn`.  About half the activations are negative on
these inputs, so both SELU branches run; no gradient vanishes."""
import functools

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
}
SCALES = {'2d-5x5-m8-scaled': (1.0, 10.0, 0.1)}
# one size past each backward limit: refused before a launch under 'hip', taken by torch under 'auto'
PAST = {'2d-24x24-m8': (2, 24, 24, 8, 8, 2), '2d-17x17-m16': (2, 17, 17, 16, 8, 2)}
# the largest 2-D square image whose backward fits 65 536 bytes of LDS, per mid (out = 8)
BACKWARD_LIMITS = {8: 23, 16: 16, 32: 11, 64: 7}
FLOOR = 1e-6                  # the floor of the bar max(4 x noise, FLOOR): tests/test_gpu_cnn.py


def make_inputs(name, case=None):
    """(u [B, 1, (n0,) n1] fp32, module (kernel='torch', CPU), d_feat [B, out] fp32): the same for every test of the case."""
    dim, n0, n1, mid, out, B = case or {**CASES, **PAST}[name]
    gen = torch.Generator().manual_seed(1234 + 17 * n0 + 31 * n1 + mid + out + dim)
    u = torch.randn((B, 1, n1) if dim == 1 else (B, 1, n0, n1), generator=gen)
    for b, s in enumerate(SCALES.get(name, ())):
        u[b] *= s
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
    dim = CASES[name][0]
    u, module, d_feat = make_inputs(name)
    f64, g64, a64 = run_restatement(u, params_of(module), d_feat, dim, torch.float64)
    f32, g32, _ = run_restatement(u, params_of(module), d_feat, dim, torch.float32)
    noise = [rel(f32, f64)] + [rel(a, b) for a, b in zip(g32, g64)]
    return {'u': u, 'module': module, 'd_feat': d_feat, 'feat': f64, 'grads': g64, 'acts': a64, 'noise': noise}


def bar(noise):
    return max(4.0 * noise, FLOOR)
