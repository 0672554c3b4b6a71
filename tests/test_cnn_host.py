"""The global CNN features on the HIP kernels, as far as no GPU is needed: the C-ABI's sizes, limits and refusals
(include/gadapt_hip.h, csrc/gadapt_cnn_plan.h), the Python switches around them, and the yardstick of tests/test_gpu_cnn.py."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from cnn_cases import (BACKWARD_LIMITS, BACKWARD_LIMITS_1D, CASES, FLOOR, FORWARD_LIMITS, FORWARD_ONLY, PAST, PAST_FORWARD, PLANTS, make_inputs,
                       params_of, reference, rel, run_restatement)
from g_adaptivity_amd import GNN, MeshDataset, _native as nv, hot_path_opt
from g_adaptivity_amd.features import LDS_BUDGET, GlobalFeatureExtractorCNN, global_cnn, hip_limit
from oracle.pyg_restatement import _GlobalCNN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['gadapt_cnn_forward_lds_bytes', 'gadapt_cnn_backward_lds_bytes', 'gadapt_cnn_workspace_floats', 'gadapt_cnn_param_floats',
       'gadapt_cnn_forward', 'gadapt_cnn_backward']
_buf = (C.c_double * 64)()
P = C.addressof(_buf)                                           # a non-null HOST address: every call below is refused before a launch


def test_header_and_prototypes_agree_for_the_new_symbols():
    header = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'gadapt_hip.h')).read(), flags=re.S)
    for name in NEW:
        ret, args = re.search(r'(\w+)\s+' + name + r'\s*\(([^;{}]*?)\)\s*;', header).groups()
        res, argtypes = nv.PROTOTYPES[name]
        assert res is {'int64_t': C.c_int64, 'int': C.c_int}[ret], name
        want = [C.c_void_p if '*' in a else {'int': C.c_int, 'int64_t': C.c_int64}[a.split()[0]] for a in args.split(',')]
        assert want == argtypes, name
        assert hasattr(nv.lib(), name)
    assert nv.lib().gadapt_abi_version() == 9


@pytest.mark.parametrize('name', list(CASES) + list(PAST))
def test_lds_bytes_follow_the_documented_formulas(name):
    """forward: 2 images, backward: 3, of (n0 + 2)(n1 + 2) max(mid, out) floats, each beside n0 n1 pixel offsets."""
    dim, n0, n1, mid, out, B = {**CASES, **PAST}[name]
    lib = nv.lib()
    image, table = 4 * (n0 + 2) * (n1 + 2) * max(mid, out), 4 * n0 * n1
    assert lib.gadapt_cnn_forward_lds_bytes(dim, n0, n1, mid, out) == 2 * image + table
    assert lib.gadapt_cnn_backward_lds_bytes(dim, n0, n1, mid, out) == 3 * image + table
    taps = 3 ** dim
    assert lib.gadapt_cnn_param_floats(dim, mid, out) == taps * (mid + 2 * mid * mid + mid * out) + 3 * mid + out
    assert lib.gadapt_cnn_workspace_floats(B, dim, n0, n1, mid, out) == B * n0 * n1 * (3 * mid + out)
    fits = lib.gadapt_cnn_backward_lds_bytes(dim, n0, n1, mid, out) <= LDS_BUDGET
    assert fits == (name in CASES)
    assert (hip_limit(dim, n0, n1, mid, out) is None) == fits


def test_backward_limits_are_the_largest_that_fit():
    lib = nv.lib()
    assert LDS_BUDGET == 65536
    for mid, n in BACKWARD_LIMITS.items():
        assert lib.gadapt_cnn_backward_lds_bytes(2, n, n, mid, 8) <= LDS_BUDGET < lib.gadapt_cnn_backward_lds_bytes(2, n + 1, n + 1, mid, 8), mid
        assert lib.gadapt_cnn_forward_lds_bytes(2, n + 1, n + 1, mid, 8) <= LDS_BUDGET          # the forward admits more
    assert lib.gadapt_cnn_backward_lds_bytes(2, 23, 23, 8, 8) == 60000 + 4 * 529
    assert lib.gadapt_cnn_backward_lds_bytes(2, 11, 11, 32, 8) == 65380 and lib.gadapt_cnn_backward_lds_bytes(2, 7, 7, 64, 8) == 62404


def test_1d_backward_limits_are_the_longest_that_fit():
    lib = nv.lib()
    for mid, n in BACKWARD_LIMITS_1D.items():
        assert lib.gadapt_cnn_backward_lds_bytes(1, 1, n, mid, 8) <= LDS_BUDGET < lib.gadapt_cnn_backward_lds_bytes(1, 1, n + 1, mid, 8), mid
        assert lib.gadapt_cnn_forward_lds_bytes(1, 1, n + 1, mid, 8) <= LDS_BUDGET              # the forward admits more
        assert hip_limit(1, 1, n, mid, 8) is None and 'backward' in hip_limit(1, 1, n + 1, mid, 8)
    assert lib.gadapt_cnn_backward_lds_bytes(1, 1, 222, 8, 8) == 65400 and lib.gadapt_cnn_backward_lds_bytes(1, 1, 111, 16, 8) == 65532


def test_forward_limits_are_the_largest_that_fit():
    lib = nv.lib()
    for mid, n in FORWARD_LIMITS.items():
        assert lib.gadapt_cnn_forward_lds_bytes(2, n, n, mid, 8) <= LDS_BUDGET < lib.gadapt_cnn_forward_lds_bytes(2, n + 1, n + 1, mid, 8), mid
        assert n > BACKWARD_LIMITS[mid]
    assert lib.gadapt_cnn_forward_lds_bytes(2, 29, 29, 8, 8) == 64868 and lib.gadapt_cnn_forward_lds_bytes(2, 30, 30, 8, 8) == 69136


def test_forward_only_rows_fit_the_forward_alone():
    """FORWARD_ONLY: refused for a call that records for a backward, taken without one; PAST_FORWARD: refused either way, and the
    sentence names the launch that does not fit."""
    for name, (dim, n0, n1, mid, out, B) in FORWARD_ONLY.items():
        assert hip_limit(dim, n0, n1, mid, out, training=False) is None, name
        assert 'backward' in hip_limit(dim, n0, n1, mid, out, training=True), name
    for name, (dim, n0, n1, mid, out, B) in PAST_FORWARD.items():
        assert 'forward' in hip_limit(dim, n0, n1, mid, out, training=False) and 'backward' not in hip_limit(dim, n0, n1, mid, out, training=False), name
        assert 'backward' in hip_limit(dim, n0, n1, mid, out, training=True), name


def test_size_functions_refuse_bad_sizes():
    lib = nv.lib()
    for f in (lib.gadapt_cnn_forward_lds_bytes, lib.gadapt_cnn_backward_lds_bytes):
        for bad in ((0, 1, 5, 8, 8), (3, 5, 5, 8, 8), (2, 0, 5, 8, 8), (2, 5, 0, 8, 8), (1, 2, 5, 8, 8), (2, 5, 5, 0, 8), (2, 5, 5, 8, 0)):
            assert f(*bad) == -1, bad
    assert lib.gadapt_cnn_workspace_floats(0, 2, 5, 5, 8, 8) == -1
    assert lib.gadapt_cnn_param_floats(3, 8, 8) == -1 and lib.gadapt_cnn_param_floats(2, 0, 8) == -1


FWD_OK = dict(u=P, umax=P, n_meshes=2, dim=2, n0=5, n1=5, mid=8, out=8, w0=P, b0=P, w1=P, b1=P, w2=P, b2=P, w3=P, b3=P, feat=P, acts=P, stream=None)
BWD_OK = dict(d_feat=P, acts=P, u=P, umax=P, n_meshes=2, dim=2, n0=5, n1=5, mid=8, out=8, w0=P, b0=P, w1=P, b1=P, w2=P, b2=P, w3=P, b3=P,
              partials=P, d_params=P, stream=None)
NULL_F = [({k: None}, 'cnn_forward: null pointer') for k in ('u', 'umax', 'feat', 'w0', 'b0', 'w2', 'b3')]
NULL_B = [({k: None}, 'cnn_backward: null pointer') for k in ('d_feat', 'acts', 'u', 'umax', 'partials', 'd_params', 'w1', 'b2')]
SIZES = [({'n_meshes': 0}, 'n_meshes < 1'), ({'dim': 0}, 'dim must be 1 or 2'), ({'dim': 3}, 'dim must be 1 or 2'), ({'n0': 0}, '1 <= n0, n1'),
         ({'n1': -1}, '1 <= n0, n1'), ({'dim': 1}, '(n0 = 1 when dim = 1)'), ({'mid': 0}, '1 <= mid, out'), ({'out': 0}, '1 <= mid, out')]
REFUSALS = [('gadapt_cnn_forward', FWD_OK, b, t) for b, t in NULL_F + SIZES + [
                ({'n0': 40, 'n1': 40}, 'cnn_forward: 2 LDS images'), ({'n0': 12, 'n1': 12, 'mid': 64}, 'above the 65536-byte LDS budget'),
                ({'acts': None, 'dim': 3}, 'dim must be 1 or 2'),
                ({'n0': 30, 'n1': 30}, 'cnn_forward: 2 LDS images'), ({'n0': 30, 'n1': 30}, '= 69136 bytes, above the 65536-byte LDS budget')]] + \
           [('gadapt_cnn_backward', BWD_OK, b, t) for b, t in NULL_B + SIZES + [
                ({'n0': 24, 'n1': 24}, 'cnn_backward: 3 LDS images'), ({'n0': 24, 'n1': 24}, '= 67200 bytes, above the 65536-byte LDS budget'),
                ({'n0': 17, 'n1': 17, 'mid': 16}, 'above the 65536-byte LDS budget'),
                ({'dim': 1, 'n0': 1, 'n1': 223}, '= 65692 bytes, above the 65536-byte LDS budget'),
                ({'dim': 1, 'n0': 1, 'n1': 112, 'mid': 16}, 'cnn_backward: 3 LDS images'), ({'n0': 12, 'n1': 12, 'mid': 32}, 'cnn_backward: 3 LDS images'),
                ({'n0': 8, 'n1': 8, 'mid': 64}, 'cnn_backward: 3 LDS images'), ({'partials': None, 'n_meshes': 1, 'dim': 3}, 'dim must be 1 or 2')]]


@pytest.mark.parametrize('entry,ok,breaks,text', REFUSALS, ids=[f"{e[11:]}-{'+'.join(f'{k}={v}' for k, v in b.items())}" for e, _, b, _ in REFUSALS])
def test_refusal_before_any_launch(entry, ok, breaks, text):
    """Every list here fails a check, so nothing is launched on the host addresses; the code is the library's bad-argument code and the
    message names what was wrong (for a size, the limit)."""
    assert breaks
    lib = nv.lib()
    rc = getattr(lib, entry)(*dict(ok, **breaks).values())
    assert rc == -1 and text in lib.gadapt_last_error().decode(), (rc, lib.gadapt_last_error())


def test_default_route_is_torch_and_its_bits_are_the_four_convolutions():
    assert hot_path_opt()['glob_feat_kernel'] == 'torch'
    for name in ('2d-4x7-m8-o3', '1d-21-m16'):
        dim = CASES[name][0]
        u, module, _ = make_inputs(name)
        assert module.kernel == 'torch'
        conv = F.conv1d if dim == 1 else F.conv2d
        x = u / torch.max(torch.abs(u))
        for c in module.convs:
            x = F.selu(conv(x, c.weight, c.bias, stride=1, padding=1))
        want = (F.adaptive_avg_pool1d(x, 1) if dim == 1 else F.adaptive_avg_pool2d(x, (1, 1))).flatten(1)
        assert torch.equal(module(u), want)


def test_kernel_keyword_and_state_dict_keys():
    with pytest.raises(ValueError):
        GlobalFeatureExtractorCNN(1, 8, 8, kernel='bogus')
    with pytest.raises(ValueError):
        GlobalFeatureExtractorCNN(2, 8, 8, kernel='hip')                # one input channel, four layers only
    with pytest.raises(ValueError):
        GlobalFeatureExtractorCNN(1, 8, 8, num_layers=3, kernel='hip')
    keys = [f'convs.{k}.{t}' for k in range(4) for t in ('weight', 'bias')]
    states = {}
    for kernel in ('torch', 'hip', 'auto'):
        torch.manual_seed(0)
        m = GlobalFeatureExtractorCNN(1, 8, 8, dim=2, kernel=kernel)
        assert list(m.state_dict()) == keys
        states[kernel] = m.state_dict()
    for kernel in ('hip', 'auto'):                                       # the same initialisation, and they load each other's
        assert all(torch.equal(states['torch'][k], states[kernel][k]) for k in keys)
        GlobalFeatureExtractorCNN(1, 8, 8, dim=2, kernel=kernel).load_state_dict(states['torch'], strict=True)
    ds = MeshDataset([7, 7], 2, seed=0)
    for kernel in ('torch', 'hip', 'auto'):
        model = GNN(ds, hot_path_opt(mesh_dims=[7, 7], hidden_dim=16, num_layers=2, gnn_inc_glob_feat_f=True, gnn_inc_glob_feat_uu=True,
                                     glob_feat_kernel=kernel))
        assert model.global_feature_extractor_cnn_f.kernel == kernel and model.global_feature_extractor_cnn_uu.kernel == kernel
        assert sum(k.startswith('global_feature_extractor_cnn_') for k in model.state_dict()) == 16
    with pytest.raises(ValueError):
        GNN(ds, hot_path_opt(mesh_dims=[7, 7], gnn_inc_glob_feat_f=True, glob_feat_kernel='bogus'))


def test_python_side_refusals_need_no_gpu():
    u, module, _ = make_inputs('2d-5x5-m8-scaled')
    ps = params_of(module)
    with pytest.raises(ValueError, match='four layers'):
        global_cnn(u, ps[2:4] + ps[2:], 2)                              # 8 -> 8 channels where 1 -> 8 belongs
    with pytest.raises(ValueError):
        global_cnn(u, ps[:6], 2)
    with pytest.raises(ValueError):
        global_cnn(u[:, 0], ps, 2)                                      # [B, n0, n1]: no channel axis
    with pytest.raises(ValueError, match='no gradient'):
        global_cnn(u.clone().requires_grad_(True), ps, 2)
    with pytest.raises(nv.NativeError, match='no CPU fallback'):
        global_cnn(u, ps, 2)
    with pytest.raises(nv.NativeError):
        GlobalFeatureExtractorCNN(1, 8, 8, dim=2, kernel='hip')(u)
    auto = GlobalFeatureExtractorCNN(1, 8, 8, dim=2, kernel='auto')      # 'auto' on the CPU: torch's bits
    auto.load_state_dict(module.state_dict())
    assert torch.equal(auto(u), module(u))
    assert 'above the 65536-byte budget' in hip_limit(2, 24, 24, 8, 8) and hip_limit(2, 24, 24, 8, 8, training=False) is None


@pytest.mark.parametrize('name', list(CASES))
def test_restatement_is_the_oracle_in_fp64_and_quiet_in_fp32(name):
    dim, n0, n1, mid, out, B = CASES[name]
    ref = reference(name)
    oracle = _GlobalCNN(1, mid, out, dim=dim).double()
    oracle.load_state_dict({k: v.double() for k, v in ref['module'].state_dict().items() if k.startswith('convs.')})
    feat = oracle(ref['u'].double())
    grads = torch.autograd.grad(feat, list(oracle.parameters()), grad_outputs=ref['d_feat'].double())
    assert rel(ref['feat'], feat) <= 1e-12
    for g, want in zip(ref['grads'], grads):
        assert rel(g, want) <= 1e-12
    assert min(g.abs().max().item() for g in grads) > 0.0               # no gradient vanishes
    neg = torch.cat([a.flatten() for a in ref['acts']])
    assert 0.2 < (neg < 0).double().mean().item() < 0.8                 # both SELU branches
    assert max(ref['noise']) < FLOOR, ref['noise']                      # the yardstick is quiet: the floor decides the bar


@pytest.mark.parametrize('name', list(CASES))
def test_cases_meet_their_conditions_on_the_fp64_restatement(name):
    """What tests/cnn_cases.py promises of every row, from the fp64 restatement alone: no gradient is small enough for a relative error
    to hide in (max|g| >= 1e-3 for each of the eight), and both SELU branches run - in every layer of four or more channels between 5 %
    and 95 % of the activations before the pool are negative; narrower layers may be one-sided, the network as a whole is not."""
    dim, n0, n1, mid, out, B = CASES[name]
    ref = reference(name)
    for label, g in zip([f'convs.{k}.{t}' for k in range(4) for t in ('weight', 'bias')], ref['grads']):
        assert g.abs().max().item() >= 1e-3, label
    for l, a in enumerate(ref['acts']):
        assert a.shape == (B, out if l == 3 else mid, n0 * n1)
        if a.shape[1] >= 4:
            assert 0.05 <= (a < 0).double().mean().item() <= 0.95, l
    everything = torch.cat([a.flatten() for a in ref['acts']])
    assert (everything < 0).any() and (everything > 0).any()
    if name in PLANTS:                                                  # the batch maximum sits where the row says, with that sign
        mesh, pixel, factor = PLANTS[name]
        u = ref['u']
        assert u.abs().argmax().item() == mesh * n0 * n1 + pixel and (u.flatten()[u.abs().argmax()] < 0) == (factor < 0)
        assert u.max().item() < 0.5 * u.abs().max().item()              # max u is NOT the scale


def _plan(case):
    """csrc/gadapt_cnn_plan.h restated: pixels; per layer width c the groups of four channels, ceil(c / 4), and whether the last group is
    clamped (c no multiple of 4); units of the widest layer; the workgroup sizes of the forward and the backward by threads_for."""
    dim, n0, n1, mid, out, B = case
    def threads_for(units):
        waves = min(max(units, 4), 16)
        return 64 * ((waves + 3) // 4 * 4)
    pixels = n0 * n1
    units = -(-pixels // 64) * -(-max(mid, out) // 4)
    entries = (mid * mid * 3 ** dim + mid + 63) // 64
    return {'pixels': pixels, 'mid_groups': -(-mid // 4), 'mid_tail': mid % 4, 'out_groups': -(-out // 4), 'out_tail': out % 4, 'units': units,
            'forward_threads': threads_for(units), 'backward_threads': threads_for(max(entries, units))}


# What each row claims about its launch: (pixels, groups of the mid-wide layers, live channels of their clamped tail group or 0, the same two
# for the top layer, units, forward threads, backward threads).  A later edit of a row cannot silently stop it from reaching its edge.
CLAIMS = {
    '2d-5x5-m8-b1': (25, 2, 0, 2, 0, 2, 256, 768),
    '1d-21-m16-b1': (21, 4, 0, 2, 0, 4, 256, 1024),
    '2d-5x5-m4-o8': (25, 1, 0, 2, 0, 2, 256, 256),
    '2d-5x5-m12-o16': (25, 3, 0, 4, 0, 4, 256, 1024),
    '2d-6x5-m3-o5': (30, 1, 3, 2, 1, 2, 256, 256),
    '2d-7x4-m6-o2': (28, 2, 2, 1, 2, 2, 256, 512),
    '2d-5x5-m5-o8': (25, 2, 1, 2, 0, 2, 256, 256),
    '2d-3x3-m1-o1': (9, 1, 1, 1, 1, 1, 256, 256),
    '2d-3x3-m2-o1': (9, 1, 2, 1, 1, 1, 256, 256),
    '2d-1x9-m8': (9, 2, 0, 2, 0, 2, 256, 768),
    '2d-9x1-m8': (9, 2, 0, 2, 0, 2, 256, 768),
    '2d-1x1-m8': (1, 2, 0, 2, 0, 2, 256, 768),
    '2d-2x33-m8': (66, 2, 0, 2, 0, 4, 256, 768),
    '2d-33x2-m8': (66, 2, 0, 2, 0, 4, 256, 768),
    '2d-11x11-m32': (121, 8, 0, 2, 0, 16, 1024, 1024),
    '2d-7x7-m64': (49, 16, 0, 2, 0, 16, 1024, 1024),
    '1d-1-m8': (1, 2, 0, 2, 0, 2, 256, 256),
    '1d-2-m8': (2, 2, 0, 2, 0, 2, 256, 256),
    '1d-64-m8': (64, 2, 0, 2, 0, 2, 256, 256),
    '1d-65-m8': (65, 2, 0, 2, 0, 4, 256, 256),
    '1d-101-m16': (101, 4, 0, 2, 0, 8, 512, 1024),
    '1d-222-m8': (222, 2, 0, 2, 0, 8, 512, 512),
    '1d-111-m16': (111, 4, 0, 2, 0, 8, 512, 1024),
    '2d-3x3-m8-b65': (9, 2, 0, 2, 0, 2, 256, 768),
    '2d-5x5-m8-negmax': (25, 2, 0, 2, 0, 2, 256, 768),
}


@pytest.mark.parametrize('name', list(CLAIMS))
def test_rows_reach_the_launch_plan_they_claim(name):
    assert tuple(_plan(CASES[name]).values()) == CLAIMS[name]


def test_the_rows_cover_the_edges_of_the_launch_plan():
    plans = {name: _plan(case) for name, case in CASES.items()}
    assert plans['1d-64-m8']['pixels'] == 64 and plans['1d-65-m8']['pixels'] == 65
    assert plans['2d-2x33-m8']['pixels'] == 66 == plans['2d-33x2-m8']['pixels']
    assert CASES['2d-6x5-m3-o5'][1] > CASES['2d-6x5-m3-o5'][2] and CASES['2d-7x4-m6-o2'][1] > CASES['2d-7x4-m6-o2'][2]         # n0 > n1
    tails = {name: (p['mid_groups'], p['mid_tail']) for name, p in plans.items()}
    assert tails['2d-3x3-m1-o1'] == (1, 1) and tails['2d-3x3-m2-o1'] == (1, 2)          # a tail group and nothing else
    assert tails['2d-6x5-m3-o5'] == (1, 3)
    assert tails['2d-5x5-m5-o8'] == (2, 1) and tails['2d-7x4-m6-o2'] == (2, 2)          # a full group and a tail
    assert tails['2d-5x5-m12-o16'] == (3, 0) and plans['2d-5x5-m12-o16']['out_groups'] == 4      # more than one group each, out > mid
    assert (plans['2d-6x5-m3-o5']['out_groups'], plans['2d-6x5-m3-o5']['out_tail']) == (2, 1)
    for name in ('2d-5x5-m4-o8', '2d-5x5-m12-o16', '2d-6x5-m3-o5', '2d-5x5-m5-o8'):
        assert CASES[name][4] > CASES[name][3], name                                      # out > mid
    assert {name for name, case in CASES.items() if case[5] == 1} == {'2d-5x5-m8-b1', '1d-21-m16-b1'}
    assert CASES['2d-3x3-m8-b65'][5] == 65
    sizes = {p['forward_threads'] for p in plans.values()} | {p['backward_threads'] for p in plans.values()}
    assert {256, 1024} <= sizes and any(256 < s < 1024 for s in sizes) and sizes <= {256, 512, 768, 1024}
    lib = nv.lib()                                                       # the limit rows sit AT their limits
    for name in ('2d-11x11-m32', '2d-7x7-m64', '1d-222-m8', '1d-111-m16'):
        dim, n0, n1, mid, out, B = CASES[name]
        grown = (n0 + 1, n1 + 1) if dim == 2 else (1, n1 + 1)
        assert lib.gadapt_cnn_backward_lds_bytes(dim, n0, n1, mid, out) <= LDS_BUDGET < lib.gadapt_cnn_backward_lds_bytes(dim, *grown, mid, out), name
