"""CPU checks of the strided Monge-Ampere route (fp64 potential, up to 81 x 81): what tests/test_gpu_ma_strided.py relies on,
proven on the restatements (tests/ma_restatement.py in fp64, tests/ma_strided_restatement.py in the route's mixed arithmetic)
over the shared case table (tests/ma_strided_cases.py), the stored 64 x 64 yardstick, and the API surface that needs no GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ma_restatement as R  # noqa: E402
import ma_strided_cases as SK  # noqa: E402

from g_adaptivity_amd import MeshDataset, _native_mesh, hot_path_opt, ma_batch, square_mesh  # noqa: E402
from g_adaptivity_amd import monge_ampere  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'gadapt_mesh.h')
NEW_SYMBOLS = ('gadapt_ma_strided_max_side', 'gadapt_ma_strided_lds_bytes', 'gadapt_ma_batch_strided')


def test_the_table_covers_every_slot_count_edge():
    assert [SK.slots(SK.CASES[n].N) for n in SK.FIXED] == [1, 1, 2, 2, 3, 4, 5, 7]
    assert [SK.slots(n) for n in (32, 33, 45, 46, 63, 64, 65, 81)] == [1, 2, 2, 3, 4, 4, 5, 7]
    assert 33 * 33 - 1024 == 65                                                    # the second slot of n33_g2


@pytest.mark.parametrize('name', SK.FIXED)
def test_fixed_cases_stay_convex_move_and_the_mixed_form_follows_fp64(name):
    c = SK.CASES[name]
    z64, steps, _, status, lmin = SK.fixed64(name)
    zm, steps_m, _, status_m, lmin_m = SK.fixed_mixed(name)[:5]
    _, noise = SK.noise(name)
    moved = (z64 - torch.stack(R.grid(c.N, torch.float64))).abs().max().item()
    err = (zm.double() - z64).abs().max().item()
    print(f"ma strided {name} N={c.N} K={SK.slots(c.N)}: min lambda {lmin:.3f}, moved {moved:.3e}, mixed - fp64 {err:.3e}, "
          f"noise {noise:.3e}, bar {4 * noise:.3e}")
    assert (steps, status) == (SK.UPDATES, R.CAP) == (steps_m, status_m)
    assert lmin > 0 and lmin_m > 0                                                  # at every evaluation on the way
    assert moved > 1e-3
    assert zm.dtype == torch.float32 and err <= 4 * noise


def test_ds33_converges_convex_untangled_and_equidistributes():
    c = SK.case('ds33')
    xy, steps, res, status, lmin = SK.converged64('ds33')
    y = SK.yardstick('ds33')
    before, after = R.uniform_spread(c.N, c.params), R.cell_spread(xy, c.params)
    print(f"ma strided ds33: stopping steps fp64 / mixed / mixed' {y.j64} / {y.jm} / {y.jmp}, res {res:.3e}, min lambda {lmin:.3f}, "
          f"noise {y.noise:.3e}, cell spread {before:.4f} -> {after:.4f}")
    assert status == R.CONVERGED and res <= SK.TOL and 0 < steps < 20000 and lmin > 0
    assert SK.converged_mixed('ds33')[3] == R.CONVERGED and SK.converged_mixed('ds33', True)[3] == R.CONVERGED
    assert abs(y.jm - y.j64) <= 4 and abs(y.jmp - y.j64) <= 4                       # the mixed form follows fp64
    assert R.triangles_keep_orientation(xy, square_mesh(c.N).cells)
    assert after <= 0.5 * before
    assert (SK.converged_mixed('ds33')[-1].double() - xy).abs().max().item() <= 4 * y.noise


def test_the_stored_64_yardstick_is_self_consistent():
    c = SK.case('ds64')
    f = np.load(SK.GOLDEN)
    assert os.path.getsize(SK.GOLDEN) < 100 * 1024
    assert f['phi64'].dtype == np.float64 and f['phi64'].shape == (64, 64)
    assert np.array_equal(f['gauss'], R.inputs(c.params, torch.float32)[0].numpy())   # the case rebuilt here is the stored one
    phi = torch.from_numpy(f['phi64'])
    gx, gy = R.grid(c.N, torch.float64)
    x, y, r, lam = R.evaluate(phi, c.N, gx, gy, *R.inputs(c.params, torch.float64))
    w1 = torch.ones(c.N, dtype=torch.float64)
    w1[0] = w1[-1] = 0.5
    rbar = (w1[:, None] * w1[None, :] * r).sum() / float((c.N - 1) ** 2)
    res = max((r.max() - rbar).item(), (rbar - r.min()).item())
    steps = [int(v) for v in f['steps']]
    yd = SK.yardstick('ds64')
    before, after = R.uniform_spread(c.N, c.params), R.cell_spread(yd.z64, c.params)
    print(f"ma strided ds64: stored steps fp64 / mixed / mixed' {steps}, res {res:.3e}, min lambda {lam.min().item():.3f}, "
          f"noise {float(f['noise']):.3e}, cell spread {before:.4f} -> {after:.4f}")
    assert res <= SK.TOL and lam.min().item() > 0
    assert max(steps) - min(steps) <= 4 and 20000 > min(steps) > 10000
    assert 0 < float(f['noise']) < 1e-6
    assert torch.equal(yd.z64, torch.stack([x, y])) and (yd.j64, yd.jm, yd.jmp) == tuple(steps)
    assert R.triangles_keep_orientation(yd.z64, square_mesh(c.N).cells) and after <= 0.5 * before


def test_header_declarations_match_the_prototypes():
    hdr = open(HEADER).read()
    kinds = {'int': C.c_int, 'int64_t': C.c_int64, 'double': C.c_double, 'float': C.c_float}
    for name in NEW_SYMBOLS:
        ret, args = re.search(r'^(int64_t|int)\s+' + name + r'\s*\(([^;]*)\);', hdr, flags=re.M).groups()
        res, argtypes = _native_mesh.PROTOTYPES[name]
        assert res is kinds[ret], name
        want = [C.c_void_p if '*' in a else kinds[a.split()[0]] for a in (a.strip() for a in args.split(',')) if a not in ('', 'void')]
        assert argtypes == want, name
    assert _native_mesh.PROTOTYPES['gadapt_ma_batch_strided'] == _native_mesh.PROTOTYPES['gadapt_ma_batch']
    assert '#define GADAPT_MESH_ABI 2' in hdr and _native_mesh.ABI_VERSION == 2     # the ABI grows by addition


def test_limits_and_lds_of_the_library():
    lib = _native_mesh.lib()                                                       # loads without a GPU
    assert lib.gadapt_ma_strided_max_side() == 81 == _native_mesh.MA_STRIDED_MAX_SIDE == monge_ampere.STRIDED_MAX_SIDE
    assert lib.gadapt_ma_max_side() == 32 == monge_ampere.MAX_SIDE                 # the lane route keeps its limit
    assert lib.gadapt_ma_strided_lds_bytes(6561) == 8 * 6561 + 4 * (4 * 16 + 8 * 8) <= 64 * 1024   # one fp64 image
    assert lib.gadapt_ma_strided_lds_bytes(9) == 8 * 9 + 512
    assert lib.gadapt_ma_strided_lds_bytes(8) == _native_mesh.E_SIZE and lib.gadapt_ma_strided_lds_bytes(6562) == _native_mesh.E_SIZE


def test_host_entry_refuses_bad_sizes_before_any_launch():
    """gadapt_ma_batch_strided checks the host copy of the descriptors first: these return their codes without touching a device."""
    lib = _native_mesh.lib()
    one = C.c_void_p(8)                                                            # never dereferenced: the checks come first

    def call(desc, cfl=0.2, tol=1e-4, max_steps=10):
        d = (C.c_int32 * len(desc))(*desc)
        return lib.gadapt_ma_batch_strided(len(desc) // 4, C.cast(d, C.c_void_p), one, one, one, cfl, tol, max_steps, one, one, one,
                                           one, one, None)

    assert call([82, 0, 0, 1]) == _native_mesh.E_SIZE
    msg = lib.gadapt_mesh_last_error()
    assert b'N = 82' in msg and b'81' in msg
    assert call([64, 0, 0, 9]) == _native_mesh.E_SIZE
    assert call([64, 0, 0, 1], max_steps=_native_mesh.MAX_STEPS + 1) == _native_mesh.E_SIZE
    assert call([2, 0, 0, 1]) == -1 and call([64, 0, 0, 1], cfl=0.0) == -1
    assert call([64, -1, 0, 1]) == -1 and call([64, 0, 0, 1], tol=float('nan')) == -1
    assert call([64, 0, 0, 1, 82, 4096, 1, 1]) == _native_mesh.E_SIZE              # the second mesh of a batch is checked too


def test_argument_errors():
    p = dict(SK.CASES['n33_g2'].params)
    assert monge_ampere.ROUTES == ('lane', 'strided')
    with pytest.raises(ValueError, match='nope'):
        ma_batch([11], [p], route='nope')
    with pytest.raises(ValueError, match='81'):
        ma_batch([82], [p], route='strided')
    with pytest.raises(ValueError, match='at least 3'):
        ma_batch([2], [p], route='strided')
    with pytest.raises(ValueError, match='32'):                                    # the lane refusal keeps its wording ...
        ma_batch([33], [p])
    with pytest.raises(ValueError, match="route='strided'"):                       # ... and says where to go
        ma_batch([33], [p], route='lane')
    with pytest.raises(ValueError, match='2-D only'):
        MeshDataset([21], 2, target='monge_ampere', target_params={'solver': {'route': 'strided'}})
    with pytest.raises(TypeError):
        MeshDataset([11, 11], 2, target='monge_ampere', target_params={'solver': {'rout': 'strided'}})
    with pytest.raises(ValueError, match='nope'):
        MeshDataset([11, 11], 2, target='monge_ampere', target_params={'solver': {'route': 'nope'}})


def test_hot_path_opt_lists_the_default_route():
    assert hot_path_opt()['ma_route'] == 'lane' and hot_path_opt()['mmpde5_route'] == 'lane'
    assert hot_path_opt(ma_route='strided')['ma_route'] == 'strided'
