"""CPU checks of the Monge-Ampere target meshes: what tests/test_gpu_ma.py relies on, proven on the fp64 restatement of the
iteration (tests/ma_restatement.py) over the shared case table (tests/ma_cases.py), and the API surface of
g_adaptivity_amd.monge_ampere that needs no GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ma_cases as K  # noqa: E402
import ma_restatement as R  # noqa: E402

from g_adaptivity_amd import (MA2d, MeshDataset, MixedMeshDataset, _native_mesh, deform_mesh_ma2d, ma_batch, monitor_ma,  # noqa: E402
                              square_mesh)
from g_adaptivity_amd._native import NativeError  # noqa: E402
from g_adaptivity_amd.monge_ampere import CAP, CONVERGED, NONCONVEX  # noqa: E402


@pytest.mark.parametrize('name', list(K.CASES))
def test_fp64_restatement_converges_convex_untangled_and_equidistributes(name):
    c = K.CASES[name]
    xy, steps, res, status, lmin = K.converged(name, 'fp64')
    before, after = R.uniform_spread(c.N, c.params), R.cell_spread(xy, c.params)
    print(f"{name}: {steps} updates, res {res:.3e}, min lambda {lmin:.3f}, cell spread {before:.4f} -> {after:.4f}")
    assert status == R.CONVERGED and res <= K.TOL and 0 < steps < 20000
    assert lmin > 0                                                    # at every evaluation on the way
    assert R.triangles_keep_orientation(xy, square_mesh(c.N).cells)
    assert after <= 0.5 * before
    # the Neumann condition as the reflection builds it: boundary nodes keep their normal coordinate, corners stay
    gx, gy = R.grid(c.N, torch.float64)
    assert torch.equal(xy[0][0], gx[0]) and torch.equal(xy[0][-1], gx[-1])
    assert torch.equal(xy[1][:, 0], gy[:, 0]) and torch.equal(xy[1][:, -1], gy[:, -1])


@pytest.mark.parametrize('name', K.FIXED)
def test_fixed_step_cases_move_by_more_than_rounding(name):
    """A comparison after a fixed number of updates means something only if the nodes moved: by at least 1 000 spacings of
    fp32 at 1.0 in the fp64 restatement."""
    c = K.CASES[name]
    xy, steps, _, status, _ = K.fixed(name, 'fp64')
    assert steps == c.updates and status == R.CAP
    assert (xy - torch.stack(R.grid(c.N, torch.float64))).abs().max().item() >= 1000 * 2.0 ** -23


@pytest.mark.parametrize('precision', ['fp32', 'fp64'])
def test_cfl_one_loses_convexity_after_one_update(precision):
    """The case of the GPU status test, with room to spare: min lambda is -0.167 after the first update."""
    c = K.CASES['narrow11']
    dtype = {'fp32': torch.float32, 'fp64': torch.float64}[precision]
    _, steps, _, status, lmin = R.ma(c.N, c.params, dtype=dtype, cfl=1.0)
    assert status == R.NONCONVEX and steps == 1 and lmin < -0.1


@pytest.mark.parametrize('name', list(K.CASES))
def test_cfl_one_loses_convexity_in_every_case(name):
    """Wider Gaussians survive the first update and lose convexity a few updates later: never a quiet wrong mesh."""
    c = K.CASES[name]
    for dtype in (torch.float32, torch.float64):
        _, steps, _, status, lmin = R.ma(c.N, c.params, dtype=dtype, cfl=1.0, max_steps=50)
        assert status == R.NONCONVEX and 1 <= steps < 50 and not lmin > 0


def test_five_steps_reach_the_cap():
    c = K.CASES['narrow11']
    _, steps, res, status, _ = R.ma(c.N, c.params, max_steps=5)
    assert status == R.CAP and steps == 5 and res > K.TOL


def test_constant_monitor_is_the_grid():
    xy, steps, _, status, _ = R.ma(11, {'centers': [], 'scales': []})
    assert steps == 0 and status == R.CONVERGED and torch.equal(xy, torch.stack(R.grid(11, torch.float32)))


def test_monitor_ma_is_the_restated_monitor_and_signed():
    c = K.CASES['n11_g8']
    gx, gy = R.grid(33, torch.float64)
    want = R.monitor(gx, gy, *R.inputs(c.params, torch.float64))                # mon_reg and mon_power rounded to fp32 there: 6e-8
    assert torch.allclose(monitor_ma(gx, gy, c.params), want, rtol=1e-6, atol=0)
    plain = {k: c.params[k] for k in ('centers', 'scales')}
    dflt = R.monitor(gx, gy, *R.inputs(plain, torch.float64))
    assert torch.allclose(monitor_ma(gx, gy, plain), dflt, rtol=1e-6, atol=0) and dflt.min().item() >= 1.0
    # signed sums (diag_hessian_ma), not monitor_2d's per-Gaussian absolute values: with mon_reg = 0 and mon_power = 1 its square
    # is u_xx^2 + u_yy^2, equal to monitor_2d - 1 for one Gaussian and below it wherever two Gaussians' curvatures cancel
    from g_adaptivity_amd import monitor_2d
    for count, cancels in ((1, False), (2, True)):
        p = dict(K.drawn(5, count), mon_reg=0.0, mon_power=1.0)
        signed, absolute = monitor_ma(gx, gy, p) ** 2, monitor_2d(gx, gy, p) - 1
        assert (signed <= absolute * (1 + 1e-12) + 1e-12).all()
        assert bool((signed < 0.99 * absolute).any()) == cancels


def test_status_words_and_limits_match_the_header():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'gadapt_mesh.h')).read()
    for macro, value in (('GADAPT_MA_CONVERGED', CONVERGED), ('GADAPT_MA_CAP', CAP), ('GADAPT_MA_NONCONVEX', NONCONVEX),
                         ('GADAPT_MA_DESC', _native_mesh.MA_DESC)):
        assert f'#define {macro}' in hdr and hdr.split(f'#define {macro}')[1].split()[0] == str(value), macro
    assert (CONVERGED, CAP, NONCONVEX) == (R.CONVERGED, R.CAP, R.NONCONVEX)
    assert '#define GADAPT_MESH_ABI 2' in hdr
    lib = _native_mesh.lib()                                          # loads without a GPU; resolves the new symbols
    assert lib.gadapt_ma_max_side() == 32 == _native_mesh.MA_MAX_SIDE and lib.gadapt_ma_max_gauss() == 8 == _native_mesh.MA_MAX_GAUSS
    assert lib.gadapt_ma_lds_bytes(1024) == 4 * (4 * 16 + 8 * 8 + 2 * 1024) and lib.gadapt_ma_lds_bytes(1025) == _native_mesh.E_SIZE


def test_a_stale_library_says_rebuild(monkeypatch):
    """A build from before these symbols has the same ABI number: NativeError with 'rebuild', not AttributeError."""
    monkeypatch.setattr(_native_mesh, '_lib', None)
    monkeypatch.setitem(_native_mesh.PROTOTYPES, 'gadapt_ma_not_built_yet', (_native_mesh._I, []))
    with pytest.raises(NativeError, match='rebuild'):
        _native_mesh.lib()


def test_host_entry_refuses_bad_sizes_before_any_launch():
    """gadapt_ma_batch checks the host copy of the descriptors first: these return their codes without touching a device."""
    import ctypes as C
    lib = _native_mesh.lib()
    one = C.c_void_p(8)                                               # never dereferenced: the checks come first

    def call(desc, cfl=0.2, tol=1e-4, max_steps=10):
        d = (C.c_int32 * len(desc))(*desc)
        return lib.gadapt_ma_batch(len(desc) // 4, C.cast(d, C.c_void_p), one, one, one, cfl, tol, max_steps, one, one, one, one, one, None)

    assert call([33, 0, 0, 1]) == _native_mesh.E_SIZE and b'N = 33' in lib.gadapt_mesh_last_error()
    assert call([11, 0, 0, 9]) == _native_mesh.E_SIZE
    assert call([11, 0, 0, 1], max_steps=_native_mesh.MAX_STEPS + 1) == _native_mesh.E_SIZE
    assert call([2, 0, 0, 1]) == -1 and call([11, -1, 0, 1]) == -1 and call([11, 0, 0, -1]) == -1
    assert call([11, 0, 0, 1], cfl=0.0) == -1 and call([11, 0, 0, 1], tol=float('nan')) == -1
    assert call([11, 0, 0, 1, 40, 121, 1, 1]) == _native_mesh.E_SIZE   # the second mesh of a batch is checked too


def test_argument_errors():
    p = dict(K.CASES['ds11'].params)
    nine = K.drawn(1, 9)
    with pytest.raises(ValueError, match='at least 3'):
        ma_batch([2], [p])
    with pytest.raises(ValueError, match='32'):
        ma_batch([33], [p])
    with pytest.raises(ValueError, match='square'):
        ma_batch([(8, 9)], [p])
    with pytest.raises(ValueError, match='at most 8'):
        ma_batch([11], [nine])
    with pytest.raises(ValueError, match='mon_reg'):
        ma_batch([11], [{'centers': p['centers'], 'scales': p['scales'], 'mon_power': 0.2}])
    with pytest.raises(ValueError, match='mon_reg'):
        monitor_ma(torch.zeros(3), torch.zeros(3), {'centers': [], 'scales': [], 'mon_power': 0.2})
    with pytest.raises(ValueError):
        ma_batch([11, 11], [p])
    with pytest.raises(ValueError):
        ma_batch([], [])
    with pytest.raises(ValueError):
        ma_batch([11], [p], max_steps=10 ** 9)
    with pytest.raises(ValueError):
        ma_batch([11], [p], cfl=0.0)
    with pytest.raises(ValueError):
        ma_batch([11], [p], tol=-1.0)
    with pytest.raises(ValueError, match='square'):
        MA2d(torch.zeros(72, 2), 8, p)
    with pytest.raises(ValueError, match='square'):
        deform_mesh_ma2d(torch.zeros(72, 2), 8, 9, p)
    with pytest.raises(TypeError):
        MA2d(torch.zeros(121, 2), 11, p, route='strided')
    with pytest.raises(ValueError, match='2-D only'):
        MeshDataset([21], 2, target='monge_ampere')


def test_target_names():
    with pytest.raises(ValueError, match='monge_ampere'):
        MeshDataset([11, 11], 2, target='ma')                         # the reference's short name stays refused, and says where to go


def test_native_error_without_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)    # where there is one, as where there is none
    p = K.CASES['ds11'].params
    with pytest.raises(NativeError, match='GPU'):
        MeshDataset([11, 11], 2, target='monge_ampere')
    with pytest.raises(NativeError, match='GPU'):
        MixedMeshDataset([9, 11], 2, target='monge_ampere')
    with pytest.raises(NativeError, match='GPU'):
        ma_batch([11], [p])
    with pytest.raises(NativeError, match='GPU'):
        MA2d(square_mesh(11).x_comp, 11, p)
