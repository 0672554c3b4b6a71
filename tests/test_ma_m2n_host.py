"""CPU checks of the Monge-Ampere target meshes with the M2N 'fast' monitor: what tests/test_gpu_ma_m2n.py relies on, proven on the
fp64 restatement of the iteration (tests/ma_m2n_restatement.py) over the shared case table (tests/ma_m2n_cases.py), and the API
surface of g_adaptivity_amd.monge_ampere for `mesh_type = 'M2N'` that needs no GPU."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ma_cases as MC  # noqa: E402
import ma_m2n_cases as K  # noqa: E402
import ma_m2n_restatement as M  # noqa: E402

from g_adaptivity_amd import (MA2d, MeshDataset, MixedMeshDataset, _native_mesh, deform_mesh_ma2d, ma_batch, monitor_m2n,  # noqa: E402
                              square_mesh)
from g_adaptivity_amd._native import NativeError  # noqa: E402

NEW_SYMBOLS = ('gadapt_ma_m2n_batch', 'gadapt_ma_m2n_batch_strided', 'gadapt_ma_m2n_lds_bytes', 'gadapt_ma_m2n_strided_lds_bytes')


@pytest.mark.parametrize('name', K.CONVERGING + ['sym11'])
def test_fp64_restatement_converges_convex_untangled_and_equidistributes(name):
    c = K.CASES[name]
    xy, steps, res, status, lmin = K.converged(name, 'fp64')
    before, after = M.uniform_spread(c.N, c.params), M.cell_spread(xy, c.params)
    print(f"m2n {name}: {steps} updates, res {res:.3e}, min lambda {lmin:.3f}, cell spread {before:.4f} -> {after:.4f}")
    assert status == M.CONVERGED and res <= K.TOL and 0 < steps < 20000
    assert lmin > 0                                                    # at every evaluation on the way
    assert M.triangles_keep_orientation(xy, square_mesh(c.N).cells)
    assert after <= 0.5 * before                                       # (mon_reg, beta) = (0.1, 1.5) in all three
    gx, gy = M.grid(c.N, torch.float64)
    assert torch.equal(xy[0][0], gx[0]) and torch.equal(xy[0][-1], gx[-1])
    assert torch.equal(xy[1][:, 0], gy[:, 0]) and torch.equal(xy[1][:, -1], gy[:, -1])


@pytest.mark.parametrize('name', K.CONVERGING)
def test_fp32_and_mixed_restatements_are_quiet(name):
    """The stopping steps of the two routes' arithmetic, plain and perturbed, recorded and near the fp64 step (the issue's
    survey saw gaps of about 1 %, 7 % at most); the noise at the fp64 step is finite and far below a cell."""
    c = K.CASES[name]
    j64 = K.converged(name, 'fp64')[1]
    for route, arith in K.ARITH_OF_ROUTE.items():
        (_, j, _, st, lm), (_, jp, _, stp, lmp) = K.converged(name, arith), K.converged(name, arith, True)
        _, noise = K.noise(name, route, j64)
        print(f"m2n {name} {route}: stopping steps {arith} / {arith}' / fp64 {j} / {jp} / {j64}; noise at {j64}: {noise:.3e}")
        assert st == stp == M.CONVERGED and lm > 0 and lmp > 0
        assert abs(j - j64) <= 0.1 * j64 and abs(jp - j64) <= 0.1 * j64
        assert 0 < noise < 1e-3 / (c.N - 1)


@pytest.mark.parametrize('name', K.FIXED + K.FIXED_STRIDED)
def test_fixed_step_cases_stay_convex_and_move_by_more_than_rounding(name):
    """A comparison after a fixed number of updates means something only if the nodes moved: by at least 1 000 spacings of
    fp32 at 1.0 in the fp64 restatement.  The noise of each route that runs the case is finite."""
    c = K.CASES[name]
    xy, steps, _, status, lmin = K.fixed(name, 'fp64')
    assert steps == c.updates and status == M.CAP and lmin > 0
    assert (xy - torch.stack(M.grid(c.N, torch.float64))).abs().max().item() >= 1000 * 2.0 ** -23
    for route in (('lane', 'strided') if c.N <= 32 else ('strided',)):
        noise = K.noise(name, route)[1]
        print(f"m2n {name} N={c.N} {route}: noise {noise:.3e}")
        assert 0 < noise < 1e-5


@pytest.mark.parametrize('arith', ['fp32', 'fp64', 'mixed'])
def test_the_nonconvex_case_loses_convexity_at_the_first_update(arith):
    c = K.CASES['nonconvex15']
    _, steps, _, status, lmin = M.ma(c.N, c.params, arith=arith, cfl=K.CFL)
    assert status == M.NONCONVEX and steps == 1 and lmin < -0.1
    _, steps, res, status, lmin = M.ma(c.N, c.params, arith=arith, cfl=0.05, max_steps=5)      # "lower cfl"
    assert status == M.CAP and steps == 5 and lmin > 0 and res > K.TOL


def test_five_steps_reach_the_cap_and_a_constant_monitor_is_the_grid():
    c = K.CASES['ds11']
    _, steps, res, status, _ = M.ma(c.N, c.params, arith='fp32', max_steps=5)
    assert status == M.CAP and steps == 5 and res > K.TOL
    for arith in ('fp32', 'mixed'):
        xy, steps, _, status, _ = M.ma(11, dict(K.RUN, centers=[], scales=[]), arith=arith)
        assert steps == 0 and status == M.CONVERGED and torch.equal(xy, torch.stack(M.grid(11, torch.float32)))


def test_monitor_m2n_is_the_restated_monitor_with_the_last_gaussians_uxy():
    gx, gy = M.grid(33, torch.float64)
    for name in ('n11_g8', 'n11_g2', 'n9_g1'):
        p = K.CASES[name].params
        g, reg, beta = M.constants(p, torch.float64)                   # mon_reg and beta rounded to fp32 there: 6e-8
        got = monitor_m2n(gx, gy, p)
        assert torch.allclose(got, M.monitor(gx, gy, g, reg, beta), rtol=1e-6, atol=0)
        assert abs(got.max().item() - (p['mon_reg'] + p['M2N_beta'])) < 1e-6 and got.min().item() >= p['mon_reg']
        # the reference's `=`: with one Gaussian nothing differs from a summed u_xy, with more the earlier ones' u_xy are dropped
        Fs = M.hessian_norm(gx, gy, g, last_only=False)
        summed = M.normalised(Fs, Fs.max(), reg, beta)
        assert bool(((got - summed).abs() > 1e-3).any()) == (len(p['centers']) > 1), name
    two = K.CASES['n11_g2'].params
    swapped = dict(two, centers=two['centers'][::-1], scales=two['scales'][::-1])
    assert (monitor_m2n(gx, gy, two) - monitor_m2n(gx, gy, swapped)).abs().max().item() > 1e-3   # the order of the Gaussians matters
    flat = monitor_m2n(gx, gy, dict(K.RUN, centers=[], scales=[]))
    assert torch.equal(flat, torch.full_like(gx, 0.1))
    assert 'mon_power' not in K.RUN
    assert torch.equal(monitor_m2n(gx, gy, dict(two, mon_power=0.3, M2N_alpha=2.0)), monitor_m2n(gx, gy, two))   # read by neither


def test_header_states_the_new_entry_points():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'gadapt_mesh.h')).read()
    assert '#define GADAPT_MESH_ABI 2' in hdr
    for name in NEW_SYMBOLS:
        assert f'{name}(' in hdr and name in _native_mesh.PROTOTYPES, name
    for phrase in ('LAST Gaussian', 'Fmax > 0', 'no powf', "'slow' and 'superslow'"):
        assert phrase in hdr, phrase


def test_symbols_resolve_and_lds_formulas():
    lib = _native_mesh.lib()                                           # loads without a GPU
    assert lib.gadapt_mesh_abi_version() == 2 == _native_mesh.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    for nodes in (9, 121, 1024):
        assert lib.gadapt_ma_m2n_lds_bytes(nodes) == 4 * (5 * 16 + 8 * 8 + 4 + 2 * nodes)      # the 4 floats hold Cxy
        assert lib.gadapt_ma_lds_bytes(nodes) == 4 * (4 * 16 + 8 * 8 + 2 * nodes)              # as before
    for nodes in (9, 1089, 6561):
        assert lib.gadapt_ma_m2n_strided_lds_bytes(nodes) == 592 + 8 * nodes
        assert lib.gadapt_ma_strided_lds_bytes(nodes) == 512 + 8 * nodes                       # as before
    assert lib.gadapt_ma_m2n_strided_lds_bytes(6561) < 64 * 1024
    assert lib.gadapt_ma_m2n_lds_bytes(1025) == lib.gadapt_ma_m2n_lds_bytes(8) == _native_mesh.E_SIZE
    assert lib.gadapt_ma_m2n_strided_lds_bytes(6562) == lib.gadapt_ma_m2n_strided_lds_bytes(8) == _native_mesh.E_SIZE


def test_a_stale_library_says_rebuild(monkeypatch):
    """A build from before these symbols has the same ABI number: NativeError with 'rebuild', not AttributeError."""
    real = C.CDLL

    class Stale:
        def __init__(self, path):
            self._h = real(path)

        def __getattr__(self, name):
            if name in NEW_SYMBOLS:
                raise AttributeError(name)
            return getattr(self._h, name)

    monkeypatch.setattr(_native_mesh, '_lib', None)
    monkeypatch.setattr(_native_mesh.C, 'CDLL', Stale)
    with pytest.raises(NativeError, match='lacks gadapt_ma_m2n.*rebuild'):
        _native_mesh.lib()


@pytest.mark.parametrize('entry, side', [('gadapt_ma_m2n_batch', 32), ('gadapt_ma_m2n_batch_strided', 81)])
def test_host_entries_refuse_bad_descriptors_before_any_launch(entry, side):
    """Both entry points check the host copy of the descriptors first: these return their codes without touching a device."""
    lib = _native_mesh.lib()
    one = C.c_void_p(8)                                                # never dereferenced: the checks come first

    def call(desc, cfl=0.2, tol=1e-4, max_steps=10, gauss=one, x=one):
        d = (C.c_int32 * len(desc))(*desc)
        return getattr(lib, entry)(len(desc) // 4, C.cast(d, C.c_void_p), one, gauss, one, cfl, tol, max_steps, x, one, one, one, one, None)

    assert call([side + 1, 0, 0, 1]) == _native_mesh.E_SIZE
    msg = lib.gadapt_mesh_last_error()
    assert f'N = {side + 1}'.encode() in msg and msg.startswith(entry.encode() + b':')
    assert call([11, 0, 0, 9]) == _native_mesh.E_SIZE
    assert call([11, 0, 0, 1], max_steps=_native_mesh.MAX_STEPS + 1) == _native_mesh.E_SIZE
    assert call([2, 0, 0, 1]) == -1 and call([11, -1, 0, 1]) == -1 and call([11, 0, -1, 1]) == -1 and call([11, 0, 0, -1]) == -1
    assert call([11, 0, 0, 1], cfl=0.0) == -1 and call([11, 0, 0, 1], cfl=float('inf')) == -1
    assert call([11, 0, 0, 1], tol=float('nan')) == -1 and call([11, 0, 0, 1], tol=-1.0) == -1
    assert call([11, 0, 0, 1], gauss=None) == -1 and call([11, 0, 0, 1], x=None) == -1
    assert call([11, 0, 0, 1, side + 8, 121, 1, 1]) == _native_mesh.E_SIZE   # the second mesh of a batch is checked too


def test_python_refusals_come_before_the_gpu_check(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)    # every refusal below is raised without a device
    g = {k: K.CASES['ds11'].params[k] for k in ('centers', 'scales')}
    ok = dict(g, **K.RUN)
    with pytest.raises(ValueError, match='mesh_type'):
        ma_batch([11], [dict(ok, mesh_type='m2n')])
    with pytest.raises(ValueError, match='Please specify fast_M2N_monitor in params'):
        ma_batch([11], [dict(g, mesh_type='M2N', mon_reg=0.1)])
    with pytest.raises(ValueError, match='Please specify fast_M2N_monitor in params'):
        ma_batch([11], [dict(ok, fast_M2N_monitor='quick')])
    for slow in ('slow', 'superslow'):
        with pytest.raises(NotImplementedError, match='FEM'):
            ma_batch([11], [dict(ok, fast_M2N_monitor=slow)])
        with pytest.raises(NotImplementedError, match='FEM'):
            MA2d(square_mesh(11).x_comp, 11, dict(ok, fast_M2N_monitor=slow))
    with pytest.raises(ValueError, match='mon_reg'):
        ma_batch([11], [dict(g, **K.M2N)])
    for reg in (0.0, -0.1, float('nan')):
        with pytest.raises(ValueError, match='mon_reg'):
            ma_batch([11], [dict(ok, mon_reg=reg)])
    with pytest.raises(ValueError, match='M2N_beta'):
        ma_batch([11], [dict(ok, M2N_beta=-1.0)])
    with pytest.raises(ValueError, match='mon_reg'):
        monitor_m2n(torch.zeros(3), torch.zeros(3), dict(g, **K.M2N))
    with pytest.raises(ValueError, match='share one monitor'):
        ma_batch([11, 11], [ok, dict(g, mon_reg=0.01, mon_power=0.2)])
    with pytest.raises(ValueError, match='share one monitor'):
        ma_batch([11, 11], [dict(g, mesh_type='ma'), ok], route='strided')
    # the refusals that stay, with the M2N monitor as without it
    with pytest.raises(ValueError, match='32'):
        ma_batch([33], [ok])
    with pytest.raises(ValueError, match='81'):
        ma_batch([82], [ok], route='strided')
    with pytest.raises(ValueError, match='at most 8'):
        ma_batch([11], [dict(MC.drawn(1, 9), **K.RUN)])
    with pytest.raises(ValueError, match='2-D only'):
        MeshDataset([21], 2, target='monge_ampere', target_params=K.RUN)
    with pytest.raises(ValueError, match='monge_ampere'):
        MeshDataset([11, 11], 2, target='ma', target_params=K.RUN)
    with pytest.raises(TypeError):
        MA2d(torch.zeros(121, 2), 11, ok, route='strided')             # MA2d keeps its keyword set
    with pytest.raises(ValueError, match='square'):
        deform_mesh_ma2d(torch.zeros(72, 2), 8, 9, ok)
    # accepted and ignored keys, and the defaults, get as far as the GPU check
    for p in (ok, dict(ok, mon_power=0.2, M2N_alpha=1.0), {k: v for k, v in ok.items() if k != 'M2N_beta'}, dict(ok, M2N_beta=0.0)):
        with pytest.raises(NativeError, match='GPU'):
            ma_batch([11], [p])


def test_native_error_without_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)    # where there is one, as where there is none
    p = K.CASES['ds11'].params
    with pytest.raises(NativeError, match='GPU'):
        MeshDataset([11, 11], 2, target='monge_ampere', target_params=K.RUN)
    with pytest.raises(NativeError, match='GPU'):
        MixedMeshDataset([9, 11], 2, target='monge_ampere', target_params=K.RUN)
    with pytest.raises(NativeError, match='GPU'):
        ma_batch([11], [p], route='strided')
    with pytest.raises(NativeError, match='GPU'):
        MA2d(square_mesh(11).x_comp, 11, p)
