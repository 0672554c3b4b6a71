"""CPU checks of the Monge-Ampere target meshes with the M2N 'slow' monitor: what tests/test_gpu_ma_m2n_slow.py relies on, proven
on the restatement of the iteration (tests/ma_m2n_slow_restatement.py) over the shared case table (tests/ma_m2n_slow_cases.py),
the restated P1 solve against an assembly written another way, and the API surface of g_adaptivity_amd.monge_ampere for
`fast_M2N_monitor = 'slow'` that needs no GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ma_cases as MC  # noqa: E402
import ma_m2n_slow_cases as K  # noqa: E402
import ma_m2n_slow_restatement as S  # noqa: E402

from g_adaptivity_amd import (MA2d, MASlowResult, MeshDataset, _native_mesh, deform_mesh_ma2d, ma_batch, monitor_m2n,  # noqa: E402
                              monitor_m2n_slow, square_mesh)
from g_adaptivity_amd._native import NativeError  # noqa: E402

NEW_SYMBOLS = ('gadapt_ma_m2n_slow_batch', 'gadapt_ma_m2n_slow_lds_bytes', 'gadapt_ma_m2n_slow_max_side')
P1 = {'m2n_solve': 'p1'}


def lds_bytes(N):
    return 4 * (6 * 16 + 8 * 8 + 4 + 6 * N * N + (N - 2) ** 2 * (N - 1) + (N - 2) ** 2)


def dense_p1_solution(x, y, u, f, N):
    """The P1 solution by the textbook route, in fp64 numpy, triangle by triangle: gradients of the hat functions from the
    inverse of [1 x y], stiffness area * grad.grad, mass area / 12 * (1 + delta), Dirichlet rows by elimination."""
    cells = square_mesh(N).cells.numpy()
    X = np.stack([x.reshape(-1).numpy(), y.reshape(-1).numpy()], 1).astype(np.float64)
    uf, ff = u.reshape(-1).numpy().astype(np.float64), f.reshape(-1).numpy().astype(np.float64)
    n = N * N
    Kd, Md = np.zeros((n, n)), np.zeros((n, n))
    for t in cells:
        G = np.linalg.inv(np.concatenate([np.ones((3, 1)), X[t]], 1))[1:, :]          # column k: grad of hat function k
        area = 0.5 * abs(np.linalg.det(np.concatenate([np.ones((3, 1)), X[t]], 1)))
        Kd[np.ix_(t, t)] += area * G.T @ G
        Md[np.ix_(t, t)] += area / 12.0 * (np.ones((3, 3)) + np.eye(3))
    i, j = np.meshgrid(np.arange(N), np.arange(N), indexing='ij')
    inner = ((i > 0) & (i < N - 1) & (j > 0) & (j < N - 1)).reshape(-1)
    c = uf.copy()
    c[inner] = np.linalg.solve(Kd[np.ix_(inner, inner)], (Md @ ff)[inner] - Kd[np.ix_(inner, ~inner)] @ uf[~inner])
    return torch.from_numpy(c.reshape(N, N))


def moved_nodes(N, seed=0):
    gx, gy = S.grid(N, torch.float64)
    gen = torch.Generator().manual_seed(seed)
    bump = lambda: 0.3 / (N - 1) * (torch.rand(N, N, generator=gen, dtype=torch.float64) - 0.5)  # noqa: E731
    return gx + bump(), gy + bump()


@pytest.mark.parametrize('N', [3, 4, 9, 12])
def test_restated_solve_against_an_independent_dense_assembly(N):
    x, y = moved_nodes(N, N)
    g = S.constants(dict(MC.drawn(N, 2), **K.RUN), torch.float64)[0]
    u, f, _ = S.fields(x, y, g)
    e = S.solve_error(x, y, u, f, N)
    want = dense_p1_solution(x, y, u, f, N) - u
    err = (e - want).abs().max().item()
    print(f"slow solve N={N}: |e| {want.abs().max().item():.3e}, restatement against the dense assembly {err:.3e}")
    assert want.abs().max().item() > 1e-4 and err <= 1e-11
    assert torch.equal(e[0], torch.zeros(N, dtype=torch.float64)) and torch.equal(e[:, -1], torch.zeros(N, dtype=torch.float64))


def test_nodal_error_of_the_solve_falls_by_about_four_per_halving():
    """P1 on the uniform grid is second order at the nodes: the largest nodal error falls by about 4 when N - 1 doubles."""
    g = S.constants({'centers': [[0.45, 0.55]], 'scales': [[0.3, 0.25]], 'mon_reg': 0.1}, torch.float64)[0]
    errs = []
    for N in (9, 17, 33):
        x, y = S.grid(N, torch.float64)
        u, f, _ = S.fields(x, y, g)
        errs.append(S.solve_error(x, y, u, f, N).abs().max().item())
    print('slow solve, nodal error at 9 / 17 / 33 a side:', ' '.join(f'{e:.3e}' for e in errs))
    assert 3.0 <= errs[0] / errs[1] <= 5.0 and 3.5 <= errs[1] / errs[2] <= 4.5


def test_monitor_m2n_slow_is_the_restated_monitor():
    for name in ('n11_g8', 'n11_g2', 'n9_g1', 'n3_g1'):
        c = K.CASES[name]
        x, y = moved_nodes(c.N, 7)
        g, reg, alpha, beta = S.constants(c.params, torch.float64)           # mon_reg and beta rounded to fp32 there: 6e-8
        got, want = monitor_m2n_slow(x, y, c.params), S.monitor(x, y, g, reg, alpha, beta)
        assert torch.allclose(got, want, rtol=1e-6, atol=0), name
        assert got.dtype == torch.float64 and got.min().item() >= c.params['mon_reg'] * (1 - 1e-6)
        assert got.max().item() <= c.params['mon_reg'] + c.params['M2N_alpha'] + c.params['M2N_beta'] + 1e-6
        fast = monitor_m2n(x, y, K.fast_params(c.params))
        assert torch.allclose(monitor_m2n_slow(x, y, dict(c.params, M2N_alpha=0.0)), fast, rtol=1e-12, atol=0)   # alpha = 0 is 'fast'
        assert (got - fast).abs().max().item() > 0.5                                                              # alpha = 1 is not
        assert monitor_m2n_slow(x.float(), y.float(), c.params).dtype == torch.float32
    flat = monitor_m2n_slow(*S.grid(11, torch.float64), dict(K.RUN, centers=[], scales=[]))
    assert torch.equal(flat, torch.full((11, 11), 0.1, dtype=torch.float64))
    with pytest.raises(ValueError, match='mon_reg'):
        monitor_m2n_slow(*S.grid(5, torch.float64), dict(MC.drawn(1, 1), **K.SLOW))
    with pytest.raises(ValueError, match=r'\[N, N\]'):
        monitor_m2n_slow(torch.zeros(9), torch.zeros(9), K.CASES['n3_g1'].params)


def test_header_states_the_new_entry_point():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'gadapt_mesh.h')).read()
    assert '#define GADAPT_MESH_ABI 2' in hdr
    for name in NEW_SYMBOLS:
        assert f'{name}(' in hdr and name in _native_mesh.PROTOTYPES, name
    for phrase in ("'slow' and 'superslow'", 'K_II c = b_I - K_IB u_B', 'Emax > 0', '(|D| / 24)', 'lower of quad (i-1, j)', 'mon3 [B, 3]',
                   'NONCONVEX', 'monitor_out [total nodes]'):
        assert phrase in hdr, phrase


def test_symbols_resolve_limit_and_lds_formula():
    lib = _native_mesh.lib()                                           # loads without a GPU
    assert lib.gadapt_mesh_abi_version() == 2 == _native_mesh.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    side = lib.gadapt_ma_m2n_slow_max_side()
    assert side == _native_mesh.MA_M2N_SLOW_MAX_SIDE == K.MAX_SIDE and side >= 23          # 23 is the reference's largest mesh
    for N in (3, 4, 11, 23, side):
        assert lib.gadapt_ma_m2n_slow_lds_bytes(N * N) == lds_bytes(N), N
    assert lib.gadapt_ma_m2n_slow_lds_bytes(side * side) < 65536 <= lds_bytes(side + 1)     # no raised limit, and none to spare
    for nodes in (8, 10, 120, (side + 1) ** 2):
        assert lib.gadapt_ma_m2n_slow_lds_bytes(nodes) == _native_mesh.E_SIZE, nodes
    assert lib.gadapt_ma_m2n_lds_bytes(121) == 4 * (5 * 16 + 8 * 8 + 4 + 2 * 121)            # the 'fast' layout is as before


def test_a_stale_library_says_rebuild(monkeypatch):
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
    with pytest.raises(NativeError, match='lacks gadapt_ma_m2n_slow.*rebuild'):
        _native_mesh.lib()


def test_host_entry_refuses_bad_descriptors_before_any_launch():
    lib = _native_mesh.lib()
    entry, side = 'gadapt_ma_m2n_slow_batch', K.MAX_SIDE
    one = C.c_void_p(8)                                                # never dereferenced: the checks come first

    def call(desc, cfl=0.2, tol=1e-4, max_steps=10, gauss=one, x=one, mon=one):
        d = (C.c_int32 * len(desc))(*desc)
        return lib.gadapt_ma_m2n_slow_batch(len(desc) // 4, C.cast(d, C.c_void_p), one, gauss, mon, cfl, tol, max_steps, x, one, one, one, one,
                                            None, None)

    assert call([side + 1, 0, 0, 1]) == _native_mesh.E_SIZE
    msg = lib.gadapt_mesh_last_error()
    assert f'N = {side + 1}'.encode() in msg and msg.startswith(entry.encode() + b':')
    assert call([32, 0, 0, 1]) == _native_mesh.E_SIZE                  # the lane route's limit is not this one's
    assert call([11, 0, 0, 9]) == _native_mesh.E_SIZE
    assert call([11, 0, 0, 1], max_steps=_native_mesh.MAX_STEPS + 1) == _native_mesh.E_SIZE
    assert call([2, 0, 0, 1]) == -1 and call([11, -1, 0, 1]) == -1 and call([11, 0, -1, 1]) == -1 and call([11, 0, 0, -1]) == -1
    assert call([11, 0, 0, 1], cfl=0.0) == -1 and call([11, 0, 0, 1], cfl=float('inf')) == -1
    assert call([11, 0, 0, 1], tol=float('nan')) == -1 and call([11, 0, 0, 1], tol=-1.0) == -1
    assert call([11, 0, 0, 1], gauss=None) == -1 and call([11, 0, 0, 1], x=None) == -1 and call([11, 0, 0, 1], mon=None) == -1
    assert call([11, 0, 0, 1, side + 8, 121, 1, 1]) == _native_mesh.E_SIZE   # the second mesh of a batch is checked too


def test_python_refusals_come_before_the_gpu_check(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)    # every refusal below is raised without a device
    g = {k: K.CASES['ds11'].params[k] for k in ('centers', 'scales')}
    ok = dict(g, **K.RUN)
    # unasked, 'slow' is refused as ever, and the message names the way in
    with pytest.raises(NotImplementedError, match=r"FEM.*m2n_solve='p1'"):
        ma_batch([11], [ok])
    with pytest.raises(NotImplementedError, match='FEM'):
        MA2d(square_mesh(11).x_comp, 11, ok)
    with pytest.raises(NotImplementedError, match='FEM'):
        MeshDataset([11, 11], 2, target='monge_ampere', target_params=K.RUN)
    for kw in ({}, P1):
        with pytest.raises(NotImplementedError, match='FEM'):
            ma_batch([11], [dict(ok, fast_M2N_monitor='superslow')], **kw)
    with pytest.raises(ValueError, match='m2n_solve'):
        ma_batch([11], [ok], m2n_solve='p2')
    # asked for
    with pytest.raises(ValueError, match="'lane' only"):
        ma_batch([11], [ok], route='strided', **P1)
    with pytest.raises(ValueError, match=f'{K.MAX_SIDE} a side'):
        ma_batch([K.MAX_SIDE + 1], [ok], **P1)
    with pytest.raises(ValueError, match='32'):
        ma_batch([33], [ok], **P1)
    with pytest.raises(ValueError, match='share one monitor'):
        ma_batch([11, 11], [ok, dict(ok, fast_M2N_monitor='fast')], **P1)
    with pytest.raises(ValueError, match='share one monitor'):
        ma_batch([11, 11], [dict(g, mon_reg=0.01, mon_power=0.2), ok], **P1)
    with pytest.raises(ValueError, match='mon_reg'):
        ma_batch([11], [dict(g, **K.SLOW)], **P1)
    for reg in (0.0, -0.1, float('nan')):
        with pytest.raises(ValueError, match='mon_reg'):
            ma_batch([11], [dict(ok, mon_reg=reg)], **P1)
    with pytest.raises(ValueError, match='M2N_alpha'):
        ma_batch([11], [dict(ok, M2N_alpha=-1.0)], **P1)
    with pytest.raises(ValueError, match='M2N_beta'):
        ma_batch([11], [dict(ok, M2N_beta=float('inf'))], **P1)
    with pytest.raises(ValueError, match='at most 8'):
        ma_batch([11], [dict(MC.drawn(1, 9), **K.RUN)], **P1)
    with pytest.raises(TypeError):
        MA2d(torch.zeros(121, 2), 11, ok, route='lane', **P1)          # MA2d keeps its keyword set, plus m2n_solve
    with pytest.raises(ValueError, match='square'):
        deform_mesh_ma2d(torch.zeros(72, 2), 8, 9, ok, **P1)
    with pytest.raises(ValueError, match="'lane' only"):
        MeshDataset([11, 11], 2, target='monge_ampere', target_params=dict(K.RUN, solver=dict(P1, route='strided')))
    # accepted: the defaults, alpha = 0, and 'fast' and 'ma', which ignore the keyword, get as far as the GPU check
    for p in (ok, {k: v for k, v in ok.items() if k not in ('M2N_alpha', 'M2N_beta')}, dict(ok, M2N_alpha=0.0, mon_power=0.2),
              dict(ok, fast_M2N_monitor='fast'), dict(g, mon_reg=0.01, mon_power=0.2)):
        with pytest.raises(NativeError, match='GPU'):
            ma_batch([11], [p], **P1)
    with pytest.raises(NativeError, match='GPU'):
        MA2d(square_mesh(11).x_comp, 11, ok, **P1)
    with pytest.raises(NativeError, match='GPU'):
        MeshDataset([11, 11], 2, target='monge_ampere', target_params=dict(K.RUN, solver=P1))
    assert MASlowResult._fields == ('coords', 'steps', 'residual', 'status', 'monitor')


@pytest.mark.parametrize('name', K.FIXED)
def test_fixed_cases_stay_convex_and_the_bar_cannot_hide_a_kernel_that_ignores_E(name):
    """Proved from the restatement alone.  Every fixed case stays convex in fp64 and in fp32; the nodes move by far more than
    rounding; and 4 x noise, the GPU bar, is at most one tenth of the distance between the 'slow' and the 'fast' fp64 meshes of
    the same Gaussians, mon_reg and beta after the same updates."""
    c = K.CASES[name]
    xy, steps, _, status, lmin, _ = K.fixed(name, 'fp64')
    assert steps == c.updates and status == S.CAP and lmin > 0
    assert K.fixed(name, 'fp32')[4] > 0 and K.fixed(name, 'fp32', True)[4] > 0
    assert (xy - torch.stack(S.grid(c.N, torch.float64))).abs().max().item() >= 1000 * 2.0 ** -23
    noise, gap = K.noise(name)[1], K.gap_to_fast(name)
    m64, mnoise = K.monitor_noise(name)
    print(f"slow {name} N={c.N}: noise {noise:.3e}, gap to 'fast' {gap:.3e}; monitor at 0 updates: fp32 from fp64 {mnoise:.3e}")
    assert 0 < noise
    assert 4 * noise <= 0.1 * gap
    assert 0 < mnoise < 1e-3 and bool(torch.isfinite(m64).all())


@pytest.mark.parametrize('name', K.CONVERGING + ['sym11'])
def test_converging_cases_reach_tol_with_orientation_kept(name):
    c = K.CASES[name]
    xy, j64, res, status, lmin, _ = K.converged(name, 'fp64')
    (_, j, _, st, lm, _), (_, jp, _, stp, lmp, _) = K.converged(name, 'fp32'), K.converged(name, 'fp32', True)
    noise, gap = K.noise(name, j64)[1], K.gap_to_fast(name, j64)
    print(f"slow {name}: stopping steps fp32 / fp32' / fp64 {j} / {jp} / {j64}, res {res:.3e}, min lambda {lmin:.3f}; noise at {j64}: "
          f"{noise:.3e}, gap to 'fast' {gap:.3e}")
    assert status == st == stp == S.CONVERGED and res <= K.TOL and 0 < j64 < 20000
    assert lmin > 0 and lm > 0 and lmp > 0
    assert abs(j - j64) <= 0.1 * j64 and abs(jp - j64) <= 0.1 * j64
    assert S.triangles_keep_orientation(xy, square_mesh(c.N).cells)
    assert 0 < noise < 1e-3 / (c.N - 1) and 4 * noise <= 0.1 * gap
    gx, gy = S.grid(c.N, torch.float64)
    assert torch.equal(xy[0][0], gx[0]) and torch.equal(xy[0][-1], gx[-1])
    assert torch.equal(xy[1][:, 0], gy[:, 0]) and torch.equal(xy[1][:, -1], gy[:, -1])
    if name == 'sym11':
        # the cut joins v1 and v3: the triangulation maps to itself under (i, j) -> (j, i) and under the point reflection, not
        # under a mirror in one direction, so E and the mesh have those two symmetries only
        x, y = xy
        # (the grid's xi_i are fp32 quotients, 1 - xi_i is not xi_{N-1-i} to 6e-8: the point reflection holds to that, amplified)
        assert (x - y.t()).abs().max().item() <= 1e-12 and (x - (1 - x.flip(0).flip(1))).abs().max().item() <= 1e-6
        assert (x - (1 - x.flip(0))).abs().max().item() > 1e-3


@pytest.mark.parametrize('arith', ['fp32', 'fp64'])
def test_the_nonconvex_case_loses_convexity_at_the_first_update(arith):
    c = K.CASES['nonconvex15']
    _, steps, _, status, lmin, *_ = S.ma(c.N, c.params, arith=arith, cfl=K.NONCONVEX_CFL)
    assert status == S.NONCONVEX and steps == 1 and lmin < -0.5
    _, steps, res, status, lmin, *_ = S.ma(c.N, c.params, arith=arith, cfl=0.05, max_steps=5)     # "lower cfl"
    assert status == S.CAP and steps == 5 and lmin > 0 and res > K.TOL


def test_five_steps_reach_the_cap_and_a_constant_monitor_is_the_grid():
    c = K.CASES['ds11']
    _, steps, res, status, *_ = S.ma(c.N, c.params, arith='fp32', max_steps=5)
    assert status == S.CAP and steps == 5 and res > K.TOL
    xy, steps, _, status, *_ = S.ma(11, dict(K.RUN, centers=[], scales=[]), arith='fp32')
    assert steps == 0 and status == S.CONVERGED and torch.equal(xy, torch.stack(S.grid(11, torch.float32)))
