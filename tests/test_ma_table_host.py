"""CPU checks of the Monge-Ampere meshes from a tabulated monitor: what tests/test_gpu_ma_table.py relies on, proven on the fp64
restatement of the iteration (tests/ma_table_restatement.py) over the shared case table (tests/ma_table_cases.py), and the API
surface of `ma_table_batch`, `monitor_table`, `monitor_from_nodal`, `monitor_source` and the datasets' `uu` that needs no GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ma_cases as K  # noqa: E402
import ma_restatement as R  # noqa: E402
import ma_table_cases as TC  # noqa: E402
import ma_table_restatement as TR  # noqa: E402

from g_adaptivity_amd import (MeshDataset, MixedMeshDataset, _native_mesh, attach_ma_targets, ma_table_batch, monitor_from_nodal,  # noqa: E402
                              monitor_ma, monitor_table, square_mesh)
from g_adaptivity_amd._native import NativeError  # noqa: E402
from g_adaptivity_amd.monge_ampere import nodal_grid  # noqa: E402

EPS = 2.0 ** -52


def test_a_linear_table_gives_the_same_mesh_whatever_its_size():
    """1 + x + 2 y is reproduced exactly by the bilinear form for every T, so T = 2, 9 and 33 differ by fp64 rounding only.  The
    allowed difference follows from the run's own update count j: the interpolation is a handful of roundings, at most 8 eps
    relative on m, so at most 8 eps on r = log(m det) and 16 eps on r - rbar; an update adds dt = cfl / n1^2 times that to phi,
    j updates at most j times as much (the relaxation contracts differences, it does not amplify them), and
    x = xi + (phi_E - phi_W) n1 / 2 turns two such potentials into 16 j cfl eps / n1; one more eps for the last sum.
    Measured: 1.1e-16 against 2.1e-14 after 589 updates."""
    N = 11
    runs = [TR.ma(N, TC.linear(T), arith='fp64', cfl=TC.CFL, tol=TC.TOL) for T in (2, 9, 33)]
    j = runs[0][1]
    bound = 16 * j * TC.CFL * EPS / (N - 1) + EPS
    for run in runs:
        assert run[3] == TR.CONVERGED and run[1] == j and j > 100
    for run in runs[1:]:
        d = (run[0] - runs[0][0]).abs().max().item()
        print(f"linear table, {j} updates: {d:.3e} against {bound:.3e}")
        assert d <= bound
    assert (runs[0][0] - torch.stack(R.grid(N, torch.float64))).abs().max().item() > 0.05     # and it is not the grid


@pytest.mark.parametrize('arith', TR.ARITHMETICS)
def test_a_constant_table_is_the_grid(arith):
    xy, steps, res, status, *_ = TR.ma(11, TC.constant(5), arith=arith)
    want = torch.float64 if arith == 'fp64' else torch.float32
    assert steps == 0 and status == TR.CONVERGED and res <= 1e-6 and torch.equal(xy, torch.stack(R.grid(11, want)))


def test_finer_tables_converge_to_the_analytic_monitor():
    """ds11 (`ma_cases`), fp64 restatement to tol = 1e-4 with `monitor_table(params, T)` against `ma_restatement.ma` of the same
    params: max |z_T - z| = 6.796e-03, 2.056e-03, 2.470e-05 for T = 9, 33, 129 (445, 440, 445 updates; the analytic run 442)."""
    c = K.CASES['ds11']
    z = K.converged('ds11', 'fp64')[0]
    dist = []
    for T in (9, 33, 129):
        xy, _, _, status, *_ = TR.ma(c.N, monitor_table(c.params, T), arith='fp64', cfl=TC.CFL, tol=TC.TOL)
        assert status == TR.CONVERGED
        dist.append((xy - z).abs().max().item())
    print('T = 9, 33, 129: ' + ', '.join(f'{d:.3e}' for d in dist))
    assert dist[0] > dist[1] > dist[2]


@pytest.mark.parametrize('name', TC.CONVERGING)
def test_table_meshes_equidistribute_the_analytic_monitor(name):
    """T = 33 tables: the converged mesh's `cell_spread`, measured with the ANALYTIC monitor as everywhere else, is below the
    uniform grid's.  ds11: 0.0366 against 0.1247 (ratio 0.29; the analytic run reaches 0.0372); ds15: 0.0306 against 0.1874
    (0.16; analytic 0.0355)."""
    c = TC.case(name)
    assert c.T >= 33
    xy, steps, res, status, lmin, _ = TC.converged(name, 'fp64')
    before, after = R.uniform_spread(c.N, c.params), R.cell_spread(xy, c.params)
    print(f"{name}: {steps} updates, cell spread {before:.4f} -> {after:.4f} (ratio {after / before:.2f})")
    assert status == TR.CONVERGED and res <= TC.TOL and lmin > 0
    assert after < before
    assert R.triangles_keep_orientation(xy, square_mesh(c.N).cells)


@pytest.mark.parametrize('name', sorted(TC.CASES))
def test_fixed_step_cases_move_by_more_than_rounding_and_stay_convex(name):
    c = TC.case(name)
    xy, steps, _, status, lmin, _ = TC.fixed(name, 'fp64')
    assert steps == c.updates and status == TR.CAP and lmin > 0
    assert (xy - torch.stack(R.grid(c.N, torch.float64))).abs().max().item() >= 1000 * 2.0 ** -23
    assert 2 <= c.T <= 1024 and bool((c.table > 0).all()) and c.table.shape == (c.T, c.T)


def test_the_case_table_covers_what_it_has_to():
    lane = {TC.CASES[n].N for n, r in TC.FIXED if r == 'lane'}
    strided = {TC.CASES[n].N for n, r in TC.FIXED if r == 'strided'}
    assert {3, 8, 9, 11, 32} <= lane and {11, 32, 33, 81} <= strided
    assert {TC.slots(n) for n in strided} >= {1, 2, 7}
    ts = {(c.N, c.T) for c in TC.CASES.values()}
    assert any(t == 2 for _, t in ts) and any(n == t for n, t in ts) and (11, 17) in ts and any(t == 101 for _, t in ts)
    assert all(c.updates <= TC.UPDATES == 300 for c in TC.CASES.values() if c.N >= 32)


def test_the_restated_monitor_is_the_bilinear_form():
    """Exact at the lattice points, exact for a linear table anywhere, clamped outside the square, 0-indexed from a NaN."""
    M = TC.analytic(K.drawn(11, 2), 17)
    x, y = TC.lattice(17)
    assert torch.allclose(TR.table_monitor(x, y, M), M, rtol=4 * EPS, atol=0)
    p = torch.rand(50, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    want = 1.0 + p[:, 0] + 2.0 * p[:, 1]
    for T in (2, 9, 33):
        assert torch.allclose(TR.table_monitor(p[:, 0], p[:, 1], TC.linear(T)), want, rtol=16 * EPS, atol=0)
    out = torch.tensor([-0.5, 1.5, float('nan')], dtype=torch.float64)
    got = TR.table_monitor(out, torch.zeros(3, dtype=torch.float64), TC.linear(9))
    assert got.tolist() == [1.0, 2.0, 1.0]
    one = torch.ones(1, dtype=torch.float32)
    assert TR.table_monitor(one, one, TC.linear(9).float()).item() == 4.0          # x == 1 exactly: the last row and column


# ---------------------------------------------------------------------------------------------- monitor_table, monitor_from_nodal

def test_monitor_table_is_the_monitor_on_the_lattice():
    p = K.CASES['ds11'].params
    x, y = TC.lattice(9)
    assert torch.equal(monitor_table(p, 9), monitor_ma(x, y, p)) and monitor_table(p, 9).dtype == torch.float64
    assert monitor_table(p, 9)[2, 5] == monitor_ma(torch.tensor(0.25, dtype=torch.float64), torch.tensor(0.625, dtype=torch.float64), p)
    m2n = dict(p, mesh_type='M2N', fast_M2N_monitor='fast', mon_reg=0.1)
    t = monitor_table(m2n, 17)
    assert abs(t.max().item() - (0.1 + 1.5)) <= 1e-12 and t.min().item() >= 0.1   # its maximum over the lattice
    for T in (1, 1025):
        with pytest.raises(ValueError, match='2..1024'):
            monitor_table(p, T)


def test_monitor_from_nodal_is_exact_for_a_quadratic():
    """u = x^2 + 3 y^2: u_xx = 2, u_yy = 6 at every lattice point, the boundary rows and columns included.  A second difference
    of values up to 4 multiplied by (T-1)^2 carries at most 4 * 4 eps (T-1)^2 absolute error; the monitor's slope is below 1."""
    for T in (3, 5, 9, 33):
        x, y = TC.lattice(T)
        for reg, p in ((1.0, 0.2), (0.01, 0.2), (0.5, 1.0)):
            got = monitor_from_nodal(x * x + 3.0 * y * y, mon_reg=reg, mon_power=p)
            want = (reg + 40.0 ** 0.5) ** p
            assert got.shape == (T, T) and got.dtype == torch.float64
            assert (got - want).abs().max().item() <= 16 * EPS * (T - 1) ** 2 + 4 * EPS * want, (T, reg, p)


def test_monitor_from_nodal_is_local_and_scales_with_the_spacing():
    T = 9
    x, y = TC.lattice(T)
    u = torch.sin(3 * x) * torch.cos(2 * y)
    bump = u.clone()
    bump[4, 5] += 0.01
    changed = (monitor_from_nodal(bump) != monitor_from_nodal(u)).nonzero()
    assert len(changed) > 0 and all(abs(i - 4) <= 1 and abs(j - 5) <= 1 for i, j in changed.tolist())
    # the same nodal values on a lattice of half the spacing have four times the second differences: with mon_reg = 0 and
    # mon_power = 1 the monitor is their norm
    v5 = torch.rand(5, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    m5 = monitor_from_nodal(v5, mon_reg=0.0, mon_power=1.0)
    x5, y5 = TC.lattice(5)
    x9, y9 = TC.lattice(9)
    q = lambda a, b: a * a - 2.0 * a * b + 3.0 * b * b                  # noqa: E731
    m5q, m9q = monitor_from_nodal(q(x5, y5), mon_reg=0.0, mon_power=1.0), monitor_from_nodal(q(x9, y9), mon_reg=0.0, mon_power=1.0)
    assert torch.allclose(m5q, torch.full_like(m5q, 40.0 ** 0.5), rtol=1e-12) and torch.allclose(m9q, torch.full_like(m9q, 40.0 ** 0.5), rtol=1e-12)
    # and raw values: a 5 x 5 field read as T = 5 has (4 / 8)^2 the second differences of the same numbers spaced 1 / 8 apart
    pad = torch.zeros(9, 9, dtype=torch.float64)
    pad[:5, :5] = v5
    m9 = monitor_from_nodal(pad, mon_reg=0.0, mon_power=1.0)
    assert torch.allclose(m9[1:4, 1:4], 4.0 * m5[1:4, 1:4], rtol=1e-12)
    for bad in (torch.zeros(2, 2), torch.zeros(3, 4), torch.zeros(9), torch.zeros(3, 3, dtype=torch.int64)):
        with pytest.raises(ValueError, match='monitor_from_nodal'):
            monitor_from_nodal(bad)
    assert monitor_from_nodal(torch.zeros(4, 4, dtype=torch.float32)).dtype == torch.float32


# ---------------------------------------------------------------------------------------------- argument checks, no GPU call

def test_argument_errors_come_before_any_gpu_call(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)    # a GPU call would be a NativeError
    t = TC.linear(9)
    with pytest.raises(ValueError, match='at least 3'):
        ma_table_batch([2], [t])
    with pytest.raises(ValueError, match='32'):
        ma_table_batch([33], [t])
    with pytest.raises(ValueError, match='81'):
        ma_table_batch([82], [t], route='strided')
    with pytest.raises(ValueError, match='square'):
        ma_table_batch([(8, 9)], [t])
    with pytest.raises(ValueError, match='route'):
        ma_table_batch([11], [t], route='wide')
    with pytest.raises(ValueError, match='2..1024'):
        ma_table_batch([11], [torch.ones(1, 1)])
    with pytest.raises(ValueError, match='2..1024'):
        ma_table_batch([11], [torch.ones(1025, 1025)])
    for bad in (torch.ones(9, 8), torch.ones(81), torch.ones(9, 9, dtype=torch.int32), [[1.0, 1.0], [1.0, 1.0]]):
        with pytest.raises(ValueError, match='mesh 1: monitor table'):
            ma_table_batch([11, 11], [t, bad])
    with pytest.raises(ValueError, match='2 mesh sizes and 1 monitor tables'):
        ma_table_batch([11, 11], [t])
    with pytest.raises(ValueError):
        ma_table_batch([], [])
    with pytest.raises(ValueError, match='max_steps'):
        ma_table_batch([11], [t], max_steps=10 ** 9)
    with pytest.raises(ValueError, match='cfl'):
        ma_table_batch([11], [t], cfl=0.0)
    with pytest.raises(ValueError, match='cfl'):
        ma_table_batch([11], [t], tol=-1.0)
    with pytest.raises(NativeError, match='GPU'):                     # and a good call gets as far as the device
        ma_table_batch([11], [t])


def test_monitor_source_checks(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    ds = MeshDataset([11, 11], 2, seed=0)
    with pytest.raises(ValueError, match='M2N'):
        attach_ma_targets(ds.samples, {'monitor_source': 'uu', 'mesh_type': 'M2N', 'fast_M2N_monitor': 'fast', 'mon_reg': 0.1})
    with pytest.raises(ValueError, match='M2N'):
        MeshDataset([11, 11], 2, target='monge_ampere', target_params={'monitor_source': 'uu', 'mesh_type': 'M2N', 'mon_reg': 0.1})
    with pytest.raises(ValueError, match='monitor_source'):
        attach_ma_targets(ds.samples, {'monitor_source': 'fem'})
    with pytest.raises(ValueError, match='m2n_solve'):
        attach_ma_targets(ds.samples, {'monitor_source': 'uu'}, m2n_solve='p1')
    with pytest.raises(ValueError, match='mon_reg'):
        attach_ma_targets(ds.samples, {'monitor_source': 'uu', 'mon_power': 0.2})
    with pytest.raises(NativeError, match='GPU'):
        attach_ma_targets(ds.samples, {'monitor_source': 'uu', 'mon_reg': 0.1, 'mon_power': 0.2})
    with pytest.raises(NativeError, match='GPU'):
        MixedMeshDataset([9, 11], 2, target='monge_ampere', target_params={'monitor_source': 'uu'})
    with pytest.raises(NativeError, match='GPU'):                     # 'analytic' is the default path
        attach_ma_targets(ds.samples, {'monitor_source': 'analytic'})


def test_nodal_grid_reads_the_write_back_mapping_the_other_way():
    from g_adaptivity_amd.mmpde5 import unit_grid, write_back_to_nodes
    mesh = square_mesh(7)
    perm = torch.randperm(49, generator=torch.Generator().manual_seed(3))
    x_comp = mesh.x_comp[perm]                                        # any node order
    values = torch.arange(49, dtype=torch.float32)
    g = nodal_grid(x_comp, values, 7)
    gx, gy = unit_grid(7)
    back = write_back_to_nodes(x_comp, gx, gy, g, g)
    assert torch.equal(back[:, 0], values)
    assert torch.equal(nodal_grid(mesh.x_comp, values, 7), values.view(7, 7))


def _fields(ds):
    out = {}
    for k, d in enumerate(ds.samples):
        for key in d.keys():
            out[(k, key)] = getattr(d, key)
    return out


def _same_fields(a, b):
    fa, fb = _fields(a), _fields(b)
    assert fa.keys() == fb.keys() and len(fa) > 0
    for key, va in fa.items():
        vb = fb[key]
        if torch.is_tensor(va):
            assert torch.equal(va, vb) and va.dtype == vb.dtype, key
        elif isinstance(va, dict):
            assert va.keys() == vb.keys() and all(np.array_equal(np.asarray(va[k]), np.asarray(vb[k])) for k in va), key
        elif hasattr(va, 'coordinates'):
            assert (va.coordinates.cell_node_map().values == vb.coordinates.cell_node_map().values).all(), key
        else:
            assert (torch.as_tensor(va) == torch.as_tensor(vb)).all(), key


def test_the_datasets_defaults_are_unchanged(monkeypatch):
    _same_fields(MeshDataset([11, 11], 3, seed=4), MeshDataset([11, 11], 3, seed=4, uu='exact'))
    _same_fields(MeshDataset([21], 3, seed=4), MeshDataset([21], 3, seed=4, uu='exact', uu_params=None))
    _same_fields(MixedMeshDataset([9, 11], 4, seed=5), MixedMeshDataset([9, 11], 4, seed=5, uu='exact'))
    ds = MeshDataset([11, 11], 2, seed=4)
    assert all(torch.equal(d.uu_tensor, d.u_true_tensor) for d in ds.samples)
    with pytest.raises(ValueError, match='uu'):
        MeshDataset([11, 11], 2, uu='coarse')
    with pytest.raises(TypeError, match='uu_params'):
        MeshDataset([11, 11], 2, uu='fem', uu_params={'band': 'window'})
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(NativeError, match='GPU'):
        MeshDataset([11, 11], 2, uu='fem')
    with pytest.raises(NativeError, match='GPU'):
        MixedMeshDataset([9, 11], 2, uu='fem', uu_params={'fem_band': 'window'})


# ---------------------------------------------------------------------------------------------- header, library, ctypes

NEW = ('gadapt_ma_table_max_side', 'gadapt_ma_table_batch', 'gadapt_ma_table_batch_strided')


def test_header_and_ctypes_prototypes_agree_for_the_new_symbols():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'gadapt_mesh.h')).read()
    text = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    kinds = {'int': C.c_int, 'int64_t': C.c_int64, 'double': C.c_double}
    for name in NEW:
        ret, args = re.search(r'^\s*(int64_t|int)\s+' + name + r'\s*\(([^;{]*)\);', text, flags=re.M).groups()
        res, argtypes = _native_mesh.PROTOTYPES[name]
        want = [C.c_void_p if '*' in a else kinds[a.split()[0]] for a in (a.strip() for a in args.split(',')) if a not in ('', 'void')]
        assert res is kinds[ret] and argtypes == want, name
    # gadapt_ma_batch's list with `tables` in the place of `gauss` and without `mon`
    names = lambda n: [re.search(r'(\w+)\s*$', p).group(1) for p in re.search(r'\b' + n + r'\s*\(([^;{]*)\);', text).group(1).split(',')]  # noqa: E731
    base = names('gadapt_ma_batch')
    want = [('tables' if a == 'gauss' else a) for a in base if a != 'mon']
    assert names('gadapt_ma_table_batch') == want == names('gadapt_ma_table_batch_strided')
    for macro, value in (('GADAPT_MA_D_TABLE_OFF', 2), ('GADAPT_MA_D_TABLE_T', 3), ('GADAPT_MESH_ABI', _native_mesh.ABI_VERSION)):
        assert re.search(rf'#define {macro}\s+{value}\b', hdr), macro
    assert _native_mesh.ABI_VERSION == 2
    lib = _native_mesh.lib()                                          # loads without a GPU; resolves the new symbols
    assert lib.gadapt_ma_table_max_side() == 1024 == _native_mesh.MA_TABLE_MAX_SIDE


@pytest.mark.parametrize('entry, side', [('gadapt_ma_table_batch', 32), ('gadapt_ma_table_batch_strided', 81)])
def test_host_entries_refuse_bad_sizes_before_any_launch(entry, side):
    """Both entry points check the host copy of the descriptors first: these return their codes without touching a device."""
    lib = _native_mesh.lib()
    one = C.c_void_p(8)                                               # never dereferenced: the checks come first

    def call(desc, cfl=0.2, tol=1e-4, max_steps=10, tables=one):
        d = (C.c_int32 * len(desc))(*desc)
        return getattr(lib, entry)(len(desc) // 4, C.cast(d, C.c_void_p), one, tables, cfl, tol, max_steps, one, one, one, one, one, None)

    E = _native_mesh.E_SIZE
    assert call([side + 1, 0, 0, 9]) == E and f'N = {side + 1}'.encode() in lib.gadapt_mesh_last_error()
    assert call([11, 0, 0, 1]) == E and b'T = 1' in lib.gadapt_mesh_last_error()
    assert call([11, 0, 0, 1025]) == E and call([11, 0, 0, 0]) == E and call([11, 0, 0, -3]) == E
    assert call([11, 0, 0, 9], max_steps=_native_mesh.MAX_STEPS + 1) == E
    assert call([11, 0, 2 ** 31 - 50, 9]) == E                         # the table would end beyond 2^31 floats
    assert call([2, 0, 0, 9]) == -1 and call([11, -1, 0, 9]) == -1 and call([11, 0, -1, 9]) == -1
    assert call([11, 0, 0, 9], cfl=0.0) == -1 and call([11, 0, 0, 9], tol=float('nan')) == -1
    assert call([11, 0, 0, 9], tables=None) == -1
    assert call([11, 0, 0, 9, side + 1, 121, 81, 9]) == E              # the second mesh of a batch is checked too
    assert call([11, 0, 0, 9, 11, 121, 81, 1025]) == E
