"""CPU checks of the MMPDE5 generator: the test-side restatement against the golden data recorded from the reference
(tools/make_mmpde5_golden.py) and against properties of the continuous problem, the monitor functions, and the API surface of
g_adaptivity_amd.mmpde5 that needs no GPU."""
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mmpde5_restatement as R  # noqa: E402

from g_adaptivity_amd import MeshDataset, MixedMeshDataset, _native_mesh, mmpde5_batch, monitor_1d, monitor_2d  # noqa: E402
from g_adaptivity_amd.mmpde5 import monitor_arrays_1d, monitor_arrays_2d  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mmpde5')
CASES = sorted(os.path.basename(f)[:-len('.npz')] for f in glob.glob(os.path.join(GOLDEN, '*.npz')))


def load(name):
    g = np.load(os.path.join(GOLDEN, f'{name}.npz'))
    two = int(g['dim']) == 2
    z0 = torch.stack([torch.tensor(g['x0']), torch.tensor(g['y0'])]) if two else torch.tensor(g['x0'])
    z = torch.stack([torch.tensor(g['x']), torch.tensor(g['y'])]) if two else torch.tensor(g['x'])
    params = {k[len('param_'):]: (g[k].tolist() if g[k].ndim else float(g[k])) for k in g.files if k.startswith('param_')}
    return g, z0, z, torch.tensor(g['ms']), torch.tensor(g['m2']), params


def test_all_golden_cases_present():
    assert CASES == ['1d_n21_power_only', '1d_n21_reg0p01', '1d_n21_reg0p1', '2d_n11', '2d_n15', 'burgers_n17']


@pytest.mark.parametrize('name', CASES)
def test_fp32_restatement_reproduces_the_reference(name):
    g, z0, z, ms, m2, _ = load(name)
    out, j, measure = R.mmpde5(z0, ms, m2)
    assert j == int(g['j']) and j < 10000 and measure <= 1e-6
    # the same operations in the same order: to fp32 rounding (a few ulp of coordinates <= 1)
    assert (out - z).abs().max().item() <= 4 * 2.0 ** -24


@pytest.mark.parametrize('name', [c for c in CASES if not c.startswith('burgers')])
def test_monitor_against_the_reference_arrays(name):
    g, _, _, ms, m2, params = load(name)
    n = int(g['n'])
    if int(g['dim']) == 1:
        got = monitor_arrays_1d(lambda t: monitor_1d(t, params), n)
    else:
        got = monitor_arrays_2d(lambda a, b: monitor_2d(a, b, params), n)
    # same formula, another association of the polynomial factor: fp32 rounding of values of order 1
    assert torch.allclose(got[0], ms, rtol=2e-5, atol=0) and torch.allclose(got[1], m2, rtol=2e-5, atol=0)


def test_monitor_quirks():
    xi = torch.linspace(0, 1, 41, dtype=torch.float64)
    p = {'centers': [[0.5]], 'scales': [[0.1]]}
    dflt = monitor_1d(xi, p)
    assert torch.allclose(dflt, monitor_1d(xi, dict(p, mon_power=0.2))) and dflt.max().item() == pytest.approx(2 ** 0.2)
    assert torch.allclose(monitor_1d(xi, dict(p, mon_reg=0.1)), dflt)                   # mon_reg alone is not read
    assert monitor_1d(xi, dict(p, mon_reg=0.1, mon_power=0.5)).min().item() == pytest.approx(0.1 ** 0.5, rel=1e-6)
    # normalised by the maximum of the grid of the call: a grid that misses the peak still reaches 1
    assert monitor_1d(torch.linspace(0, 0.3, 7, dtype=torch.float64), p).max().item() == pytest.approx(2 ** 0.2)
    x, y = torch.meshgrid(xi, xi, indexing='ij')
    p2 = {'centers': [[0.3, 0.6]], 'scales': [[0.2, 0.25]]}
    assert torch.equal(monitor_2d(x, y, dict(p2, mon_reg=5.0)), monitor_2d(x, y, p2))   # mon_reg is ignored in 2-D
    assert monitor_2d(x, y, p2).min().item() >= 1.0


def test_fp64_boundary_fixed_and_constant_monitor_is_a_fixed_point():
    g, z0, _, ms, m2, _ = load('2d_n11')
    out, j, _ = R.mmpde5(z0, ms, m2, dtype=torch.float64, max_steps=300)
    for k in range(2):
        assert torch.equal(out[k][0], z0[k][0].double()) and torch.equal(out[k][-1], z0[k][-1].double())
        assert torch.equal(out[k][:, 0], z0[k][:, 0].double()) and torch.equal(out[k][:, -1], z0[k][:, -1].double())
    assert (out - z0.double()).abs().max().item() > 1e-3                                   # and the interior did move
    lin = torch.linspace(0, 1, 11, dtype=torch.float64)                                   # uniform in fp64, not a rounded fp32 grid
    u0 = torch.stack(torch.meshgrid(lin, lin, indexing='ij'))
    flat, j, measure = R.mmpde5(u0, torch.full_like(ms, 1.7), torch.full_like(m2, 1.7), dtype=torch.float64, max_steps=50)
    assert (flat - u0).abs().max().item() <= 1e-12 and j == 1                             # nothing to do: one step, below tol
    x1 = torch.linspace(0, 1, 21, dtype=torch.float64)
    line, j, _ = R.mmpde5(x1, torch.ones(20), torch.ones(21), dtype=torch.float64, max_steps=50)
    assert (line - x1).abs().max().item() <= 1e-12 and j == 1


@pytest.mark.parametrize('name', ['1d_n21_reg0p1', '1d_n21_reg0p01', 'burgers_n17'])
def test_fp64_equidistribution_1d(name):
    """At the stationary state ms[i] (X[i+1] - X[i]) is the same in every cell.  The loop stops when one step moves the nodes
    by tol = 1e-6 in all; a step is h * rhs and rhs = (flux difference) / dxi^2 / tau / m2, so the flux differences left
    are bounded by tol * dxi^2 * tau * max(m2) / h summed over the nodes, and the flux range over N - 1 cells by that sum."""
    g, z0, _, ms, m2, _ = load(name)
    n = int(g['n'])
    out, j, measure = R.mmpde5(z0, ms, m2, dtype=torch.float64)
    assert measure <= 1e-6 and j < 10000
    flux = ms.double() * (out[1:] - out[:-1])
    h, dxi = 0.05 / n ** 3, 1.0 / (n - 1)
    bound = 1e-6 * dxi ** 2 * 0.1 * m2.max().item() / h
    assert (flux.max() - flux.min()).item() <= bound
    assert (flux.max() - flux.min()).item() <= 0.05 * flux.mean().item()                   # equidistributed to a few per cent


def test_header_symbols_match_prototypes():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'gadapt_mesh.h')).read()
    body = hdr[hdr.index('#define GADAPT_MESH_ABI'):]
    decls = re.findall(r'^\s*(int64_t|int|const char\*)\s+(gadapt_\w+)\s*\(([^;]*)\);', body, flags=re.M | re.S)
    assert {name for _, name, _ in decls} == set(_native_mesh.PROTOTYPES)
    assert f"#define GADAPT_MESH_ABI {_native_mesh.ABI_VERSION}" in hdr
    import ctypes as C
    kinds = {'int': C.c_int, 'int64_t': C.c_int64, 'double': C.c_double, 'float': C.c_float}
    for ret, name, args in decls:
        res, argtypes = _native_mesh.PROTOTYPES[name]
        assert res is {'int': C.c_int, 'int64_t': C.c_int64, 'const char*': C.c_char_p}[ret], name
        want = []
        for a in [a.strip() for a in args.split(',') if a.strip() not in ('', 'void')]:
            want.append(C.c_void_p if '*' in a else kinds[a.split()[0]])
        assert argtypes == want, name
    for macro, value in (('GADAPT_MMPDE5_MAX_NODES', _native_mesh.MAX_NODES), ('GADAPT_MMPDE5_MAX_STEPS', _native_mesh.MAX_STEPS),
                         ('GADAPT_MMPDE5_DESC', _native_mesh.DESC), ('GADAPT_MESH_E_SIZE', _native_mesh.E_SIZE),
                         ('GADAPT_MMPDE5_CONVERGED', _native_mesh.CONVERGED), ('GADAPT_MMPDE5_CAP', _native_mesh.CAP),
                         ('GADAPT_MMPDE5_STIFF', _native_mesh.STIFF)):
        assert re.search(rf'#define {macro}\s+{value}\b', hdr), macro


def test_value_errors_beyond_the_limits():
    ones = torch.ones
    with pytest.raises(ValueError, match='1024'):
        mmpde5_batch([torch.linspace(0, 1, 1025)], [(ones(1024), ones(1025))])
    with pytest.raises(ValueError, match='1024'):
        mmpde5_batch([torch.zeros(2, 33, 33)], [(ones(32, 32), ones(33, 33))])
    with pytest.raises(ValueError):
        mmpde5_batch([torch.zeros(2, 8, 9)], [(ones(7, 8), ones(8, 9))])                  # square grids only
    with pytest.raises(ValueError):
        mmpde5_batch([torch.linspace(0, 1, 21)], [(ones(21), ones(21))])                  # ms has N - 1 entries
    with pytest.raises(ValueError):
        mmpde5_batch([torch.linspace(0, 1, 21)], [(ones(20), ones(21))], max_steps=10 ** 9)
    with pytest.raises(ValueError):
        mmpde5_batch([torch.linspace(0, 1, 21)], [(ones(20), ones(21))], tol=-1.0)
    with pytest.raises(ValueError):
        mmpde5_batch([], [])
    with pytest.raises(ValueError):
        MeshDataset([11, 11], 2, target='ma')


# sha256 over the node fields of the default datasets, recorded from the commit before `target=` existed (fixed seeds)
def _digest(ds):
    import hashlib
    h = hashlib.sha256()
    for s in ds.samples:
        for k in ('x_comp', 'x_phys', 'f_tensor', 'uu_tensor', 'u_true_tensor'):
            h.update(getattr(s, k).numpy().tobytes())
    return h.hexdigest()


RECORDED = {
    'square': 'a123892b6cb5dd51b2b0c877cdae1f8910ec3612899c1461669cf100ec90379f',
    'interval': 'ce3773a7898312f012ada168ea9e20a434ffce94f679b05f20ab7fbc7e2224f4',
    'mixed': '794e55aaac4316ee50b5b09f2c418a4067a4732eb61f7c4fd6945f91366fac9a',
}


@pytest.mark.parametrize('kind', ['square', 'interval', 'mixed'])
def test_noise_targets_are_unchanged(kind):
    make = {'square': lambda **k: MeshDataset([11, 11], 3, seed=5, **k), 'interval': lambda **k: MeshDataset([21], 4, seed=7, **k),
            'mixed': lambda **k: MixedMeshDataset([9, 11], 4, seed=2, **k)}[kind]
    assert _digest(make()) == RECORDED[kind]                 # the default is today's data, bit for bit
    assert _digest(make(target='noise')) == RECORDED[kind]
    assert not hasattr(make().samples[0], 'ma_its')


# ---------------------------------------------------------------- the wave and workgroup edges of test_gpu_mmpde5.py
EDGE_1D = (3, 4, 63, 64, 65, 128, 129, 1023, 1024)        # 1 wave, 1 / 2 / 3 waves with the last nearly empty, 16 waves
EDGE_2D = (3, 7, 8, 9, 16, 17, 31, 32)                    # 9, 49, 64, 81, 256, 289, 961, 1024 nodes
EDGE_STEPS = 50


def edge_case(dim, N):
    """Uniform start and a random constant monitor (1 + rand at the cells, constant at the nodes), as
    test_alone_and_in_a_mixed_batch_bit_identical builds them.  The RK4 step is the default cfl / N^3 at every size."""
    g = torch.Generator().manual_seed(10 * N + dim)
    lin = torch.linspace(0, 1, N)
    if dim == 1:
        return lin, (1 + torch.rand(N - 1, generator=g), torch.ones(N))
    return torch.stack(torch.meshgrid(lin, lin, indexing='ij')), (1 + torch.rand(N - 1, N - 1, generator=g), torch.ones(N, N) * 1.5)


_edge = {}


def edge_restated(dim, N, dtype):
    """(Z, measure) of the restatement after EDGE_STEPS steps with tol = 0, computed once per session."""
    if (dim, N, dtype) not in _edge:
        z0, (ms, m2) = edge_case(dim, N)
        z, j, measure = R.mmpde5(z0, ms, m2, dtype=dtype, tol=0, max_steps=EDGE_STEPS)
        assert j == EDGE_STEPS
        _edge[(dim, N, dtype)] = (z, measure)
    return _edge[(dim, N, dtype)]


@pytest.mark.parametrize('dim,N', [(1, n) for n in EDGE_1D] + [(2, n) for n in EDGE_2D])
def test_edge_cases_move_in_fifty_default_steps(dim, N):
    """A comparison after 50 steps means something only if the nodes have moved by more than rounding: the fp64 restatement
    moves some node by at least 100 spacings of fp32 at 1.0 (measured: 184 at N = 1024 in 1-D, the least; 5e4 at 32 x 32)."""
    z0, _ = edge_case(dim, N)
    z, measure = edge_restated(dim, N, torch.float64)
    assert bool(torch.isfinite(z).all()) and measure > 0
    assert (z - z0.double()).abs().max().item() >= 100 * 2.0 ** -23
