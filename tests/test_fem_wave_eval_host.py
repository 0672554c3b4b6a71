"""The wave-parallel FEM kernels under the evaluation and the mesh descent, the host side: gadapt_fem_eval_errors_wave and
gadapt_fem_descend_wave of libgadapt_fem.so (symbols, prototypes, refusals before any launch, each compared with what the lane
entry point answers to the same broken argument list), and the `forward` / `adjoint` keywords of `poisson_eval_errors`,
`mesh_descent_2d` and `evaluation._errors_of`.  No GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from g_adaptivity_amd import _native_fem as nf
from g_adaptivity_amd import evaluation as ev
from g_adaptivity_amd import fem, hot_path_opt, mesh_descent_2d, poisson_eval_errors
from g_adaptivity_amd._native import NativeError
from g_adaptivity_amd.mesh_graph import MeshData, square_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'gadapt_fem.h')).read()
# wave entry point -> (its lane twin, the parameters it adds)
WAVE = {'gadapt_fem_eval_errors_wave': ('gadapt_fem_eval_errors', ['sol_work']),
        'gadapt_fem_descend_wave': ('gadapt_fem_descend', ['routes'])}

_buf = (C.c_double * 64)()                                    # dummy non-null HOST address, 8-byte aligned: never dereferenced
P = C.addressof(_buf)
_lat = (C.c_float * 4)(0.0, 0.5, 1.0, 0.0)
VALID = {'n_meshes': 1, 'n_nodes': 4, 'n_tris': 2, 'nlat': 3, 'max_lds_bytes': 1024, 'max_tris': 2, 'epochs': 1, 'lr': 0.1, 'routes': 3,
         'stream': None, 'lat_x': C.addressof(_lat), 'lat_y': C.addressof(_lat)}
BUDGET = 65536


def _decl(entry):
    return re.search(r'\b' + entry + r'\s*\(([^;]*)\);', HEADER).group(1)


def _names(entry):
    return [re.search(r'(\w+)\s*$', p).group(1) for p in _decl(entry).split(',')]


def _types(entry):
    return [re.sub(r'\s+', ' ', re.sub(r'\w+\s*$', '', p)).strip() for p in _decl(entry).split(',')]


@pytest.mark.parametrize('entry', sorted(WAVE))
def test_wave_symbol_header_and_prototype(entry):
    base, added = WAVE[entry]
    assert hasattr(nf.lib(), entry)                                            # exported by the library
    names, types = _names(entry), _types(entry)
    assert len(names) == len(nf.PROTOTYPES[entry][1]) == len(nf.PROTOTYPES[base][1]) + 1
    assert [n for n in names if n not in added] == _names(base)                # the lane entry point's list, one parameter more
    assert [t for n, t in zip(names, types) if n not in added] == _types(base)
    assert nf.PROTOTYPES[entry][0] is nf.PROTOTYPES[base][0]


def test_where_the_new_parameters_stand():
    names = _names('gadapt_fem_eval_errors_wave')
    i = names.index('sol_work')
    assert names[i - 1:i + 3] == ['lfac', 'sol_work', 'partials', 'err'] and _types('gadapt_fem_eval_errors_wave')[i] == 'float*'
    assert nf.PROTOTYPES['gadapt_fem_eval_errors_wave'][1][i] is C.c_void_p
    names = _names('gadapt_fem_descend_wave')
    assert names[-3:] == ['sign', 'routes', 'stream'] and _types('gadapt_fem_descend_wave')[-2] == 'int'
    assert nf.PROTOTYPES['gadapt_fem_descend_wave'][1][-2] is C.c_int
    assert (nf.ROUTE_WAVE_FORWARD, nf.ROUTE_WAVE_ADJOINT) == (1, 2)
    assert re.search(r'#define GADAPT_FEM_ROUTE_WAVE_FORWARD 1\b', HEADER) and re.search(r'#define GADAPT_FEM_ROUTE_WAVE_ADJOINT 2\b', HEADER)


def test_abi_version_is_unchanged():
    assert nf.lib().gadapt_fem_abi_version() == 4 and nf.ABI_VERSION == 4
    assert re.search(r'#define GADAPT_FEM_ABI 4\b', HEADER)


def test_entry_points_table():
    assert fem.ENTRY_POINTS['eval_errors_wave'] == {'lds': 'gadapt_fem_eval_errors_wave'}
    assert fem.ENTRY_POINTS['eval_errors'] == {'lds': 'gadapt_fem_eval_errors', 'window': 'gadapt_fem_eval_errors_window'}
    assert fem.ENTRY_POINTS['forward_wave'] == {'lds': 'gadapt_fem_forward_wave'}


def _call(entry, breaks):
    assert breaks, "an unbroken argument list would be launched on host addresses"
    names = _names(entry)
    assert set(breaks) <= set(names), (entry, breaks)
    lib = nf.lib()
    rc = getattr(lib, entry)(*[breaks[n] if n in breaks else VALID.get(n, P) for n in names])
    return rc, lib.gadapt_fem_last_error().decode()


def _same_refusal(entry, breaks, routes=None):
    """(code, message) of the wave entry point, asserted to be the lane entry point's for the same broken list, with the entry
    point's name substituted where it appears."""
    base = WAVE[entry][0]
    rc0, msg0 = _call(base, breaks)
    rc, msg = _call(entry, breaks if routes is None else dict(breaks, routes=routes))
    assert rc0 < 0, (base, breaks, 'the lane entry point accepted a list that was meant to be refused')
    want = re.sub(r'\b' + base + r'\b', entry, msg0)
    assert (rc, msg) == (rc0, want), (entry, breaks, (rc, msg), (rc0, want))
    return rc, msg


HEAD = ['meta', 'cells', 'node_mesh', 'int_idx', 'int_node', 'nt_ptr', 'nt_idx', 'gptr', 'gpar', 'x']
SIZES = ['n_meshes', 'n_nodes', 'n_tris', 'max_tris']


def test_eval_errors_wave_refuses_before_any_launch():
    """Every call here fails a check, and the checks come before the first launch (tests/test_fem_abi_host.py's pattern)."""
    entry = 'gadapt_fem_eval_errors_wave'
    null = f'{entry}: null pointer or bad size'
    for name in HEAD + ['rhs', 'coeffs', 'partials', 'err']:
        assert _same_refusal(entry, {name: None}) == (-1, null), name          # GADAPT_FEM_E_BADARG
    for size in SIZES:
        assert _same_refusal(entry, {size: 0}) == (-1, null), size
        assert _same_refusal(entry, {size: -3}) == (-1, null), size
    rc, msg = _same_refusal(entry, {'nlat': 1})
    assert rc == -1 and msg.startswith('evaluation lattice')
    for lds in (0, BUDGET + 1):
        rc, msg = _same_refusal(entry, {'max_lds_bytes': lds})
        assert rc == -5 and 'LDS' in msg                                       # GADAPT_FEM_E_LDS
    rc, msg = _same_refusal(entry, {'max_tris': 2049})
    assert rc == -5 and 'bin mask' in msg
    assert _same_refusal(entry, {'nlat': 46341}) == (-1, f'{entry}: nlat * nlat exceeds the int range')
    # the order of two faults
    for breaks in ({'meta': None, 'nlat': 1}, {'nlat': 1, 'max_lds_bytes': 0}, {'partials': None, 'max_lds_bytes': 0},
                   {'partials': None, 'nlat': 46341}, {'lfac': None, 'nlat': 46341}, {'max_tris': 2049, 'nlat': 46341},
                   {'err': None, 'meta': None}, {'lat_x': None}, {'lat_y': None}):
        _same_refusal(entry, breaks)


def test_eval_errors_wave_refuses_a_null_sol_work_where_partials_is_refused():
    entry = 'gadapt_fem_eval_errors_wave'
    null = f'{entry}: null pointer or bad size'
    assert _call(entry, {'sol_work': None}) == (-1, null)
    assert _call(entry, {'sol_work': None}) == _call(entry, {'partials': None}) == _call(entry, {'err': None})
    # after the LDS checks, before nlat's range: as partials and err are
    for more in ({'max_lds_bytes': 0}, {'max_tris': 2049}, {'nlat': 1}, {'meta': None}, {'nlat': 46341}):
        assert _call(entry, dict(more, sol_work=None)) == _call(entry, dict(more, partials=None)), more
    rc, msg = _call(entry, {'sol_work': None, 'max_lds_bytes': 0})
    assert rc == -5 and 'LDS' in msg
    assert _call(entry, {'sol_work': None, 'nlat': 46341}) == (-1, null)


@pytest.mark.parametrize('routes', [0, 1, 2, 3])
def test_descend_wave_refuses_before_any_launch(routes):
    entry = 'gadapt_fem_descend_wave'
    null = f'{entry}: null pointer or bad size'
    required = HEAD + ['tri_mesh', 'lat_x', 'lat_y', 'rhs', 'coeffs', 'lfac', 'sol', 'loss', 'g_sol', 'gc', 'mu', 'tgrad', 'gx',
                       'loss_hist', 'first_tangled', 'min_area', 'sign']
    for name in required:
        assert _same_refusal(entry, {name: None}, routes) == (-1, null), name
    for size in SIZES:
        assert _same_refusal(entry, {size: 0}, routes) == (-1, null), size
    assert _same_refusal(entry, {'epochs': -1}, routes) == (-1, null)
    for breaks in ({'nlat': 1}, {'nlat': 4}, {'nlat': 4, 'max_lds_bytes': 0}, {'epochs': -1, 'nlat': 4}):
        _same_refusal(entry, breaks, routes)
    assert _same_refusal(entry, {'nlat': 4}, routes) == (-1, f'{entry}: the Simpson rule needs an odd nlat >= 3')
    lds = f'{entry}: band factor or triangle bin mask outside the LDS budget'
    for breaks in ({'max_lds_bytes': 0}, {'max_lds_bytes': BUDGET + 1}, {'max_tris': 2049}, {'x_ref': None, 'max_lds_bytes': 0},
                   {'mesh_hist': None, 'max_lds_bytes': 0}, {'loss_hist': None, 'epochs': 0, 'max_lds_bytes': 0},
                   {'nlat': 46341, 'max_lds_bytes': 0}):
        assert _same_refusal(entry, breaks, routes) == (-5, lds), breaks
    # the lattice loss's row sums, under gadapt_fem_modular_forward's name from both; an nlat beyond the int range ends here
    rows = "gadapt_fem_modular_forward: the lattice's row sums exceed the LDS budget"
    assert _same_refusal(entry, {'nlat': 16385}, routes) == (-5, rows)
    assert _same_refusal(entry, {'nlat': 46341}, routes) == (-5, rows)


@pytest.mark.parametrize('routes', [4, 7, 8, -1, 1 << 16])
def test_descend_wave_refuses_unknown_routes(routes):
    entry = 'gadapt_fem_descend_wave'
    rc, msg = _call(entry, {'routes': routes})                                 # everything else is in order
    assert rc == -1 and msg.startswith(f'{entry}: routes')
    assert _call(entry, {'routes': routes, 'meta': None}) == (rc, msg)         # refused first
    assert _call(entry, {'routes': routes, 'max_lds_bytes': 0}) == (rc, msg)


# ------------------------------------------------------------------------------------------------ the keywords
def _one_mesh(n=5):
    m = square_mesh(n)
    p = [{'centers': [np.array([0.4, 0.6], 'f')], 'scales': [np.array([0.3, 0.2], 'f')]}]
    return m, p


def test_keywords_are_keyword_only_with_the_lane_default():
    for fn, names in ((poisson_eval_errors, ['forward']), (mesh_descent_2d, ['forward', 'adjoint'])):
        params = inspect.signature(fn).parameters
        for name in names:
            assert (params[name].kind, params[name].default) == (inspect.Parameter.KEYWORD_ONLY, 'lane'), (fn, name)
    assert hot_path_opt()['fem_forward'] == 'lane' and hot_path_opt()['fem_adjoint'] == 'lane'


def test_poisson_eval_errors_forward_is_checked_before_the_device():
    m, p = _one_mesh()
    x = m.x_comp.clone()                                                       # a CPU tensor: the value check comes first
    kw = dict(cells=m.cells, boundary=m.boundary_nodes)
    with pytest.raises(ValueError, match="poisson_eval_errors: forward='wave'.*band='window'"):
        poisson_eval_errors(x, [m.num_nodes], p, 9, band='window', forward='wave', **kw)
    with pytest.raises(ValueError, match="poisson_eval_errors: forward must be one of .*'lane', 'wave'.*'diag'"):
        poisson_eval_errors(x, [m.num_nodes], p, 9, forward='diag', **kw)
    for forward in ('lane', 'wave'):                                           # a valid value: the next check is the device's
        with pytest.raises(NativeError, match='MI355X only'):
            poisson_eval_errors(x, [m.num_nodes], p, 9, forward=forward, **kw)


def test_poisson_eval_errors_1d_does_not_read_forward():
    """1-D input ignores `forward` as it ignores `band`: whatever it holds, the first refusal of a CPU tensor is the device's."""
    x = torch.linspace(0, 1, 11)
    p = [{'centers': [np.array([0.4], 'f')], 'scales': [np.array([0.3], 'f')]}]
    for shape in (x, x[:, None]):
        for kw in ({'forward': 'diag'}, {'forward': 'wave', 'band': 'window'}, {'forward': None}):
            with pytest.raises(NativeError, match='MI355X only'):
                poisson_eval_errors(shape, [11], p, 9, **kw)


def test_mesh_descent_2d_unknown_routes_raise_before_the_device():
    m, p = _one_mesh()
    x = m.x_comp.clone()
    args = (x, m.cells, m.boundary_nodes, [m.num_nodes], p, 3, 0.05)
    with pytest.raises(ValueError, match="mesh_descent_2d: forward must be one of .*'lane', 'wave'.*'diag'"):
        mesh_descent_2d(*args, forward='diag')
    with pytest.raises(ValueError, match="mesh_descent_2d: adjoint must be one of .*'lane', 'wave'.*'diag'"):
        mesh_descent_2d(*args, adjoint='diag')
    with pytest.raises(ValueError, match="forward must be one of"):
        mesh_descent_2d(*args, forward='diag', adjoint='diag')
    for kw in ({}, {'forward': 'wave'}, {'adjoint': 'wave'}, {'forward': 'wave', 'adjoint': 'wave'}):
        with pytest.raises(NativeError, match='MI355X only'):
            mesh_descent_2d(*args, **kw)
    with pytest.raises(TypeError):
        mesh_descent_2d(*args, None, None, None, False, None, 'wave')          # keyword-only


def test_errors_of_refuses_the_window_wave_pair():
    m, p = _one_mesh()
    s = MeshData(x_comp=m.x_comp, x_phys=m.x_comp, cells=m.cells, boundary_nodes=m.boundary_nodes, pde_params=p[0])
    window = hot_path_opt(mesh_dims=[5, 5], fem_forward='wave', fem_band='window')
    with pytest.raises(ValueError, match="fem_forward.*forward='wave'.*band='window'"):
        ev._errors_of([s.x_comp], [s], 9, window, torch.device('cpu'))
    with pytest.raises(ValueError, match="fem_forward.*'diag'"):
        ev._errors_of([s.x_comp], [s], 9, hot_path_opt(mesh_dims=[5, 5], fem_forward='diag'), torch.device('cpu'))
    with pytest.raises(ValueError, match="forward='wave'.*band='window'"):
        ev.eval_grid_MMPDE_MA([s], dict(window, device='cpu'))
    for opt in (hot_path_opt(mesh_dims=[5, 5], fem_forward='wave'), hot_path_opt(mesh_dims=[5, 5])):
        with pytest.raises(NativeError, match='MI355X only'):                  # a valid pair goes on to the device's check
            ev._errors_of([s.x_comp], [s], 9, opt, torch.device('cpu'))
