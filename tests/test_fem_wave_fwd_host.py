"""The wave-parallel FEM forward, the host side: the two entry points of libgadapt_fem.so (symbols, prototypes, refusals before
any launch, each compared with what the lane entry point answers to the same broken argument list), and the `forward` /
opt['fem_forward'] keyword.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from g_adaptivity_amd import _native_fem as nf
from g_adaptivity_amd import fem, hot_path_opt
from g_adaptivity_amd.mesh_graph import MeshData, square_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'gadapt_fem.h')).read()
WAVE = {'gadapt_fem_forward_wave': 'gadapt_fem_forward', 'gadapt_fem_modular_forward_wave': 'gadapt_fem_modular_forward'}

_buf = (C.c_double * 64)()                                    # dummy non-null HOST address, 8-byte aligned: never dereferenced
P = C.addressof(_buf)
_lat = (C.c_float * 4)(0.0, 0.5, 1.0, 0.0)
VALID = {'n_meshes': 1, 'n_nodes': 4, 'n_tris': 2, 'nlat': 3, 'max_lds_bytes': 1024, 'max_tris': 2, 'reduction': nf.LOSS_MSE,
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
    base = WAVE[entry]
    assert hasattr(nf.lib(), entry)                                            # exported by the library
    assert nf.PROTOTYPES[entry] == nf.PROTOTYPES[base]
    assert _names(entry) == _names(base) and _types(entry) == _types(base)     # the header: the argument list of the lane entry point
    assert len(_names(entry)) == len(nf.PROTOTYPES[entry][1])
    assert fem.ENTRY_POINTS['forward_wave'] == {'lds': 'gadapt_fem_forward_wave'}
    assert fem.ENTRY_POINTS['modular_forward_wave'] == {'lds': 'gadapt_fem_modular_forward_wave'}


def test_abi_version_is_unchanged():
    assert nf.lib().gadapt_fem_abi_version() == 4 and nf.ABI_VERSION == 4
    assert re.search(r'#define GADAPT_FEM_ABI 4\b', HEADER)


def _call(entry, breaks):
    assert breaks, "an unbroken argument list would be launched on host addresses"
    names = _names(entry)
    assert set(breaks) <= set(names), (entry, breaks)
    lib = nf.lib()
    rc = getattr(lib, entry)(*[breaks[n] if n in breaks else VALID.get(n, P) for n in names])
    return rc, lib.gadapt_fem_last_error().decode()


def _same_refusal(entry, breaks):
    """(code, message) of the wave entry point, asserted to be the lane entry point's for the same broken list, with the entry
    point's name substituted where it appears."""
    base = WAVE[entry]
    rc0, msg0 = _call(base, breaks)
    rc, msg = _call(entry, breaks)
    assert rc0 < 0, (base, breaks, 'the lane entry point accepted a list that was meant to be refused')
    want = re.sub(r'\b' + base + r'\b', entry, msg0)
    assert (rc, msg) == (rc0, want), (entry, breaks, (rc, msg), (rc0, want))
    return rc, msg


POINTERS = ['meta', 'cells', 'node_mesh', 'int_idx', 'int_node', 'nt_ptr', 'nt_idx', 'gptr', 'gpar', 'x', 'rhs', 'coeffs', 'lfac', 'sol']
SIZES = ['n_meshes', 'n_nodes', 'n_tris', 'max_tris']
# broken lists of both entry points: orders of two faults, the bin mask beyond the budget, a huge nlat (no upper limit here)
ORDER = [{'meta': None, 'nlat': 1}, {'nlat': 1, 'max_lds_bytes': 0}, {'sol': None, 'meta': None}, {'max_lds_bytes': BUDGET + 1},
         {'max_tris': 2049}, {'max_lds_bytes': 0, 'max_tris': 2049}, {'lfac': None, 'max_lds_bytes': 0}, {'sol': None, 'max_tris': 2049},
         {'nlat': 46341, 'sol': None}, {'lat_x': None}, {'lat_y': None}]


def test_forward_wave_refuses_before_any_launch():
    """Every call here fails a check, and the checks come before the first launch (tests/test_fem_abi_host.py's pattern)."""
    entry = 'gadapt_fem_forward_wave'
    null = f'{entry}: null pointer or bad size'
    for name in POINTERS:
        assert _same_refusal(entry, {name: None}) == (-1, null), name          # GADAPT_FEM_E_BADARG
    for size in SIZES:
        assert _same_refusal(entry, {size: 0}) == (-1, null), size
        assert _same_refusal(entry, {size: -3}) == (-1, null), size
    rc, msg = _same_refusal(entry, {'nlat': 1})
    assert rc == -1 and msg.startswith('evaluation lattice')
    rc, msg = _same_refusal(entry, {'max_lds_bytes': 0})
    assert rc == -5 and 'LDS' in msg                                           # GADAPT_FEM_E_LDS
    for breaks in ORDER:
        _same_refusal(entry, breaks)


def test_modular_forward_wave_refuses_before_any_launch():
    """The loss arguments under the entry point's own name, before the shared ones, which gadapt_fem_modular_forward has always
    reported under gadapt_fem_forward's name: so does the wave entry point."""
    entry = 'gadapt_fem_modular_forward_wave'
    bad = f'{entry}: null output or unknown reduction'
    for breaks in ({'loss': None}, {'g_sol': None}, {'reduction': 2}, {'reduction': -1}, {'n_meshes': 0}, {'reduction': 2, 'meta': None}):
        assert _same_refusal(entry, breaks) == (-1, bad), breaks
    for breaks in ({'reduction': nf.LOSS_SIMPSON, 'nlat': 4}, {'reduction': nf.LOSS_SIMPSON, 'nlat': 1},
                   {'reduction': nf.LOSS_SIMPSON, 'nlat': 4, 'meta': None}):
        assert _same_refusal(entry, breaks) == (-1, f'{entry}: the Simpson rule needs an odd nlat >= 3'), breaks
    for breaks in ({'nlat': 16385}, {'nlat': 16385, 'reduction': nf.LOSS_SIMPSON}, {'nlat': 16385, 'meta': None}):
        assert _same_refusal(entry, breaks) == (-5, f"{entry}: the lattice's row sums exceed the LDS budget"), breaks
    null = 'gadapt_fem_forward: null pointer or bad size'
    for name in POINTERS:
        assert _same_refusal(entry, {name: None}) == (-1, null), name
    for size in SIZES[1:]:
        assert _same_refusal(entry, {size: 0}) == (-1, null), size
        assert _same_refusal(entry, {size: -3}) == (-1, null), size
    rc, msg = _same_refusal(entry, {'nlat': 1})
    assert rc == -1 and msg.startswith('evaluation lattice')
    rc, msg = _same_refusal(entry, {'max_lds_bytes': 0})
    assert rc == -5 and 'LDS' in msg
    for breaks in ORDER:
        _same_refusal(entry, breaks)


# ------------------------------------------------------------------------------------------------ the keyword
def test_hot_path_opt_lists_the_lane_forward():
    assert hot_path_opt()['fem_forward'] == 'lane'
    assert hot_path_opt(fem_forward='wave')['fem_forward'] == 'wave'


def _one_mesh(n=5):
    m = square_mesh(n)
    p = [{'centers': [np.array([0.4, 0.6], 'f')], 'scales': [np.array([0.3, 0.2], 'f')]}]
    return m, p


def _topology(m, band='lds'):
    return fem.FemTopology(m.cells.numpy(), m.boundary_nodes.numpy(), [m.num_nodes], [m.cells.shape[0]], 'cpu', band)


def test_keyword_is_the_last_parameter_and_keyword_only():
    import inspect
    for fn in (fem.fem_poisson, fem.modular_loss_2d, fem.PdeBatch.__init__):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert (last.name, last.kind, last.default) == ('forward', inspect.Parameter.KEYWORD_ONLY, 'lane'), fn
    assert inspect.signature(fem.PdeBatch.from_data).parameters['forward'].default is None


def test_unknown_forward_raises_before_anything_is_launched():
    m, p = _one_mesh()
    lat = torch.linspace(0, 1, 5)
    x = m.x_comp.clone()                                                       # a CPU tensor: the value check comes before the device check
    match = "forward must be one of .*'lane', 'wave'.*'diag'"
    with pytest.raises(ValueError, match=match):
        fem.fem_poisson(x, m.cells, m.boundary_nodes, [m.num_nodes], p, (lat, lat), forward='diag')
    with pytest.raises(ValueError, match=match):
        fem.modular_loss_2d(x, m.cells, m.boundary_nodes, [m.num_nodes], p, 5, 'mse', forward='diag')
    with pytest.raises(ValueError, match=match):
        fem.PdeBatch(_topology(m), lat, lat, 8, forward='diag')


def test_wave_forward_on_the_windowed_route_raises():
    m, p = _one_mesh()
    lat = torch.linspace(0, 1, 5)
    x = m.x_comp.clone()
    match = "forward='wave'.*band='window'"
    with pytest.raises(ValueError, match=match):
        fem.fem_poisson(x, m.cells, m.boundary_nodes, [m.num_nodes], p, (lat, lat), band='window', forward='wave')
    with pytest.raises(ValueError, match=match):
        fem.modular_loss_2d(x, m.cells, m.boundary_nodes, [m.num_nodes], p, 5, 'mse', band='window', forward='wave')
    with pytest.raises(ValueError, match=match):
        fem.PdeBatch(_topology(m, 'window'), lat, lat, 8, forward='wave')
    assert fem.PdeBatch(_topology(m), lat, lat, 8, forward='wave').forward == 'wave'
    assert fem.PdeBatch(_topology(m), lat, lat, 8).forward == 'lane'


class _Model:
    dim = 2

    def __init__(self, opt):
        self.opt = opt


def test_unknown_opt_fem_forward_raises():
    m, p = _one_mesh()
    opt = hot_path_opt(mesh_dims=[5, 5], loss_type='pde_loss', fem_forward='diag')
    data = MeshData(x_comp=m.x_comp, cells=m.cells, boundary_nodes=m.boundary_nodes, batch=None, pde_params=p)
    with pytest.raises(ValueError, match="fem_forward.*'diag'"):
        fem.gnn_pde_tail(_Model(opt), data, m.x_comp.clone())
    with pytest.raises(ValueError, match="fem_forward.*'diag'"):
        fem.gradient_meshpoints_2D(dict(opt, grad_type='PDE_loss_direct_mse'), data, m.x_comp.clone())
    window = hot_path_opt(mesh_dims=[5, 5], loss_type='pde_loss', fem_forward='wave', fem_band='window')
    with pytest.raises(ValueError, match="forward='wave'.*band='window'"):
        fem.gnn_pde_tail(_Model(window), data, m.x_comp.clone())
    with pytest.raises(ValueError, match="forward='wave'.*band='window'"):
        fem.gradient_meshpoints_2D(dict(window, grad_type='PDE_loss_direct_mse'), data, m.x_comp.clone())


def test_check_tail_still_returns_band_and_adjoint():
    for fwd in ('lane', 'wave'):
        opt = hot_path_opt(mesh_dims=[5, 5], loss_type='pde_loss', fem_adjoint='wave', fem_forward=fwd)
        assert fem._check_tail(_Model(opt)) == ('lds', 'wave')
