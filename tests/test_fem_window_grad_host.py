"""Host side of the differentiable windowed FEM route (band='window' of fem_poisson, modular_loss_2d and their callers): the
three C-ABI symbols, their argument lists against the resident-band entry points', and the route arguments refused before the
GPU is asked for.  No GPU."""
import ctypes as C
import os
import re

import pytest
import torch

from g_adaptivity_amd import _native_fem as nf
from g_adaptivity_amd.fem import fem_poisson, gradient_meshpoints_2D, modular_loss_2d
from g_adaptivity_amd.mesh_graph import MeshData, square_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I = C.c_void_p, C.c_int
NEW = ('gadapt_fem_forward_window', 'gadapt_fem_modular_forward_window', 'gadapt_fem_backward_window')


def _header():
    return open(os.path.join(ROOT, 'include', 'gadapt_fem.h')).read()


def _params_of(name):
    """The parameter declarations of `name` in the header, in order."""
    decl = re.search(r'\b' + name + r'\s*\(([^;]*)\);', _header()).group(1)
    return [' '.join(p.split()) for p in decl.split(',')]


def test_symbols_in_library_table_and_header():
    lib = nf.lib()
    for name in NEW:
        assert name in nf.PROTOTYPES, name
        fn = getattr(lib, name)
        res, args = nf.PROTOTYPES[name]
        assert res is _I and fn.restype is _I and list(fn.argtypes) == args, name
        assert len(_params_of(name)) == len(args), name


def test_argument_lists_follow_the_base_entry_points():
    # forward: the workspace in lfac's place, tri_slab after it
    base, win = _params_of('gadapt_fem_forward'), _params_of('gadapt_fem_forward_window')
    k = base.index('float* lfac')
    assert win == base[:k] + ['float* work', 'int tri_slab'] + base[k + 1:]
    tb, tw = nf.PROTOTYPES['gadapt_fem_forward'][1], nf.PROTOTYPES['gadapt_fem_forward_window'][1]
    assert tw == tb[:k + 1] + [_I] + tb[k + 1:]
    # modular forward: the same, with the outputs loss and g_sol kept
    base, win = _params_of('gadapt_fem_modular_forward'), _params_of('gadapt_fem_modular_forward_window')
    k = base.index('float* lfac')
    assert win == base[:k] + ['float* work', 'int tri_slab'] + base[k + 1:]
    assert win[-3:] == ['float* loss', 'float* g_sol', 'void* stream']
    tb, tw = nf.PROTOTYPES['gadapt_fem_modular_forward'][1], nf.PROTOTYPES['gadapt_fem_modular_forward_window'][1]
    assert tw == tb[:k + 1] + [_I] + tb[k + 1:]
    # backward: the workspace in lfac's place, nothing else
    base, win = _params_of('gadapt_fem_backward'), _params_of('gadapt_fem_backward_window')
    k = base.index('const float* lfac')
    assert win == base[:k] + ['float* work'] + base[k + 1:]
    assert nf.PROTOTYPES['gadapt_fem_backward_window'][1] == nf.PROTOTYPES['gadapt_fem_backward'][1]


def test_abi_number_unchanged():
    assert nf.ABI_VERSION == 4 and nf.lib().gadapt_fem_abi_version() == 4
    assert '#define GADAPT_FEM_ABI 4' in _header()


def test_entry_points_validate_before_launching():
    lib = nf.lib()
    fwd = [1, 4, 2] + [None] * 12 + [2, 1024, 2] + [None] * 3 + [0] + [None] * 2
    assert lib.gadapt_fem_forward_window(*fwd) == -1 and b'gadapt_fem_forward_window' in lib.gadapt_fem_last_error()
    mod = [1, 4, 2] + [None] * 12 + [3, 1024, 2, nf.LOSS_MSE] + [None] * 3 + [0] + [None] * 4
    assert lib.gadapt_fem_modular_forward_window(*mod) == -1 and b'gadapt_fem_modular_forward_window' in lib.gadapt_fem_last_error()
    bwd = [1, 4, 2] + [None] * 13 + [2, 1024] + [None] * 9
    assert lib.gadapt_fem_backward_window(*bwd) == -1 and b'gadapt_fem_backward_window' in lib.gadapt_fem_last_error()
    # all pointers given (host memory: nothing may be launched on it): the slab, the ring and the alignment are refused first
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    lat = (C.c_float * 2)(0.0, 1.0)
    pl = C.addressof(lat)

    def forward(lds, slab, work=p):
        return lib.gadapt_fem_forward_window(1, 4, 2, *([p] * 10), pl, pl, 2, lds, 2, p, p, work, slab, p, None)
    for slab in (-32, 48, 1):
        assert forward(1024, slab) == -1 and b'tri_slab' in lib.gadapt_fem_last_error()
    assert forward(0, 0) == -5 and forward(lib.gadapt_fem_lds_budget() + 1, 0) == -5
    assert forward(1024, 0, work=p + 4) == -1                                    # the fp64 workspace must be 8-byte aligned
    assert lib.gadapt_fem_backward_window(1, 4, 2, *([p] * 11), pl, pl, 2, 0, p, p, None, p, p, p, p, p, None) == -5
    assert lib.gadapt_fem_backward_window(1, 4, 2, *([p] * 11), pl, pl, 2, 1024, p, p + 4, None, p, p, p, p, p, None) == -1


def _cpu_case(n=5):
    m = square_mesh(n)
    p = {'centers': [[0.5, 0.5]], 'scales': [[0.3, 0.3]]}
    return m, p


def test_bad_band_is_a_value_error_before_the_gpu_requirement():
    m, p = _cpu_case()
    x = m.x_comp.clone()                                                        # a CPU tensor: a good band would raise NativeError
    lat = torch.linspace(0, 1, 11)
    with pytest.raises(ValueError, match='band'):
        fem_poisson(x, m.cells, m.boundary_nodes, [m.num_nodes], [p], [lat, lat], band='ring')
    with pytest.raises(ValueError, match='band'):
        modular_loss_2d(x, m.cells, m.boundary_nodes, [m.num_nodes], [p], 11, 'mse', band='ring')
    data = MeshData(cells=m.cells, boundary_nodes=m.boundary_nodes, pde_params=[p])
    opt = dict(grad_type='PDE_loss_direct_mse', mesh_dims=[5, 5], eval_quad_points=101, load_quad_points=101, fem_band='ring')
    with pytest.raises(ValueError, match='band'):
        gradient_meshpoints_2D(opt, data, x)
    for slab in (-32, 48, 1):
        with pytest.raises(ValueError, match='tri_slab'):
            fem_poisson(x, m.cells, m.boundary_nodes, [m.num_nodes], [p], [lat, lat], band='window', tri_slab=slab)
        with pytest.raises(ValueError, match='tri_slab'):
            modular_loss_2d(x, m.cells, m.boundary_nodes, [m.num_nodes], [p], 11, 'mse', band='window', tri_slab=slab)
