"""pde_loss as a captured step, the host side: the two wave-adjoint entry points of libgadapt_fem.so (symbols, prototypes,
refusals before any launch), the `adjoint` / opt['fem_adjoint'] keyword, and `fem.PdeBatch`'s Gaussian staging.  No GPU."""
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
WAVE = {'gadapt_fem_backward_wave': 'gadapt_fem_backward', 'gadapt_fem_backward_window_wave': 'gadapt_fem_backward_window'}

_buf = (C.c_double * 64)()                                    # dummy non-null HOST address, 8-byte aligned: never dereferenced
P = C.addressof(_buf)
VALID = {'n_meshes': 1, 'n_nodes': 4, 'n_tris': 2, 'nlat': 3, 'max_lds_bytes': 1024, 'stream': None}


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
    assert fem.ENTRY_POINTS['backward_wave'] == {'lds': 'gadapt_fem_backward_wave', 'window': 'gadapt_fem_backward_window_wave'}


def test_abi_version_is_unchanged():
    assert nf.lib().gadapt_fem_abi_version() == 4 and nf.ABI_VERSION == 4
    assert re.search(r'#define GADAPT_FEM_ABI 4\b', HEADER)


def _call(entry, breaks):
    assert breaks, "an unbroken argument list would be launched on host addresses"
    names = _names(entry)
    assert set(breaks) <= set(names)
    lib = nf.lib()
    rc = getattr(lib, entry)(*[breaks[n] if n in breaks else VALID.get(n, P) for n in names])
    return rc, lib.gadapt_fem_last_error().decode()


REQUIRED = ['meta', 'cells', 'node_mesh', 'tri_mesh', 'int_idx', 'int_node', 'nt_ptr', 'nt_idx', 'gptr', 'gpar', 'x', 'coeffs', 'gc', 'mu',
            'tgrad', 'gx']


@pytest.mark.parametrize('entry,factor', [('gadapt_fem_backward_wave', 'lfac'), ('gadapt_fem_backward_window_wave', 'work')])
def test_wave_entry_points_refuse_before_any_launch(entry, factor):
    """Every call here fails a check, and the checks come before the first launch (tests/test_fem_abi_host.py's pattern)."""
    null = f'{entry}: null pointer or bad size'
    for name in REQUIRED + [factor]:
        assert _call(entry, {name: None}) == (-1, null), name                  # GADAPT_FEM_E_BADARG
    for size in ('n_meshes', 'n_nodes', 'n_tris'):
        assert _call(entry, {size: 0}) == (-1, null), size
    assert _call(entry, {'n_meshes': -3}) == (-1, null)
    rc, msg = _call(entry, {'nlat': 1})
    assert rc == -1 and msg.startswith('evaluation lattice')
    # g_coeffs and g_sol are optional: a NULL one is accepted on the way to a later refusal (the LDS of the adjoint solve)
    rc, msg = _call(entry, {'g_coeffs': None, 'g_sol': None, 'max_lds_bytes': 0})
    assert rc == -5 and 'LDS' in msg, (rc, msg)                                # GADAPT_FEM_E_LDS
    if factor == 'work':
        assert _call(entry, {'work': P + 4}) == (-1, null)                     # the fp64 workspace: 8-byte aligned


# ------------------------------------------------------------------------------------------------ the keyword
def test_hot_path_opt_lists_the_lane_adjoint():
    assert hot_path_opt()['fem_adjoint'] == 'lane'
    assert hot_path_opt(fem_adjoint='wave')['fem_adjoint'] == 'wave'


def _one_mesh(n=5):
    m = square_mesh(n)
    p = [{'centers': [np.array([0.4, 0.6], 'f')], 'scales': [np.array([0.3, 0.2], 'f')]}]
    return m, p


def test_unknown_adjoint_raises_before_anything_is_launched():
    m, p = _one_mesh()
    lat = torch.linspace(0, 1, 5)
    x = m.x_comp.clone()                                                       # a CPU tensor: the value check comes before the device check
    with pytest.raises(ValueError, match="adjoint must be one of .*'diag'"):
        fem.fem_poisson(x, m.cells, m.boundary_nodes, [m.num_nodes], p, (lat, lat), adjoint='diag')
    with pytest.raises(ValueError, match="adjoint must be one of .*'diag'"):
        fem.modular_loss_2d(x, m.cells, m.boundary_nodes, [m.num_nodes], p, 5, 'mse', adjoint='diag')
    with pytest.raises(ValueError, match="adjoint must be one of .*'diag'"):
        fem.PdeBatch(_topology(m), lat, lat, 8, adjoint='diag')


def test_unknown_opt_fem_adjoint_raises():
    m, p = _one_mesh()
    opt = hot_path_opt(mesh_dims=[5, 5], loss_type='pde_loss', fem_adjoint='diag')

    class Model:
        dim = 2
    Model.opt = opt
    data = MeshData(x_comp=m.x_comp, cells=m.cells, boundary_nodes=m.boundary_nodes, batch=None, pde_params=p)
    with pytest.raises(ValueError, match="fem_adjoint.*'diag'"):
        fem.gnn_pde_tail(Model(), data, m.x_comp.clone())
    o = dict(opt, grad_type='PDE_loss_direct_mse')
    with pytest.raises(ValueError, match="fem_adjoint.*'diag'"):
        fem.gradient_meshpoints_2D(o, data, m.x_comp.clone())


# ------------------------------------------------------------------------------------------------ PdeBatch
def _topology(m, copies=1):
    n, t = m.num_nodes, m.cells.shape[0]
    cells = np.concatenate([m.cells.numpy() + b * n for b in range(copies)])
    bnd = np.concatenate([m.boundary_nodes.numpy()] * copies)
    return fem.FemTopology(cells, bnd, [n] * copies, [t] * copies, 'cpu')


def _gauss(k, seed):
    rng = np.random.default_rng(seed)
    return {'centers': [rng.uniform(0, 1, 2).astype('f') for _ in range(k)], 'scales': [rng.uniform(0.1, 0.5, 2).astype('f') for _ in range(k)]}


def test_pde_batch_packs_what_pack_gaussians_packs():
    lat = torch.linspace(0, 1, 5)
    pb = fem.PdeBatch(_topology(square_mesh(5), 3), lat, lat, cap=3 * 8)
    assert (pb.n_meshes, pb.n_nodes, pb.n_tris, pb.cap) == (3, 75, 96, 24) and all(type(v) is int for v in (pb.n_nodes, pb.n_tris))
    assert pb.gptr.shape == (4,) and pb.gptr.dtype == torch.int32 and pb.gpar.shape == (24, 4) and pb.gpar.dtype == torch.float32
    assert pb.host_gptr.shape == pb.gptr.shape and pb.host_gpar.shape == pb.gpar.shape
    ptr0, par0 = pb.gptr.data_ptr(), pb.gpar.data_ptr()
    for counts, seed in (((1, 3, 2), 0), ((3, 1, 1), 1), ((2, 2, 2), 2)):        # mixed counts; a second batch with fewer rows
        params = [_gauss(k, 10 * seed + i) for i, k in enumerate(counts)]
        pb.set_params(params)
        gptr, gpar = fem.pack_gaussians(params, 'cpu')
        g = gpar.shape[0]
        assert torch.equal(pb.host_gptr, gptr) and torch.equal(pb.host_gpar[:g], gpar)       # the staging buffer
        assert torch.equal(pb.gptr, gptr) and torch.equal(pb.gpar[:g], gpar)                 # ... and what the kernels are given
        assert (pb.gptr.data_ptr(), pb.gpar.data_ptr()) == (ptr0, par0)                      # the same tensors
    assert pb.gptr.tolist() == [0, 2, 4, 6]


def test_pde_batch_refuses_more_rows_than_its_capacity():
    lat = torch.linspace(0, 1, 5)
    pb = fem.PdeBatch(_topology(square_mesh(5), 2), lat, lat, cap=4)
    pb.set_params([_gauss(2, 0), _gauss(2, 1)])
    before = (pb.host_gptr.clone(), pb.host_gpar.clone(), pb.gpar.clone())
    with pytest.raises(ValueError, match=r'\b5 Gaussians.*room for 4\b'):
        pb.set_params([_gauss(2, 2), _gauss(3, 3)])
    assert all(torch.equal(a, b) for a, b in zip(before, (pb.host_gptr, pb.host_gpar, pb.gpar)))   # raised before any copy
    with pytest.raises(ValueError, match='3 meshes'):
        pb.set_params([_gauss(1, 0)] * 3)
