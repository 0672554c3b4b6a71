"""Host side of the windowed FEM route (band='window'): the new C-ABI symbols, the ring's LDS need, the workspace size and the
topology's two limits.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from g_adaptivity_amd import _native_fem as nf
from g_adaptivity_amd.fem import FemTopology
from g_adaptivity_amd.mesh_graph import square_mesh
from g_adaptivity_amd.params import hot_path_opt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I, _L = C.c_void_p, C.c_int, C.c_int64


def test_symbols_and_signatures():
    lib = nf.lib()
    want = {
        'gadapt_fem_window_lds_bytes': (_L, [_I, _I]),
        'gadapt_fem_window_workspace_floats': (_L, [_I, _P]),
        # gadapt_fem_eval_errors' arguments with the workspace in lfac's place and tri_slab after it
        'gadapt_fem_eval_errors_window': (_I, [_I, _I, _I] + [_P] * 12 + [_I, _I, _I] + [_P] * 3 + [_I] + [_P] * 3),
    }
    for name, (res, args) in want.items():
        assert nf.PROTOTYPES[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    base = nf.PROTOTYPES['gadapt_fem_eval_errors'][1]
    assert len(want['gadapt_fem_eval_errors_window'][1]) == len(base) + 1
    header = open(os.path.join(ROOT, 'include', 'gadapt_fem.h')).read()
    for name in want:
        assert re.search(r'\b' + name + r'\(', header), name


def test_abi_number_unchanged():
    assert nf.ABI_VERSION == 4 and nf.lib().gadapt_fem_abi_version() == 4
    assert '#define GADAPT_FEM_ABI 4' in open(os.path.join(ROOT, 'include', 'gadapt_fem.h')).read()


def test_ring_lds_bytes():
    lib = nf.lib()
    budget = lib.gadapt_fem_lds_budget()
    at64 = lib.gadapt_fem_window_lds_bytes(3844, 63)                       # more than 64 x 64 nodes need (their band is 62)
    assert 0 < at64 <= budget
    assert at64 >= 8 * (64 * 64 + 64) + 4 * (63 * 64 // 2)                  # w + 1 fp64 rows of w + 1, their right-hand side, the pairs
    need = [lib.gadapt_fem_window_lds_bytes(3844, w) for w in range(0, 130)]
    assert all(b > a for a, b in zip(need, need[1:]))                       # grows with w
    # the largest square mesh the header and the README state: 81 x 81 (band 79); 128 x 128 (band 126) is refused
    assert lib.gadapt_fem_window_lds_bytes(79 * 79, 79) <= budget < lib.gadapt_fem_window_lds_bytes(80 * 80, 80)
    assert lib.gadapt_fem_window_lds_bytes(126 * 126, 126) > budget


def test_workspace_floats():
    lib = nf.lib()
    meta = np.zeros((2, nf.META), np.int32)
    meta[0, nf.M_N_INT], meta[0, nf.M_BAND] = 81, 10
    meta[1, nf.M_N_INT], meta[1, nf.M_BAND] = 3844, 63
    # the issue's sum n_int (w + 1), held in fp64 (two floats each) with the fp64 intermediate y [n_int] beside each factor
    assert lib.gadapt_fem_window_workspace_floats(2, meta.ctypes.data) == 2 * (81 * 11 + 3844 * 64) + 2 * (81 + 3844)
    assert lib.gadapt_fem_window_workspace_floats(0, meta.ctypes.data) < 0


def test_topology_routes_at_64():
    m = square_mesh(64)
    args = (m.cells.numpy(), m.boundary_nodes.numpy(), [64 * 64], [int(m.cells.shape[0])], 'cpu')
    topo = FemTopology(*args, band='window')
    assert topo.route == 'window' and int(topo.n_int[0]) == 62 * 62 and int(topo.band[0]) == 62
    assert topo.lds_bytes == nf.lib().gadapt_fem_window_lds_bytes(3844, 62)
    assert topo.band_floats == 3844 * 63
    assert nf.lib().gadapt_fem_window_workspace_floats(1, topo.host['meta'].ctypes.data) == 2 * 3844 * (63 + 1)
    assert topo.max_tris == 2 * 63 * 63
    with pytest.raises(NotImplementedError, match=r"LDS.*26 x 26.*band='window'"):
        FemTopology(*args, band='lds')
    with pytest.raises(NotImplementedError, match=r"LDS.*26 x 26"):
        FemTopology(*args)                                                  # the default is the resident band
    with pytest.raises(ValueError, match='band'):
        FemTopology(*args, band='auto')
    for n, fits in ((81, True), (82, False), (128, False)):
        big = square_mesh(n)
        big_args = (big.cells.numpy(), big.boundary_nodes.numpy(), [n * n], [int(big.cells.shape[0])], 'cpu')
        if fits:
            assert int(FemTopology(*big_args, band='window').band[0]) == n - 2
        else:
            with pytest.raises(NotImplementedError, match='81 x 81'):
                FemTopology(*big_args, band='window')


def test_opt_key_listed_with_its_default():
    assert hot_path_opt()['fem_band'] == 'lds'
