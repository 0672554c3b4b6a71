"""CPU checks of route='strided' of the MMPDE5 generator (g_adaptivity_amd.mmpde5): the refusals, which come before any device
is looked for, and that the size-edge cases of tests/test_gpu_mmpde5_strided.py move by more than rounding."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_mmpde5_host import edge_case, edge_restated  # noqa: E402

from g_adaptivity_amd import _native_mesh, mmpde5_batch  # noqa: E402

# lanes T = min(whole waves, 1024), nodes per lane K = ceil(N^2 / T):
#   33: K = 2, 65 nodes in the second slot     45: K = 2, nearly full     46: the first K = 3
#   64: K = 4, exactly full                    65: K = 5, nearly empty    81: K = 7, the largest LDS
STRIDED_EDGE_2D = (33, 45, 46, 64, 65, 81)


def test_edges_are_the_edges_of_the_lane_mapping():
    k = {n: -(-n * n // min((n * n + 63) // 64 * 64, 1024)) for n in STRIDED_EDGE_2D}
    assert k == {33: 2, 45: 2, 46: 3, 64: 4, 65: 5, 81: 7}
    assert 33 * 33 - 1024 == 65 and 64 * 64 == 4 * 1024 and 65 * 65 - 4 * 1024 == 129
    assert _native_mesh.STRIDED_MAX_SIDE == 81 and _native_mesh.MAX_NODES == 1024 and _native_mesh.ABI_VERSION == 2


def test_strided_refusals_come_before_the_device():
    ones = torch.ones
    with pytest.raises(ValueError, match='81'):
        mmpde5_batch([torch.zeros(2, 82, 82)], [(ones(81, 81), ones(82, 82))], route='strided')
    with pytest.raises(ValueError, match='1024'):
        mmpde5_batch([torch.linspace(0, 1, 1025)], [(ones(1024), ones(1025))], route='strided')
    with pytest.raises(ValueError, match='route'):
        mmpde5_batch([torch.linspace(0, 1, 21)], [(ones(20), ones(21))], route='wide')
    with pytest.raises(ValueError, match='route'):
        mmpde5_batch([torch.zeros(2, 82, 82)], [(ones(81, 81), ones(82, 82))], route=None)


def test_default_route_still_refuses_33():
    ones = torch.ones
    for kw in ({}, {'route': 'lane'}):
        with pytest.raises(ValueError, match='1024'):
            mmpde5_batch([torch.zeros(2, 33, 33)], [(ones(32, 32), ones(33, 33))], **kw)


@pytest.mark.parametrize('N', STRIDED_EDGE_2D)
def test_strided_edge_cases_move_in_fifty_default_steps(N):
    """As test_mmpde5_host.test_edge_cases_move_in_fifty_default_steps: the fp64 restatement moves some node by at least 100
    spacings of fp32 at 1.0 (measured: 46 033 at N = 33, down to 12 690 at N = 81)."""
    z0, _ = edge_case(2, N)
    z, measure = edge_restated(2, N, torch.float64)
    moved = (z - z0.double()).abs().max().item() / 2.0 ** -23
    print(f"mmpde5 2d N={N}: moved by {moved:.0f} spacings")
    assert bool(torch.isfinite(z).all()) and measure > 0
    assert moved >= 100


def test_c_abi_checks_sizes_before_anything_is_launched():
    """The entry point refuses on the host copy of `desc`; the device pointers are never read (no device is needed)."""
    import ctypes as C
    lib = _native_mesh.lib()
    assert lib.gadapt_mesh_abi_version() == 2 and lib.gadapt_mmpde5_strided_max_side() == 81
    assert lib.gadapt_mmpde5_strided_lds_bytes(81 * 81) == 4 * (2 * 16 + 4 * 6561) == 105104
    assert lib.gadapt_mmpde5_strided_lds_bytes(82 * 82) == _native_mesh.E_SIZE
    ptr = C.c_void_p(8)                                                                     # non-null, never dereferenced

    def call(fn, dim, n):
        desc = (C.c_int32 * 4)(dim, n, 0, 0)
        rc = fn(1, C.cast(desc, C.c_void_p), ptr, ptr, ptr, ptr, ptr, ptr, 0.1, 1e-6, 10, ptr, ptr, ptr, ptr, ptr, None)
        return rc, lib.gadapt_mesh_last_error().decode()

    rc, msg = call(lib.gadapt_mmpde5_batch_strided, 2, 82)
    assert rc == _native_mesh.E_SIZE and '81' in msg
    rc, msg = call(lib.gadapt_mmpde5_batch_strided, 1, 1025)
    assert rc == _native_mesh.E_SIZE and '1024' in msg
    rc, msg = call(lib.gadapt_mmpde5_batch, 2, 33)                                          # the default route as before
    assert rc == _native_mesh.E_SIZE and '1024' in msg and '32' in msg
