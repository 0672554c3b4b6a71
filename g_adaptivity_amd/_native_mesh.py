"""ctypes binding of `libgadapt_mesh.so`, the batched MMPDE5 and Monge-Ampere target-mesh generators (C-ABI in include/gadapt_mesh.h).

There is no CPU fallback: if the library is missing, or a call fails, this raises `NativeError`.
"""
from __future__ import annotations

import ctypes as C
import os

from ._native import NativeError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libgadapt_mesh.so')

ABI_VERSION = 2
MAX_NODES = 1024                                       # GADAPT_MMPDE5_MAX_NODES (route='lane'; 1-D on both routes)
STRIDED_MAX_SIDE = 81                                  # gadapt_mmpde5_strided_max_side(): 2-D, route='strided'
MAX_STEPS = 10000000                                   # GADAPT_MMPDE5_MAX_STEPS
DESC = 4                                               # GADAPT_MMPDE5_DESC: dim, N, node offset, cell offset
E_SIZE = -3                                            # GADAPT_MESH_E_SIZE
CONVERGED, CAP, STIFF = 0, 1, 2                        # GADAPT_MMPDE5_CONVERGED / _CAP / _STIFF
MA_MAX_SIDE = 32                                       # gadapt_ma_max_side(): Monge-Ampere meshes are 2-D, N <= 32 a side
MA_STRIDED_MAX_SIDE = 81                               # gadapt_ma_strided_max_side(): route='strided', fp64 potential
MA_M2N_SLOW_MAX_SIDE = 24                              # gadapt_ma_m2n_slow_max_side(): the band of the P1 solve stays in LDS
MA_MAX_GAUSS = 8                                       # gadapt_ma_max_gauss()
MA_DESC = 4                                            # GADAPT_MA_DESC: N, node offset, Gaussian offset, Gaussian count
MA_TABLE_MAX_SIDE = 1024                               # gadapt_ma_table_max_side(): 2 <= T <= 1024 a side of a tabulated monitor
MA_CONVERGED, MA_CAP, MA_NONCONVEX = 0, 1, 2           # GADAPT_MA_CONVERGED / _CAP / _NONCONVEX

_P, _I, _L, _D = C.c_void_p, C.c_int, C.c_int64, C.c_double

# name -> (restype, argtypes); must list every symbol include/gadapt_mesh.h declares
PROTOTYPES = {
    'gadapt_mesh_abi_version': (_I, []),
    'gadapt_mesh_last_error': (C.c_char_p, []),
    'gadapt_mmpde5_max_nodes': (_I, []),
    'gadapt_mmpde5_max_steps': (_I, []),
    'gadapt_mmpde5_threads': (_I, [_I]),
    'gadapt_mmpde5_lds_bytes': (_L, [_I]),
    'gadapt_mmpde5_batch': (_I, [_I] + [_P] * 7 + [_D, _D, _I] + [_P] * 6),
    'gadapt_mmpde5_strided_max_side': (_I, []),
    'gadapt_mmpde5_strided_lds_bytes': (_L, [_I]),
    'gadapt_mmpde5_batch_strided': (_I, [_I] + [_P] * 7 + [_D, _D, _I] + [_P] * 6),
    'gadapt_ma_max_side': (_I, []),
    'gadapt_ma_max_gauss': (_I, []),
    'gadapt_ma_lds_bytes': (_L, [_I]),
    'gadapt_ma_batch': (_I, [_I] + [_P] * 4 + [_D, _D, _I] + [_P] * 6),
    'gadapt_ma_strided_max_side': (_I, []),
    'gadapt_ma_strided_lds_bytes': (_L, [_I]),
    'gadapt_ma_batch_strided': (_I, [_I] + [_P] * 4 + [_D, _D, _I] + [_P] * 6),
    'gadapt_ma_m2n_lds_bytes': (_L, [_I]),
    'gadapt_ma_m2n_strided_lds_bytes': (_L, [_I]),
    'gadapt_ma_m2n_batch': (_I, [_I] + [_P] * 4 + [_D, _D, _I] + [_P] * 6),
    'gadapt_ma_m2n_batch_strided': (_I, [_I] + [_P] * 4 + [_D, _D, _I] + [_P] * 6),
    'gadapt_ma_m2n_slow_max_side': (_I, []),
    'gadapt_ma_m2n_slow_lds_bytes': (_L, [_I]),
    'gadapt_ma_m2n_slow_batch': (_I, [_I] + [_P] * 4 + [_D, _D, _I] + [_P] * 7),
    'gadapt_ma_table_max_side': (_I, []),
    'gadapt_ma_table_batch': (_I, [_I] + [_P] * 3 + [_D, _D, _I] + [_P] * 6),
    'gadapt_ma_table_batch_strided': (_I, [_I] + [_P] * 3 + [_D, _D, _I] + [_P] * 6),
}

# (getters, expected values, the message's wording with the values got and then those expected)
LIMITS = [
    (('gadapt_mmpde5_strided_max_side',), (STRIDED_MAX_SIDE,), "strided route up to {} a side, expected {}"),
    (('gadapt_ma_max_side', 'gadapt_ma_max_gauss'), (MA_MAX_SIDE, MA_MAX_GAUSS),
     "Monge-Ampere limits {} a side / {} Gaussians, expected {} / {}; rebuild it with `make`"),
    (('gadapt_ma_strided_max_side',), (MA_STRIDED_MAX_SIDE,),
     "strided Monge-Ampere route up to {} a side, expected {}; rebuild it with `make`"),
    (('gadapt_ma_m2n_slow_max_side',), (MA_M2N_SLOW_MAX_SIDE,), "M2N 'slow' monitor up to {} a side, expected {}; rebuild it with `make`"),
    (('gadapt_ma_table_max_side',), (MA_TABLE_MAX_SIDE,), "tabulated monitors up to {} a side, expected {}; rebuild it with `make`"),
]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(f"{LIB_PATH} not found: build it with `make` (hipcc --offload-arch=gfx950); "
                              "there is no CPU fallback for the MMPDE5 generator")
        handle = C.CDLL(LIB_PATH)
        handle.gadapt_mesh_abi_version.restype = _I                    # first: a stale library lacks the newer symbols
        if handle.gadapt_mesh_abi_version() != ABI_VERSION:
            raise NativeError(f"{LIB_PATH}: ABI {handle.gadapt_mesh_abi_version()}, expected {ABI_VERSION}; rebuild it with `make`")
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(handle, name, None)
            if fn is None:                                             # same ABI number, older build: the ABI grows by addition
                raise NativeError(f"{LIB_PATH} lacks {name}: a stale build; rebuild it with `make`")
            fn.restype, fn.argtypes = res, args
        for got, want, text in LIMITS:                                 # the limits this module states are the library's
            got = tuple(getattr(handle, g)() for g in got)
            if got != want:
                raise NativeError(f"{LIB_PATH}: " + text.format(*got, *want))
        _lib = handle
    return _lib


def check(rc: int, what: str):
    """Size errors are the caller's (`ValueError`), everything else a native failure."""
    if rc < 0:
        msg = lib().gadapt_mesh_last_error().decode() or f"error {rc}"
        raise (ValueError if rc == E_SIZE else NativeError)(f"{what}: {msg} (code {rc})")
