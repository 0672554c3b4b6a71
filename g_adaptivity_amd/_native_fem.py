"""ctypes binding of `libgadapt_fem.so`, the FEM tails (2-D pde_loss, 1-D Burgers / Poisson; C-ABI in include/gadapt_fem.h).

There is no CPU fallback: if the library is missing, or a call fails, this raises `NativeError`.
"""
from __future__ import annotations

import ctypes as C
import os

from ._native import NativeError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libgadapt_fem.so')

ABI_VERSION = 4
META = 8                                   # GADAPT_FEM_META
M_N_INT, M_BAND = 5, 6                     # GADAPT_FEM_M_N_INT, GADAPT_FEM_M_BAND
LOSS_MSE, LOSS_SIMPSON = 0, 1              # GADAPT_FEM_LOSS_MSE, GADAPT_FEM_LOSS_SIMPSON

_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_int64, C.c_float

# name -> (restype, argtypes); must list every symbol include/gadapt_fem.h declares
PROTOTYPES = {
    'gadapt_fem_abi_version': (_I, []),
    'gadapt_fem_last_error': (C.c_char_p, []),
    'gadapt_fem_simpson_points': (_I, []),
    'gadapt_fem_lds_budget': (_I, []),
    'gadapt_fem_topology_host': (_L, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'gadapt_fem_factor_lds_bytes': (_L, [_I, _I]),
    'gadapt_fem_eval_lds_bytes': (_L, [_I]),
    'gadapt_fem_forward': (_I, [_I, _I, _I] + [_P] * 12 + [_I, _I, _I] + [_P] * 5),
    'gadapt_fem_eval_partials_floats': (_I, [_I]),
    'gadapt_fem_eval_errors': (_I, [_I, _I, _I] + [_P] * 12 + [_I, _I, _I] + [_P] * 6),
    'gadapt_fem_window_lds_bytes': (_L, [_I, _I]),
    'gadapt_fem_window_workspace_floats': (_L, [_I, _P]),
    'gadapt_fem_eval_errors_window': (_I, [_I, _I, _I] + [_P] * 12 + [_I, _I, _I] + [_P] * 3 + [_I] + [_P] * 3),
    'gadapt_fem_modular_forward': (_I, [_I, _I, _I] + [_P] * 12 + [_I, _I, _I, _I] + [_P] * 7),
    'gadapt_fem_backward': (_I, [_I, _I, _I] + [_P] * 13 + [_I, _I] + [_P] * 9),
    'gadapt_fem_forward_window': (_I, [_I, _I, _I] + [_P] * 12 + [_I, _I, _I] + [_P] * 3 + [_I] + [_P] * 2),
    'gadapt_fem_modular_forward_window': (_I, [_I, _I, _I] + [_P] * 12 + [_I, _I, _I, _I] + [_P] * 3 + [_I] + [_P] * 4),
    'gadapt_fem_backward_window': (_I, [_I, _I, _I] + [_P] * 13 + [_I, _I] + [_P] * 9),
    'gadapt_fem_backward_wave': (_I, [_I, _I, _I] + [_P] * 13 + [_I, _I] + [_P] * 9),
    'gadapt_fem_backward_window_wave': (_I, [_I, _I, _I] + [_P] * 13 + [_I, _I] + [_P] * 9),
    'gadapt_fem_forward_wave': (_I, [_I, _I, _I] + [_P] * 12 + [_I, _I, _I] + [_P] * 5),
    'gadapt_fem_modular_forward_wave': (_I, [_I, _I, _I] + [_P] * 12 + [_I, _I, _I, _I] + [_P] * 7),
    'gadapt_fem_eval_errors_wave': (_I, [_I, _I, _I] + [_P] * 12 + [_I, _I, _I] + [_P] * 7),
    'gadapt_fem1d_lds_bytes': (_L, [_I, _I]),
    'gadapt_fem1d_burgers_forward': (_I, [_I, _I] + [_P] * 6 + [_F] * 3 + [_I] * 7 + [_P] * 6),
    'gadapt_fem1d_burgers_backward': (_I, [_I, _I, _P, _P, _P, _F, _F, _I, _I, _I, _I] + [_P] * 7),
    'gadapt_fem1d_poisson_forward': (_I, [_I, _I] + [_P] * 4 + [_I] * 3 + [_P] * 5),
    'gadapt_fem1d_poisson_eval_errors': (_I, [_I, _I] + [_P] * 4 + [_I] * 3 + [_P] * 4),
    'gadapt_fem1d_poisson_backward': (_I, [_I, _I] + [_P] * 4 + [_I] * 3 + [_P] * 6),
    'gadapt_fem_poisson1d_loss_lds_bytes': (_L, [_I, _I]),
    'gadapt_fem_poisson1d_loss': (_I, [_I, _I] + [_P] * 4 + [_I] * 3 + [_P, _P, _I] + [_P] * 8),
    'gadapt_fem1d_expand': (_I, [_I, _I, _P, _P, _P, _I, _P, _P, _P]),
    'gadapt_fem1d_spline': (_I, [_I, _I, _P, _P, _P, _I, _P, _P, _I, _P, _P, _P]),
    'gadapt_fem_descend': (_I, [_I, _I, _I] + [_P] * 14 + [_I, _I, _I, _I, _F] + [_P] * 16),
    'gadapt_fem_descend_wave': (_I, [_I, _I, _I] + [_P] * 14 + [_I, _I, _I, _I, _F] + [_P] * 15 + [_I, _P]),
    'gadapt_fem1d_descend': (_I, [_I, _I] + [_P] * 4 + [_I] * 3 + [_P, _I, _F, _I, _I] + [_P] * 11),
}
DESCEND_INTERNAL, DESCEND_ALL = 0, 1       # GADAPT_FEM1D_DESCEND_*
ROUTE_WAVE_FORWARD, ROUTE_WAVE_ADJOINT = 1, 2   # GADAPT_FEM_ROUTE_WAVE_*
FEM1D_LOSS_L1, FEM1D_LOSS_MSE = 0, 1       # GADAPT_FEM1D_LOSS_*
SPLINE_OK, SPLINE_NOT_INCREASING, SPLINE_NOT_FINITE, SPLINE_BAD_COUNT = 0, 1, 2, 3   # GADAPT_SPLINE_S_*

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(f"{LIB_PATH} not found: build it with `make` (hipcc --offload-arch=gfx950); "
                              "there is no CPU fallback for the FEM tail")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        if handle.gadapt_fem_abi_version() != ABI_VERSION:
            raise NativeError(f"{LIB_PATH}: ABI {handle.gadapt_fem_abi_version()}, expected {ABI_VERSION}")
        _lib = handle
    return _lib


def check(rc: int, what: str):
    if rc < 0:
        msg = lib().gadapt_fem_last_error().decode() or f"error {rc}"
        raise NativeError(f"{what}: {msg} (code {rc})")


def call(name: str, *args):
    """lib().<name>(*args), raising NativeError with the library's message when it returns an error code."""
    check(getattr(lib(), name)(*args), name)
