"""Test-side yardstick of the Poisson error-reduction evaluation (g_adaptivity_amd/evaluation.py): the solve and expansion of
`fem_restatement.fem2d` / `fem1d_restatement.poisson`, then the reference's trapezium norms (`src/utils_eval.py:32-65`)
restated in torch in the dtype of the solve, and its percentage reduction (`:68-73`).

Orientation: `fem2d` returns sol row-major in meshgrid 'ij' (index i*n + j <-> (x_i, y_j)); the reference's
np.meshgrid(x, y) is 'xy'.  Each lattice cell gives dx dy / 4 of its four corner values either way, so on the lattice the
norms are the same sums in another order; here they are written in 'ij'."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fem1d_restatement as R1  # noqa: E402
import fem_restatement as R2  # noqa: E402


def lattice(n_eval, dtype):
    """np.linspace(0, 1, n) as the reference builds it, in the dtype of the solve."""
    return torch.from_numpy(np.linspace(0, 1, n_eval)).to(dtype)


def trapezium_1d(uu, u_true, x):
    dx = x[1:] - x[:-1]
    e = uu - u_true
    l2 = (e ** 2)[1:] + (e ** 2)[:-1]
    l1 = e.abs()[1:] + e.abs()[:-1]
    return (l1 * dx).sum() / 2, torch.sqrt((l2 * dx).sum() / 2)


def trapezium_2d(uu, u_true, ax):
    """uu, u_true [n*n] in 'ij' order on the axis ax [n] (both dimensions)."""
    n = ax.numel()
    e = (uu - u_true).reshape(n, n)
    d = ax[1:] - ax[:-1]
    w = d[:, None] * d[None, :]                                   # dx_i dy_j of cell (i, j)
    sq, ab = e ** 2, e.abs()
    l2 = sq[:-1, 1:] + sq[1:, :-1] + sq[1:, 1:] + sq[:-1, :-1]
    l1 = ab[:-1, 1:] + ab[1:, :-1] + ab[1:, 1:] + ab[:-1, :-1]
    return (l1 * w).sum() / 4, torch.sqrt((l2 * w).sum() / 4)


def errors_2d(coords, cells, boundary, centers, scales, n_eval, dtype):
    """(L1, L2) as Python floats of one 2-D mesh, every operation in `dtype`."""
    ax = lattice(n_eval, dtype)
    _, sol = R2.fem2d(coords.to(dtype), cells, boundary, centers, scales, ax)
    X, Y = torch.meshgrid(ax, ax, indexing='ij')
    u = R2.u_true(torch.stack([X.reshape(-1), Y.reshape(-1)], 0), centers, scales)
    l1, l2 = trapezium_2d(sol, u, ax)
    return float(l1), float(l2)


def errors_1d(mesh, centers, scales, opt, n_eval, dtype):
    """(L1, L2) as Python floats of one 1-D mesh; centers / scales as 1-element arrays."""
    ax = lattice(n_eval, dtype)
    cs = [torch.tensor(float(np.asarray(c).reshape(-1)[0]), dtype=dtype) for c in centers]
    ss = [torch.tensor(float(np.asarray(s).reshape(-1)[0]), dtype=dtype) for s in scales]
    o = {'stiff_quad_points': int(opt.get('stiff_quad_points', 3)), 'load_quad_points': int(opt.get('load_quad_points', 101))}
    _, sol = R1.poisson(mesh.to(dtype).reshape(-1), cs, ss, o, ax)
    l1, l2 = trapezium_1d(sol, R1.gauss(ax, cs, ss), ax)
    return float(l1), float(l2)


def reduction(e_initial, e_adapted):
    return None if e_adapted == 0. else (e_adapted - e_initial) / e_initial * 100


def rel(a, b):
    return abs(a - b) / abs(b)
