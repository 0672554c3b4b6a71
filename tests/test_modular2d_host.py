"""CPU checks of the 2-D modular loss: gradient_meshpoints_2D's argument checks, torchquad's points-per-dimension rule, and
the test-side restatement (tests/modular2d_restatement.py) pinned from independent sides."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fem_restatement as R  # noqa: E402
import modular2d_restatement as M  # noqa: E402

from g_adaptivity_amd import gradient_meshpoints_2D  # noqa: E402
from g_adaptivity_amd.fem import GRAD_TYPES_2D, simpson_points_per_dim  # noqa: E402
from g_adaptivity_amd.mesh_graph import MeshData, square_mesh  # noqa: E402

CENTERS = [np.array([0.4, 0.55], np.float32), np.array([0.7, 0.3], np.float32)]
SCALES = [np.array([0.3, 0.25], np.float32), np.array([0.2, 0.35], np.float32)]


def _mesh(n, jitter=0.0, seed=0, dtype=torch.float64):
    m = square_mesh(n)
    x = m.x_comp.to(dtype).clone()
    if jitter:
        g = torch.Generator().manual_seed(seed)
        d = (torch.rand(x.shape, generator=g, dtype=dtype) * 2 - 1) * jitter / (n - 1)
        d[m.boundary_nodes] = 0.0
        x = x + d
    return x, m.cells, m.boundary_nodes


def test_grad_type_missing_or_unknown_raises():
    d = MeshData(pde_params={'centers': CENTERS, 'scales': SCALES})
    x = square_mesh(5).x_comp
    with pytest.raises(ValueError, match="not specified"):
        gradient_meshpoints_2D({'mesh_dims': [5, 5]}, d, x)
    with pytest.raises(ValueError, match="incorrectly specified"):
        gradient_meshpoints_2D({'mesh_dims': [5, 5], 'grad_type': 'PDE_loss_adjoint_mse'}, d, x)
    assert GRAD_TYPES_2D == ('PDE_loss_direct_mse', 'PDE_loss_direct_L2', 'PDE_loss_adjoint_L2')


def test_one_dimensional_x_phys_raises():
    d = MeshData(pde_params={'centers': CENTERS, 'scales': SCALES})
    with pytest.raises(NotImplementedError, match=r'\[N,2\]'):
        gradient_meshpoints_2D({'mesh_dims': [5], 'grad_type': 'PDE_loss_direct_mse'}, d, torch.linspace(0, 1, 5))


def test_points_per_dimension():
    assert simpson_points_per_dim(101) == 9 == R.SIMPSON_N
    assert [simpson_points_per_dim(n) for n in (49, 51, 81, 99, 121, 10201)] == [7, 7, 9, 9, 11, 101]


def test_adjoint_equals_direct_L2_fp64():
    x, cells, bnd = _mesh(7, jitter=0.3, seed=4)
    l_d, g_d = M.direct('L2', x, cells, bnd, CENTERS, SCALES, R.SIMPSON_N, R.SIMPSON_N)
    l_a, g_a = M.adjoint_L2(x, cells, bnd, CENTERS, SCALES, R.SIMPSON_N, R.SIMPSON_N)
    assert abs(l_a.item() - l_d.item()) <= 1e-12 * abs(l_d.item())
    assert g_d.abs().max().item() > 0
    assert ((g_a - g_d).abs().max() / g_d.abs().max()).item() <= 1e-10


def test_gradcheck_direct_L2_fp64():
    x, cells, bnd = _mesh(5, jitter=0.3, seed=3)
    inner = (~bnd).nonzero().reshape(-1)
    # boxes widened by 1e-3 (a box corner is a vertex where one vertex is extremal in x and y, and phim has a kink there)
    # and held: the reference detaches them (difFEM_2d.py:298-309) and the boundary values u_true(x_B) (:172)
    boxes = [(lo - 1e-3, hi + 1e-3) for lo, hi in R.simpson_boxes(x, cells)]

    def f(xi):
        return M.direct_loss('L2', x.index_put((inner,), xi), cells, bnd, CENTERS, SCALES, R.SIMPSON_N, R.SIMPSON_N, boxes=boxes)
    assert torch.autograd.gradcheck(f, (x[inner].clone().requires_grad_(True),), eps=1e-7, atol=1e-6, rtol=1e-4)
