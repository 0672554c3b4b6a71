"""Test-side restatement of the reference's 2-D modular loss (`firedrake_difFEM/difFEM_2d.py:374-535`), op by op in torch
(CPU, fp32 or fp64, autograd), on top of tests/fem_restatement.py: stiffness, load vector, phim, the nested Simpson rule,
u_true.  The yardstick of `gradient_meshpoints_2D` (g_adaptivity_amd/fem.py).

    direct_mse   F.mse_loss of the evaluation against u_true on linspace(0, 1, n_eval)^2, autograd through a dense solve
    direct_L2    torchquad's Simpson rule of (u_true - sol)^2 over [0,1]^2, autograd through a dense solve
    adjoint_L2   literally: a detached solve, grad1 = dL/dx with the coefficients held, lambda = solve(A^T, -dL/dc),
                 grad2 = d/dx lambda . (A c - RHS) with lambda and c held

The reference calls build_mass_matrix with three of its four arguments (a TypeError as shipped); the stiffness here is
the one torch_FEM_2D builds, its evident intent."""
from __future__ import annotations

import torch

import fem_restatement as R


def _system(coords, cells, boundary, centers, scales, n_load, boxes=None):
    cells = torch.as_tensor(cells, dtype=torch.long)
    A, _ = R.stiffness(coords, cells, boundary)
    rhs = R.load_vector(coords, cells, boundary, centers, scales, n=n_load, boxes=boxes)
    return A, rhs, cells


def expand(coeffs, pts, coords, cells):
    """soln (difFEM_2d.py:312-318): sum over every node m of c_m phim(., m)."""
    sol = pts[0] * 0.0
    for m in range(coords.shape[0]):
        sol = sol + coeffs[m] * R.phim(pts, m, coords, cells)
    return sol


def grid(n, dtype):
    q = torch.linspace(0, 1, n, dtype=dtype)
    X, Y = torch.meshgrid(q, q, indexing='ij')
    return torch.stack([X.reshape(-1), Y.reshape(-1)], 0)


def l2_error(coeffs, coords, cells, centers, scales, n):
    """cubature2d_v2 of (u_true - soln)^2 over [0,1]^2 (difFEM_2d.py:472-476)."""
    lo, hi = torch.zeros(2, dtype=coords.dtype), torch.ones(2, dtype=coords.dtype)
    return R.simpson(lambda p: (R.u_true(p, centers, scales) - expand(coeffs, p, coords, cells)) ** 2, lo, hi, n)


def direct_loss(kind, coords, cells, boundary, centers, scales, n_load, n_loss, boxes=None):
    """The loss of PDE_loss_direct_mse (kind 'mse', n_loss = eval_quad_points) or PDE_loss_direct_L2 (kind 'L2', n_loss
    = Simpson points per dimension), differentiable in coords."""
    A, rhs, cells = _system(coords, cells, boundary, centers, scales, n_load, boxes)
    c = torch.linalg.solve(A, rhs.unsqueeze(1)).squeeze(1)
    if kind == 'mse':
        pts = grid(n_loss, coords.dtype)
        return torch.nn.functional.mse_loss(expand(c, pts, coords, cells), R.u_true(pts, centers, scales))
    return l2_error(c, coords, cells, centers, scales, n_loss)


def direct(kind, coords, cells, boundary, centers, scales, n_load, n_loss):
    """(loss, d loss / d coords) of the direct types."""
    x = coords.detach().clone().requires_grad_(True)
    loss = direct_loss(kind, x, cells, boundary, centers, scales, n_load, n_loss)
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g


def adjoint_L2(coords, cells, boundary, centers, scales, n_load, n_loss):
    """(loss, grad1 + grad2) of PDE_loss_adjoint_L2 (difFEM_2d.py:482-535), step by step."""
    x = coords.detach().clone().requires_grad_(True)
    A, rhs, cells = _system(x, cells, boundary, centers, scales, n_load)
    with torch.no_grad():
        out = torch.linalg.solve(A, rhs.unsqueeze(1))                  # the reference's scipy solve
    outnew = out.detach().requires_grad_(True)
    loss = l2_error(outnew[:, 0], x, cells, centers, scales, n_loss)
    grad1 = torch.autograd.grad(loss, x, retain_graph=True)[0]
    outnew_grad = torch.autograd.grad(loss, outnew, retain_graph=True)[0]
    lambda1 = torch.linalg.solve(A.detach().t(), -outnew_grad)
    g = torch.matmul(A, out) - rhs.unsqueeze(1)
    final = torch.dot(lambda1.detach()[:, 0], g[:, 0])
    grad2 = torch.autograd.grad(final, x)[0]
    return loss.detach(), grad1 + grad2
