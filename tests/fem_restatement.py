"""Test-side restatement of the reference's differentiable P1 FEM (`firedrake_difFEM/difFEM_2d.py:16-372`), op by op in
torch (CPU, fp32 or fp64, autograd).  The yardstick of the pde_loss FEM tail (g_adaptivity_amd/fem.py): stiffness by
batched `linalg.solve` of [1 x y], load vector by the nested Simpson rule on detached bounding boxes, dense solve, evaluation
by summing c_m phim(., m) over every node."""
from __future__ import annotations

import numpy as np
import torch

# Points per dimension of torchquad's Simpson().integrate(N=101, dim=2): floor(101^(1/2)) = 10, lowered to the odd 9
# (the constant the kernels use, include/gadapt_fem.h GADAPT_FEM_SIMPSON_N)
SIMPSON_N = 9


def _checks(x, a, b):
    lhs = (a[1] - b[1]) * x[0] + (b[0] - a[0]) * x[1]
    rhs = (a[1] - b[1]) * a[0] + (b[0] - a[0]) * a[1]
    return (lhs >= rhs).to(x.dtype), (lhs <= rhs).to(x.dtype)


def aux(x, a, b, c):
    l1, r1 = _checks(x, a, b)
    l2, r2 = _checks(x, b, c)
    l3, r3 = _checks(x, c, a)
    q = ((x[0] - c[0]) * (a[1] - b[1]) + (x[1] - c[1]) * (b[0] - a[0])) / ((a[1] - b[1]) * (c[0] - a[0]) + (c[1] - a[1]) * (b[0] - a[0]))
    return (l1 * l2 * l3 + r1 * r2 * r3) * (1 + q)


def phim(x, m, coords, cells):
    rows, locs = torch.where(cells == m)
    out = x[0] * 0.0
    rep = x[0] * 0.0
    for t, l in zip(rows.tolist(), locs.tolist()):
        c = coords[cells[t, l]]
        a = coords[cells[t, (l + 2) % 3]]
        b = coords[cells[t, (l + 1) % 3]]
        inc = aux(x, a, b, c)
        out = out + inc
        rep = rep + (inc > 0.0).to(x.dtype)
    return out / (rep + (rep == 0.0).to(x.dtype))


def forcing(x, centers, scales):
    sol = torch.zeros(x[0].shape, dtype=x.dtype)
    for c, s in zip(centers, scales):
        c0, c1, s0, s1 = (torch.tensor(float(v), dtype=x.dtype) for v in (c[0], c[1], s[0], s[1]))
        sol = sol + (1 / (s0 ** 4 * s1 ** 4)) * torch.exp(-((c0 - x[0]) ** 2 / s0 ** 2) - (c1 - x[1]) ** 2 / s1 ** 2) * (
            4 * c1 ** 2 * s0 ** 4 - 2 * s0 ** 2 * s1 ** 4 + 4 * s1 ** 4 * (c0 - x[0]) ** 2 - 8 * c1 * s0 ** 4 * x[1]
            - 2 * s0 ** 4 * (s1 ** 2 - 2 * x[1] ** 2))
    return sol


def u_true(x, centers, scales):
    sol = torch.zeros(x[0].shape, dtype=x.dtype)
    for c, s in zip(centers, scales):
        c0, c1, s0, s1 = (torch.tensor(float(v), dtype=x.dtype) for v in (c[0], c[1], s[0], s[1]))
        sol = sol + torch.exp(-(x[0] - c0) ** 2 / s0 ** 2 - (x[1] - c1) ** 2 / s1 ** 2)
    return sol


def simpson(integrand, lo, hi, n=SIMPSON_N):
    """torchquad's Simpson in 2-D: linspace per dimension, meshgrid 'ij', the composite rule on the last dimension first."""
    gx = torch.linspace(float(lo[0]), float(hi[0]), n, dtype=lo.dtype)
    gy = torch.linspace(float(lo[1]), float(hi[1]), n, dtype=lo.dtype)
    X, Y = torch.meshgrid(gx, gy, indexing='ij')
    f = integrand(torch.stack([X.reshape(-1), Y.reshape(-1)], 0)).reshape(n, n)
    hx, hy = (hi[0] - lo[0]) / (n - 1), (hi[1] - lo[1]) / (n - 1)
    f = (hy / 3.0 * (f[:, 0:-2][:, ::2] + 4 * f[:, 1:-1][:, ::2] + f[:, 2:][:, ::2])).sum(1)
    return (hx / 3.0 * (f[0:-2][::2] + 4 * f[1:-1][::2] + f[2:][::2])).sum(0)


def stiffness(coords, cells, boundary):
    tri = coords[cells]                                                  # [T,3,2]
    T = tri.shape[0]
    M = torch.cat([torch.ones(T, 3, 1, dtype=coords.dtype), tri], 2)
    slopes = torch.linalg.solve(M, torch.eye(3, dtype=coords.dtype).repeat(T, 1, 1))
    x, y = tri[:, :, 0], tri[:, :, 1]
    area = 0.5 * torch.abs(x[:, 0] * (y[:, 1] - y[:, 2]) + x[:, 1] * (y[:, 2] - y[:, 0]) + x[:, 2] * (y[:, 0] - y[:, 1]))
    N = coords.shape[0]
    A = torch.zeros(N, N, dtype=coords.dtype)
    for i in range(3):
        for j in range(3):
            v = (slopes[:, 1:, i] * slopes[:, 1:, j] * area.unsqueeze(1)).sum(1)
            A = A.index_put((cells[:, i], cells[:, j]), v, accumulate=True)
    A = -A
    bnd = torch.as_tensor(boundary).nonzero().reshape(-1)
    A = A.clone()
    A[bnd, :] = 0.0
    A[bnd, bnd] = 1.0
    return A, area


def simpson_boxes(coords, cells):
    """Bounding box of the vertices of each node's incident triangles, from detached coordinates (difFEM_2d.py:298-309)."""
    boxes = []
    for m in range(coords.shape[0]):
        box = coords[cells[torch.where(cells == m)[0], :].reshape(-1)].detach()
        boxes.append((box.min(0)[0], box.max(0)[0]))
    return boxes


def load_vector(coords, cells, boundary, centers, scales, n=SIMPSON_N, boxes=None):
    N = coords.shape[0]
    boxes = simpson_boxes(coords, cells) if boxes is None else boxes
    rows = []
    for m in range(N):
        if bool(boundary[m]):
            rows.append(u_true(coords[m].detach(), centers, scales).reshape(()))
        else:
            lo, hi = boxes[m]
            rows.append(simpson(lambda p: phim(p, m, coords, cells) * forcing(p, centers, scales), lo, hi, n))
    return torch.stack(rows)


def fem2d(coords, cells, boundary, centers, scales, lattice, boxes=None):
    """(coeffs [N], sol [nlat*nlat]); lattice is the 1-D axis of the square evaluation grid (meshgrid 'ij', row-major).
    `boxes` fixes the (detached) Simpson boxes, e.g. for a finite-difference check of the gradient the reference defines."""
    cells = torch.as_tensor(cells, dtype=torch.long)
    A, _ = stiffness(coords, cells, boundary)
    rhs = load_vector(coords, cells, boundary, centers, scales, boxes=boxes)
    coeffs = torch.linalg.solve(A, rhs.unsqueeze(1)).squeeze(1)
    X, Y = torch.meshgrid(lattice, lattice, indexing='ij')
    pts = torch.stack([X.reshape(-1), Y.reshape(-1)], 0).to(coords.dtype)
    sol = pts[0] * 0.0
    for m in range(coords.shape[0]):
        sol = sol + coeffs[m] * phim(pts, m, coords, cells)
    return coeffs, sol
