"""CPU restatement of the reference's MMPDE5 iteration (classical_meshing/ma_mesh_1d.py, ma_mesh_2d.py), written from its
description: the tests' yardstick for g_adaptivity_amd.mmpde5, in fp32 (the reference's own arithmetic, operation by
operation) and in fp64.

    state     X [N] or (X, Y) [N, N] ('ij' order); boundary rows and columns never move
    monitor   constant arrays: ms at the cell centres ((N-1)^d), m2 at the nodes (N^d)
    rhs       1-D: (ms[i] (X[i+1] - X[i]) - ms[i-1] (X[i] - X[i-1])) / dxi^2 / tau / m2[i]
              2-D: the same along each index direction with ms[i, j] for both forward differences and
                   ms[i-1, j] / ms[i, j-1] for the backward ones, summed; X and Y independently
    step      classical RK4, h = cfl / N^3
    loop      while j < max_steps and measure > tol: j += 1; step; measure = sum |new - old|; break if measure > 1 / tol
"""
import torch


def rhs(Z, ms, m2, tau=0.1):
    """Z [N] or [2, N, N] -> the right-hand side, zero on the boundary.  Three divisions in the reference's order."""
    n = Z.shape[-1]
    d = torch.linspace(0, 1, n, dtype=Z.dtype)[1]
    A = torch.zeros_like(Z)
    if Z.dim() == 1:
        A[1:n - 1] = (ms[1:n - 1] * (Z[2:n] - Z[1:n - 1]) - ms[0:n - 2] * (Z[1:n - 1] - Z[0:n - 2])) / d ** 2 / tau / m2[1:n - 1]
        return A
    here, west, south, den = ms[1:n - 1, 1:n - 1], ms[0:n - 2, 1:n - 1], ms[1:n - 1, 0:n - 2], m2[1:n - 1, 1:n - 1]
    for k in range(2):
        U = Z[k]
        c = U[1:n - 1, 1:n - 1]
        a1 = (here * (U[2:n, 1:n - 1] - c) - west * (c - U[0:n - 2, 1:n - 1])) / d ** 2 / tau / den
        a2 = (here * (U[1:n - 1, 2:n] - c) - south * (c - U[1:n - 1, 0:n - 2])) / d ** 2 / tau / den
        A[k, 1:n - 1, 1:n - 1] = a1 + a2
    return A


def rk4(Z, f, h):
    k1 = f(Z)
    k2 = f(Z + h * k1 / 2)
    k3 = f(Z + h * k2 / 2)
    k4 = f(Z + h * k3)
    return Z + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)


def mmpde5(Z0, ms, m2, dtype=torch.float32, cfl=0.05, step=None, tol=1e-6, max_steps=10000, tau=0.1):
    """Z0 [N] or [2, N, N], monitor arrays as above -> (Z, j, measure).  tol = 0: exactly max_steps steps."""
    Z, ms, m2 = (torch.as_tensor(a).to(dtype) for a in (Z0, ms, m2))
    n = Z.shape[-1]
    h = cfl / n ** 3 if step is None else step
    j, measure = 0, 1.0
    while j < max_steps and (tol == 0 or measure > tol):
        j += 1
        Zn = rk4(Z, lambda z: rhs(z, ms, m2, tau), h)
        moved = (Zn - Z).abs()
        measure = float(moved.sum() if Z.dim() == 1 else (moved[0] + moved[1]).sum())
        Z = Zn
        if tol > 0 and measure > 1.0 / tol:
            break
    return Z, j, measure
