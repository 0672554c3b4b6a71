"""Test-side restatement of the not-a-knot interpolating cubic spline (scipy's UnivariateSpline(x, y, s=0) and
CubicSpline(bc_type='not-a-knot')), written from its definition in torch, any dtype; nothing from scipy inside.

The spline is the C2 piecewise cubic through all points whose third derivative is continuous at x[1] and x[n-2].  With M the
second derivatives at the points, the full n x n system (solved densely here) is

    row 0      h[1] M[0] - (h[0] + h[1]) M[1] + h[0] M[2] = 0                        (s''' continuous at x[1])
    row i      h[i-1] M[i-1] + 2 (h[i-1] + h[i]) M[i] + h[i] M[i+1] = 6 (d[i] - d[i-1]),   d[i] = (y[i+1] - y[i]) / h[i]
    row n-1    h[n-2] M[n-3] - (h[n-3] + h[n-2]) M[n-2] + h[n-3] M[n-1] = 0          (s''' continuous at x[n-2])

and on [x[i], x[i+1]], t = q - x[i]:  s = y[i] + c1 t + M[i]/2 t^2 + (M[i+1] - M[i]) / (6 h[i]) t^3,
c1 = d[i] - h[i] (2 M[i] + M[i+1]) / 6.  Queries outside the data use the end pieces.
"""
import torch


def second_derivatives(x, y, dtype=torch.float64):
    x, y = torch.as_tensor(x).to(dtype), torch.as_tensor(y).to(dtype)
    n = x.shape[0]
    h = x[1:] - x[:-1]
    d = (y[1:] - y[:-1]) / h
    A = torch.zeros(n, n, dtype=dtype)
    r = torch.zeros(n, dtype=dtype)
    A[0, 0], A[0, 1], A[0, 2] = h[1], -(h[0] + h[1]), h[0]
    A[n - 1, n - 3], A[n - 1, n - 2], A[n - 1, n - 1] = h[n - 2], -(h[n - 3] + h[n - 2]), h[n - 3]
    for i in range(1, n - 1):
        A[i, i - 1], A[i, i], A[i, i + 1] = h[i - 1], 2 * (h[i - 1] + h[i]), h[i]
        r[i] = 6 * (d[i] - d[i - 1])
    return torch.linalg.solve(A, r)


def spline(x, y, q, deriv=0, dtype=torch.float64, M=None):
    """Values (deriv 0) or derivatives (1, 2) at q of the not-a-knot spline through (x, y), all arithmetic in dtype.
    M: second_derivatives(x, y, dtype) where the caller has them already."""
    x, y, q = (torch.as_tensor(a).to(dtype) for a in (x, y, q))
    n = x.shape[0]
    M = second_derivatives(x, y, dtype) if M is None else M
    i = torch.clamp(torch.searchsorted(x, q.contiguous(), right=True) - 1, 0, n - 2)      # last x[i] <= q, end pieces outside
    h = x[i + 1] - x[i]
    t = q - x[i]
    c3 = (M[i + 1] - M[i]) / (6 * h)
    c1 = (y[i + 1] - y[i]) / h - h * (2 * M[i] + M[i + 1]) / 6
    if deriv == 0:
        return y[i] + t * (c1 + t * (M[i] / 2 + t * c3))
    if deriv == 1:
        return c1 + t * (M[i] + t * 3 * c3)
    if deriv == 2:
        return M[i] + t * 6 * c3
    raise ValueError(deriv)
