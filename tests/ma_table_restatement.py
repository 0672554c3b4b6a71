"""The Monge-Ampere iteration with a TABULATED monitor (include/gadapt_mesh.h, gadapt_ma_table_batch and
gadapt_ma_table_batch_strided) restated in torch, in three arithmetics:

  'fp64'   everything in fp64: the yardstick
  'fp32'   everything in fp32: the lane route's arithmetic
  'mixed'  phi and the five stencil expressions in fp64, each rounded once to fp32, everything after that in fp32, the increment
           formed in fp32 and added in fp64: the strided route's arithmetic

The iteration is `ma_restatement`'s (and `ma_strided_restatement`'s) with the monitor swapped: no Gaussians, no pow, but the
header's bilinear read of the table M [T, T], M[i, j] at the physical point (i / (T-1), j / (T-1)), operation for operation
(`table_monitor`).  The table is rounded to fp32 first in every arithmetic: it is the same data the kernel gets.  Only the order of
the sum behind the trapezium mean differs from the kernels' (torch's).

`ma(..., perturb=seed)` multiplies the monitor per node and per evaluation by 1 + 2^-23 or 1 - 2^-23, drawn from that seed: the
price of a logf, or of an interpolation, that rounds the other way, measured, not guessed.

`grid`, `cell_spread`, `uniform_spread` and `triangles_keep_orientation` are `ma_restatement`'s.
"""
import torch
import torch.nn.functional as F

import ma_restatement as R

CONVERGED, CAP, NONCONVEX = R.CONVERGED, R.CAP, R.NONCONVEX
grid, cell_spread, uniform_spread, triangles_keep_orientation = R.grid, R.cell_spread, R.uniform_spread, R.triangles_keep_orientation
ARITHMETICS = ('fp64', 'fp32', 'mixed')


def table_in(table, dtype):
    """The table as the kernel receives it (fp32), carried in `dtype`."""
    return table.detach().to(torch.float32).to(dtype)


def table_monitor(x, y, M):
    """m of the header at the points (x, y), in their dtype; M [T, T] in the same dtype."""
    T = M.shape[0]
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    xc = torch.where(x > 0, torch.where(x < 1, x, one), zero)              # a NaN maps to 0
    yc = torch.where(y > 0, torch.where(y < 1, y, one), zero)
    fx, fy = xc * float(T - 1), yc * float(T - 1)
    i0, j0 = torch.clamp(fx.to(torch.int64), max=T - 2), torch.clamp(fy.to(torch.int64), max=T - 2)
    ax, ay = fx - i0.to(x.dtype), fy - j0.to(x.dtype)
    m00, m10, m01, m11 = M[i0, j0], M[i0 + 1, j0], M[i0, j0 + 1], M[i0 + 1, j0 + 1]
    m0 = m00 + ax * (m10 - m00)
    m1 = m01 + ax * (m11 - m01)
    return m0 + ay * (m1 - m0)


def evaluate(phi, N, gx, gy, M, flip=None):
    """(x, y, r, lambda) of the potential phi [N, N]: in the dtype of gx (phi's own on 'fp64' and 'fp32'; fp32 from an fp64 phi on
    'mixed', where the five stencil expressions are rounded once)."""
    n1 = float(N - 1)
    inv2h, invh2, inv4h2 = 0.5 * n1, n1 * n1, 0.25 * n1 * n1
    p = F.pad(phi[None, None], (1, 1, 1, 1), mode='reflect')[0, 0]          # even reflection about every edge node
    c, E, W, Nn, S = p[1:-1, 1:-1], p[2:, 1:-1], p[:-2, 1:-1], p[1:-1, 2:], p[1:-1, :-2]
    EN, ES, WN, WS = p[2:, 2:], p[2:, :-2], p[:-2, 2:], p[:-2, :-2]
    to = gx.dtype
    px, py = ((E - W) * inv2h).to(to), ((Nn - S) * inv2h).to(to)
    a = (1.0 + ((E - 2.0 * c) + W) * invh2).to(to)
    b = (1.0 + ((Nn - 2.0 * c) + S) * invh2).to(to)
    cc = ((((EN - ES) - WN) + WS) * inv4h2).to(to)
    x, y = gx + px, gy + py
    det = a * b - cc * cc
    lam = 0.5 * ((a + b) - torch.sqrt((a - b) * (a - b) + 4.0 * (cc * cc)))
    m = table_monitor(x, y, M)
    if flip is not None:
        m = m * flip
    return x, y, torch.log(m * det), lam


def ma(N, table, arith='fp32', cfl=0.2, tol=1e-4, max_steps=20000, perturb=None, also_at=None):
    """-> (xy [2, N, N], steps, res, status, lmin, xy_at): the iteration to its stopping step in the arithmetic given.  `lmin` is
    the smallest lambda met at any evaluation up to the stop.  With `also_at=j`, `xy_at` is x, y of the phi after exactly j updates
    with no stopping test applied up to there (the iteration goes on past its own stopping step if it has to)."""
    if arith not in ARITHMETICS:
        raise ValueError(arith)
    work = torch.float64 if arith == 'fp64' else torch.float32               # everything but phi
    hold = torch.float32 if arith == 'fp32' else torch.float64               # phi
    M = table_in(table, work)
    gx, gy = R.grid(N, work)
    w1 = torch.ones(N, dtype=work)
    w1[0] = w1[-1] = 0.5
    w = w1[:, None] * w1[None, :]
    invh2 = float((N - 1) * (N - 1))
    dt = torch.tensor(cfl / invh2, dtype=work)                               # (float)(cfl / n1^2)
    tol_t = torch.tensor(tol, dtype=torch.float32).to(work)                  # the kernel compares with the fp32 tol
    rng = None if perturb is None else torch.Generator().manual_seed(perturb)
    ulp = torch.tensor(2.0 ** -23, dtype=work)
    phi = torch.zeros(N, N, dtype=hold)
    steps, lowest, stop, xy_at = 0, float('inf'), None, None
    while True:
        flip = None if rng is None else 1.0 + (torch.randint(0, 2, (N, N), generator=rng).to(work) * 2.0 - 1.0) * ulp
        x, y, r, lam = evaluate(phi, N, gx, gy, M, flip)
        rbar = (w * r).sum() / invh2
        res = torch.maximum(r.max() - rbar, rbar - r.min())
        lmin = lam.min()
        if also_at == steps:
            xy_at = torch.stack([x, y])
        if stop is None:
            lowest = min(lowest, lmin.item())
            status = None
            if not (lmin.item() > 0) or not bool(torch.isfinite(res)):
                status = NONCONVEX
            elif tol > 0 and bool(res <= tol_t):
                status = CONVERGED
            elif steps == max_steps:
                status = CAP
            if status is not None:
                stop = (torch.stack([x, y]), steps, res.item(), status, lowest)
        if stop is not None and (also_at is None or xy_at is not None or stop[3] == NONCONVEX):
            return stop + (xy_at,)
        phi = phi + ((dt * torch.clamp(lmin, max=1.0)) * (r - rbar)).to(hold)
        steps += 1
