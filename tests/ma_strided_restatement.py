"""The strided Monge-Ampere route's arithmetic (include/gadapt_mesh.h, gadapt_ma_batch_strided) restated in torch: phi and its
differences in fp64, everything else fp32.

The five stencil expressions are formed in fp64 from the fp64 phi with the lane route's association and exact constants, each
rounded once to fp32; x = xi + px, det, lambda, the Gaussians, the monitor and r = log(m det) are `ma_restatement`'s fp32
operations; the increment (dt min(1, lmin)) (r - rbar) is formed in fp32 and added to phi in fp64.  Only the order of the sum
behind the trapezium mean differs from the kernel's (torch's).  `ma_restatement.ma(dtype=torch.float64)` stays the yardstick;
this file measures what the mixed arithmetic, and an expf / logf / powf that rounds the other way (`perturb`), cost against it.
"""
import torch
import torch.nn.functional as F

import ma_restatement as R

CONVERGED, CAP, NONCONVEX = R.CONVERGED, R.CAP, R.NONCONVEX


def evaluate(phi, N, gx, gy, g, reg, power, flip=None):
    """(x, y, r, lambda) in fp32 of the fp64 potential phi [N, N]; gx, gy, g, reg, power in fp32."""
    n1 = float(N - 1)
    inv2h, invh2, inv4h2 = 0.5 * n1, n1 * n1, 0.25 * n1 * n1
    p = F.pad(phi[None, None], (1, 1, 1, 1), mode='reflect')[0, 0]          # even reflection about every edge node
    c, E, W, Nn, S = p[1:-1, 1:-1], p[2:, 1:-1], p[:-2, 1:-1], p[1:-1, 2:], p[1:-1, :-2]
    EN, ES, WN, WS = p[2:, 2:], p[2:, :-2], p[:-2, 2:], p[:-2, :-2]
    px, py = ((E - W) * inv2h).float(), ((Nn - S) * inv2h).float()
    a = (1.0 + ((E - 2.0 * c) + W) * invh2).float()
    b = (1.0 + ((Nn - 2.0 * c) + S) * invh2).float()
    cc = ((((EN - ES) - WN) + WS) * inv4h2).float()
    x, y = gx + px, gy + py
    det = a * b - cc * cc
    lam = 0.5 * ((a + b) - torch.sqrt((a - b) * (a - b) + 4.0 * (cc * cc)))
    m = R.monitor(x, y, g, reg, power)
    if flip is not None:
        m = m * flip
    return x, y, torch.log(m * det), lam


def ma(N, params, cfl=0.2, tol=1e-4, max_steps=20000, perturb=None, also_at=None):
    """-> (xy [2, N, N] fp32, steps, res, status, lmin, phi fp64, xy_at): the mixed iteration to its stopping step, as
    `ma_restatement.ma`.  With `also_at=j`, `xy_at` is x, y of the phi after exactly j updates with no stopping test applied up
    to there (the iteration goes on past its own stopping step if it has to; steps, res, status and phi are the stop's)."""
    f32 = torch.float32
    g, reg, power = R.inputs(params, f32)
    gx, gy = R.grid(N, f32)
    w1 = torch.ones(N, dtype=f32)
    w1[0] = w1[-1] = 0.5
    w = w1[:, None] * w1[None, :]
    invh2 = torch.tensor(float((N - 1) * (N - 1)), dtype=f32)
    dt = torch.tensor(cfl / float((N - 1) * (N - 1)), dtype=f32)            # (float)(cfl / n1^2)
    tol_t = torch.tensor(tol, dtype=f32)
    rng = None if perturb is None else torch.Generator().manual_seed(perturb)
    ulp = torch.tensor(2.0 ** -23, dtype=f32)
    phi = torch.zeros(N, N, dtype=torch.float64)
    steps, lowest, stop, xy_at = 0, float('inf'), None, None
    while True:
        flip = None if rng is None else 1.0 + (torch.randint(0, 2, (N, N), generator=rng).to(f32) * 2.0 - 1.0) * ulp
        x, y, r, lam = evaluate(phi, N, gx, gy, g, reg, power, flip)
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
                stop = (torch.stack([x, y]), steps, res.item(), status, lowest, phi)
        if stop is not None and (also_at is None or xy_at is not None or stop[3] == NONCONVEX):
            return stop + (xy_at,)
        phi = phi + ((dt * torch.clamp(lmin, max=1.0)) * (r - rbar)).double()
        steps += 1
