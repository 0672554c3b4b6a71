"""The Monge-Ampere iteration with the M2N 'fast' monitor (include/gadapt_mesh.h, gadapt_ma_m2n_batch and
gadapt_ma_m2n_batch_strided) restated in torch, and the cell spread under that monitor.

The iteration is `ma_restatement.ma`'s with the monitor replaced: m = reg + beta F / Fmax, F = sqrt((u_xx^2 + 2 u_xy^2) + u_yy^2),
u_xy the LAST Gaussian's only (the reference assigns it with `=` inside its loop), Fmax the maximum of F over the mesh's nodes
at that evaluation, and m = reg where Fmax is not positive.  There is no power.  The operations and their association are the
header's; only the order of the sum behind the trapezium mean differs (torch's), and a maximum has no order.

`arith` chooses the arithmetic: 'fp64' (the yardstick), 'fp32' (the lane route) or 'mixed' (the strided route: phi and the five
stencil expressions in fp64, each rounded once to fp32, the rest in fp32, the fp32 increment added in fp64, as
`ma_strided_restatement` does for the 'ma' monitor).  `perturb=seed` multiplies m, after the normalisation, per node and
evaluation by 1 + 2^-23 or 1 - 2^-23: an expf / logf / sqrtf or a quotient that rounds the other way, measured.
"""
import torch
import torch.nn.functional as F

from ma_restatement import CAP, CONVERGED, NONCONVEX, grid, inputs, triangles_keep_orientation  # noqa: F401

ARITH = {'fp64': (torch.float64, torch.float64), 'fp32': (torch.float32, torch.float32), 'mixed': (torch.float64, torch.float32)}


def constants(params, dtype):
    """([G, 4] Gaussians, mon_reg, beta) as the kernel receives them (fp32), carried in `dtype`."""
    g = inputs(params, dtype)[0]
    reg, beta = params['mon_reg'], params.get('M2N_beta', 1.5)
    return g, torch.tensor(reg, dtype=torch.float32).to(dtype), torch.tensor(beta, dtype=torch.float32).to(dtype)


def hessian_norm(x, y, g, last_only=True):
    """F at the points given.  `last_only=False` sums u_xy over the Gaussians: what the reference would compute with `+=`."""
    uxx, uyy, uxy = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    for c0, c1, s0, s1 in g:
        q0, q1 = s0 * s0, s1 * s1
        iq0, iq1 = 1.0 / q0, 1.0 / q1
        a0, b0, a1, b1 = 4.0 / (q0 * q0), 2.0 / q0, 4.0 / (q1 * q1), 2.0 / q1
        cxy = (16.0 * iq0) * iq1
        dx, dy = x - c0, y - c1
        dx2, dy2 = dx * dx, dy * dy
        e = torch.exp(-(dx2 * iq0) - dy2 * iq1)
        uxx = uxx + (a0 * dx2 - b0) * e
        uyy = uyy + (a1 * dy2 - b1) * e
        mixed = (cxy * (dx * dy)) * e
        uxy = mixed if last_only else uxy + mixed
    return torch.sqrt((uxx * uxx + 2.0 * (uxy * uxy)) + uyy * uyy)


def normalised(Fn, Fmax, reg, beta):
    return reg + beta * (Fn / Fmax) if bool(Fmax > 0) else reg + torch.zeros_like(Fn)


def monitor(x, y, g, reg, beta):
    """The monitor on the points given, its maximum over those points."""
    Fn = hessian_norm(x, y, g)
    return normalised(Fn, Fn.max(), reg, beta)


def evaluate(phi, N, gx, gy, g, reg, beta, low, flip=None):
    """(x, y, r, lambda) in `low` of the potential phi [N, N]; the five stencil expressions in phi's dtype, each rounded once."""
    n1 = float(N - 1)
    inv2h, invh2, inv4h2 = 0.5 * n1, n1 * n1, 0.25 * n1 * n1
    p = F.pad(phi[None, None], (1, 1, 1, 1), mode='reflect')[0, 0]          # even reflection about every edge node
    c, E, W, Nn, S = p[1:-1, 1:-1], p[2:, 1:-1], p[:-2, 1:-1], p[1:-1, 2:], p[1:-1, :-2]
    EN, ES, WN, WS = p[2:, 2:], p[2:, :-2], p[:-2, 2:], p[:-2, :-2]
    px, py = ((E - W) * inv2h).to(low), ((Nn - S) * inv2h).to(low)
    a = (1.0 + ((E - 2.0 * c) + W) * invh2).to(low)
    b = (1.0 + ((Nn - 2.0 * c) + S) * invh2).to(low)
    cc = ((((EN - ES) - WN) + WS) * inv4h2).to(low)
    x, y = gx + px, gy + py
    det = a * b - cc * cc
    lam = 0.5 * ((a + b) - torch.sqrt((a - b) * (a - b) + 4.0 * (cc * cc)))
    m = monitor(x, y, g, reg, beta)
    if flip is not None:
        m = m * flip
    return x, y, torch.log(m * det), lam


def ma(N, params, arith='fp64', cfl=0.2, tol=1e-4, max_steps=20000, perturb=None):
    """-> (xy [2, N, N], steps, res, status, lmin): the iteration to its stopping step.  `lmin` is the smallest lambda met at
    any evaluation."""
    high, low = ARITH[arith]
    g, reg, beta = constants(params, low)
    gx, gy = grid(N, low)
    w1 = torch.ones(N, dtype=low)
    w1[0] = w1[-1] = 0.5
    w = w1[:, None] * w1[None, :]
    invh2 = torch.tensor(float((N - 1) * (N - 1)), dtype=low)
    dt = torch.tensor(cfl / float((N - 1) * (N - 1)), dtype=low)            # (float)(cfl / n1^2) on both routes
    tol_t = torch.tensor(tol, dtype=torch.float32).to(low)                  # the kernel compares with the fp32 tol
    rng = None if perturb is None else torch.Generator().manual_seed(perturb)
    ulp = torch.tensor(2.0 ** -23, dtype=low)
    phi = torch.zeros(N, N, dtype=high)
    steps, lowest = 0, float('inf')
    while True:
        flip = None if rng is None else 1.0 + (torch.randint(0, 2, (N, N), generator=rng).to(low) * 2.0 - 1.0) * ulp
        x, y, r, lam = evaluate(phi, N, gx, gy, g, reg, beta, low, flip)
        rbar = (w * r).sum() / invh2
        res = torch.maximum(r.max() - rbar, rbar - r.min())
        lmin = lam.min()
        lowest = min(lowest, lmin.item())
        if not (lmin.item() > 0) or not bool(torch.isfinite(res)):
            status = NONCONVEX
            break
        if tol > 0 and bool(res <= tol_t):
            status = CONVERGED
            break
        if steps == max_steps:
            status = CAP
            break
        phi = phi + ((dt * torch.clamp(lmin, max=1.0)) * (r - rbar)).to(high)
        steps += 1
    return torch.stack([x, y]), steps, res.item(), status, lowest


def cell_spread(xy, params):
    """cv = std(q) / mean(q) with q = m(cell centroid) * cell area over the (N - 1)^2 quads, in fp64, m normalised by the
    maximum of F over the mesh's own nodes: 0 for a mesh that equidistributes the monitor exactly."""
    xy = xy.double()
    g, reg, beta = constants(params, torch.float64)
    x, y = xy[0], xy[1]
    corners = [(x[:-1, :-1], y[:-1, :-1]), (x[1:, :-1], y[1:, :-1]), (x[1:, 1:], y[1:, 1:]), (x[:-1, 1:], y[:-1, 1:])]
    area = torch.zeros_like(x[:-1, :-1])
    for (xa, ya), (xb, yb) in zip(corners, corners[1:] + corners[:1]):
        area = area + 0.5 * (xa * yb - xb * ya)                             # shoelace, counter-clockwise in (x, y)
    cx, cy = sum(c[0] for c in corners) / 4.0, sum(c[1] for c in corners) / 4.0
    q = normalised(hessian_norm(cx, cy, g), hessian_norm(x, y, g).max(), reg, beta) * area
    return (q.std(unbiased=False) / q.mean()).item()


def uniform_spread(N, params):
    return cell_spread(torch.stack(grid(N, torch.float64)), params)
