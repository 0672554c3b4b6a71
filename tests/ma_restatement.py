"""The Monge-Ampere iteration of include/gadapt_mesh.h restated in torch, for any dtype, and the measures its tests use.

The operations and their association are the header's (and the kernel's): differences are multiplied by the exact constants
n1 / 2, n1^2, n1^2 / 4 with n1 = N - 1, quotients by a Gaussian's squared scale are products by its reciprocal, nothing is
contracted.  Only the order of the sum behind the trapezium mean differs (torch's).  The inputs (Gaussians, mon_reg, mon_power)
are rounded to fp32 first in every dtype: they are the same data the kernel gets.

`ma(..., perturb=seed)` multiplies the monitor per node and per evaluation by 1 + 2^-23 or 1 - 2^-23, drawn from that seed: the
price of an expf / logf / powf that rounds differently from the host's, measured, not guessed.
"""
import torch
import torch.nn.functional as F

CONVERGED, CAP, NONCONVEX = 0, 1, 2


def inputs(params, dtype):
    """([G, 4] Gaussians, mon_reg, mon_power) as the kernel receives them (fp32), carried in `dtype`."""
    cs, ss = params.get('centers', []), params.get('scales', [])
    rows = [[float(c[0]), float(c[1]), float(s[0]), float(s[1])] for c, s in zip(cs, ss)]
    g = torch.tensor(rows, dtype=torch.float32).reshape(-1, 4).to(dtype)
    if 'mon_power' in params:
        reg, power = params['mon_reg'], params['mon_power']
    else:
        reg, power = 1.0, 0.2
    return g, torch.tensor(reg, dtype=torch.float32).to(dtype), torch.tensor(power, dtype=torch.float32).to(dtype)


def monitor(x, y, g, reg, power):
    uxx, uyy = torch.zeros_like(x), torch.zeros_like(x)
    for c0, c1, s0, s1 in g:
        q0, q1 = s0 * s0, s1 * s1
        iq0, iq1 = 1.0 / q0, 1.0 / q1
        a0, b0, a1, b1 = 4.0 / (q0 * q0), 2.0 / q0, 4.0 / (q1 * q1), 2.0 / q1
        dx, dy = x - c0, y - c1
        dx2, dy2 = dx * dx, dy * dy
        e = torch.exp(-(dx2 * iq0) - dy2 * iq1)
        uxx = uxx + (a0 * dx2 - b0) * e
        uyy = uyy + (a1 * dy2 - b1) * e
    return torch.pow(reg + torch.sqrt(uxx * uxx + uyy * uyy), power)


def grid(N, dtype):
    """xi_i = (float)i / (float)(N - 1) in fp32, as the kernel computes it."""
    lin = (torch.arange(N, dtype=torch.float32) / torch.tensor(float(N - 1), dtype=torch.float32)).to(dtype)
    return torch.meshgrid(lin, lin, indexing='ij')


def evaluate(phi, N, gx, gy, g, reg, power, flip=None):
    """(x, y, r, lambda) of the potential phi [N, N]."""
    n1 = float(N - 1)
    inv2h, invh2, inv4h2 = 0.5 * n1, n1 * n1, 0.25 * n1 * n1
    p = F.pad(phi[None, None], (1, 1, 1, 1), mode='reflect')[0, 0]          # even reflection about every edge node
    c, E, W, Nn, S = p[1:-1, 1:-1], p[2:, 1:-1], p[:-2, 1:-1], p[1:-1, 2:], p[1:-1, :-2]
    EN, ES, WN, WS = p[2:, 2:], p[2:, :-2], p[:-2, 2:], p[:-2, :-2]
    x = gx + (E - W) * inv2h
    y = gy + (Nn - S) * inv2h
    a = 1.0 + ((E - 2.0 * c) + W) * invh2
    b = 1.0 + ((Nn - 2.0 * c) + S) * invh2
    cc = (((EN - ES) - WN) + WS) * inv4h2
    det = a * b - cc * cc
    lam = 0.5 * ((a + b) - torch.sqrt((a - b) * (a - b) + 4.0 * (cc * cc)))
    m = monitor(x, y, g, reg, power)
    if flip is not None:
        m = m * flip
    return x, y, torch.log(m * det), lam


def ma(N, params, dtype=torch.float32, cfl=0.2, tol=1e-4, max_steps=20000, perturb=None):
    """-> (xy [2, N, N], steps, res, status, lmin): the iteration to its stopping step.  `lmin` is the smallest lambda met at
    any evaluation."""
    g, reg, power = inputs(params, dtype)
    gx, gy = grid(N, dtype)
    w1 = torch.ones(N, dtype=dtype)
    w1[0] = w1[-1] = 0.5
    w = w1[:, None] * w1[None, :]
    dt = torch.tensor(cfl / float((N - 1) * (N - 1)), dtype=dtype)
    tol_t = torch.tensor(tol, dtype=torch.float32).to(dtype)                # the kernel compares with the fp32 tol
    rng = None if perturb is None else torch.Generator().manual_seed(perturb)
    ulp = torch.tensor(2.0 ** -23, dtype=dtype)
    phi = torch.zeros(N, N, dtype=dtype)
    steps, lowest = 0, float('inf')
    while True:
        flip = None if rng is None else 1.0 + (torch.randint(0, 2, (N, N), generator=rng).to(dtype) * 2.0 - 1.0) * ulp
        x, y, r, lam = evaluate(phi, N, gx, gy, g, reg, power, flip)
        rbar = (w * r).sum() / float((N - 1) * (N - 1))
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
        phi = phi + (dt * torch.clamp(lmin, max=1.0)) * (r - rbar)
        steps += 1
    return torch.stack([x, y]), steps, res.item(), status, lowest


def cell_spread(xy, params):
    """cv = std(q) / mean(q) with q = m(cell centroid) * cell area over the (N - 1)^2 quads, in fp64: 0 for a mesh that
    equidistributes the monitor exactly."""
    xy = xy.double()
    g, reg, power = inputs(params, torch.float64)
    x, y = xy[0], xy[1]
    corners = [(x[:-1, :-1], y[:-1, :-1]), (x[1:, :-1], y[1:, :-1]), (x[1:, 1:], y[1:, 1:]), (x[:-1, 1:], y[:-1, 1:])]
    area = torch.zeros_like(x[:-1, :-1])
    for (xa, ya), (xb, yb) in zip(corners, corners[1:] + corners[:1]):
        area = area + 0.5 * (xa * yb - xb * ya)                             # shoelace, counter-clockwise in (x, y)
    cx, cy = sum(c[0] for c in corners) / 4.0, sum(c[1] for c in corners) / 4.0
    q = monitor(cx, cy, g, reg, power) * area
    return (q.std(unbiased=False) / q.mean()).item()


def uniform_spread(N, params):
    return cell_spread(torch.stack(grid(N, torch.float64)), params)


def triangles_keep_orientation(xy, cells):
    """True if every triangle of `cells` [T, 3] (node = i * N + j) has a signed area of the sign it has on the uniform grid."""
    N = xy.shape[1]

    def signed(p):
        a, b, c = p[cells[:, 0]], p[cells[:, 1]], p[cells[:, 2]]
        return (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])

    moved = signed(xy.double().reshape(2, -1).t())
    flat = signed(torch.stack(grid(N, torch.float64)).reshape(2, -1).t())
    return bool((moved * flat > 0).all())
