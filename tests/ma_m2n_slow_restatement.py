"""The Monge-Ampere iteration with the M2N 'slow' monitor (include/gadapt_mesh.h, gadapt_ma_m2n_slow_batch) restated in torch.

The iteration is `ma_m2n_restatement.ma`'s on the lane route with the monitor replaced:
    m = (reg + alpha E / Emax) + beta F / Fmax,   E = (u_h - u)^2,
u the sum of the Gaussians at the nodes, u_h the P1 solution of -Laplace(u_h) = f = -(u_xx + u_yy) with u_h = u on the boundary,
on the mesh of the CURRENT nodes (`square_mesh(N)`'s triangles), with the consistent mass matrix applied to the nodal f as
the load.  Both maxima are over the mesh's nodes at that evaluation; a term whose maximum is not positive is 0.

The element terms and their association are the header's (tri_geometry, inv = 1 / (2 |D|), p = (r_l . r_k) * inv, load
(|D| / 24) * (f_l + ((f_0 + f_1) + f_2))).  The triangles are summed into a dense matrix in torch's order, not the kernel's.
The factorisation and the two substitutions are the header's, column by column and entry by entry (`cholesky_solve`): quotients
by the pivot's root, plain products and differences, so that the fp32 run carries the rounding of THAT factorisation (the fp64
yardstick takes the library's: the two differ at 1e-16, and tests/test_ma_m2n_slow_host.py compares them).  A library
Cholesky (blocked, with fused multiply-adds) rounds less and differently, and the solve is where this monitor's fp32 noise is
made: e = c - u cancels three digits.

`arith` is 'fp64' (the yardstick) or 'fp32' (the kernel's arithmetic).  `perturb=seed` multiplies m per node and evaluation by
1 + 2^-23 or 1 - 2^-23, as in ma_m2n_restatement: an expf / logf / sqrtf or a quotient that rounds the other way, measured.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from ma_restatement import CAP, CONVERGED, NONCONVEX, grid, inputs, triangles_keep_orientation  # noqa: F401

from g_adaptivity_amd import square_mesh

ARITH = {'fp64': torch.float64, 'fp32': torch.float32}


def constants(params, dtype):
    """([G, 4] Gaussians, mon_reg, alpha, beta) as the kernel receives them (fp32), carried in `dtype`."""
    g = inputs(params, dtype)[0]
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype)  # noqa: E731
    return g, f32(params['mon_reg']), f32(params.get('M2N_alpha', 1.0)), f32(params.get('M2N_beta', 1.0))


def fields(x, y, g):
    """(u, f, F) at the points given: the Gaussians' sum, f = -(u_xx + u_yy), and F with the last Gaussian's u_xy."""
    uxx, uyy, uxy, u = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
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
        u = u + e
        uxy = (cxy * (dx * dy)) * e
    return u, -(uxx + uyy), torch.sqrt((uxx * uxx + 2.0 * (uxy * uxy)) + uyy * uyy)


@functools.lru_cache(maxsize=None)
def topology(N):
    """(cells [T, 3], interior node numbers, boundary node numbers) of square_mesh(N); interior in row order r = (i-1)(N-2) + (j-1)."""
    cells = square_mesh(N).cells
    i, j = torch.meshgrid(torch.arange(N), torch.arange(N), indexing='ij')
    inner = ((i > 0) & (i < N - 1) & (j > 0) & (j < N - 1)).reshape(-1)
    node = torch.arange(N * N)
    return cells, node[inner], node[~inner]


def assemble(x, y, f, N):
    """(K [N^2, N^2], b [N^2]): the P1 stiffness matrix on the nodes (x, y) and the consistent-mass load of the nodal f."""
    cells = topology(N)[0]
    px, py = x.reshape(-1)[cells], y.reshape(-1)[cells]                                    # [T, 3]
    rx = torch.stack([py[:, 1] - py[:, 2], py[:, 2] - py[:, 0], py[:, 0] - py[:, 1]], 1)
    ry = torch.stack([px[:, 2] - px[:, 1], px[:, 0] - px[:, 2], px[:, 1] - px[:, 0]], 1)
    D = px[:, 0] * (py[:, 1] - py[:, 2]) + px[:, 1] * (py[:, 2] - py[:, 0]) + px[:, 2] * (py[:, 0] - py[:, 1])
    aD = D.abs()
    inv = 1.0 / (2.0 * aD)
    Pe = (rx[:, :, None] * rx[:, None, :] + ry[:, :, None] * ry[:, None, :]) * inv[:, None, None]
    K = torch.zeros(N * N, N * N, dtype=x.dtype)
    K.index_put_((cells[:, :, None].expand(-1, 3, 3), cells[:, None, :].expand(-1, 3, 3)), Pe, accumulate=True)
    ff = f.reshape(-1)[cells]
    load = (aD / 24.0)[:, None] * (ff + ((ff[:, 0] + ff[:, 1]) + ff[:, 2])[:, None])
    b = torch.zeros(N * N, dtype=x.dtype).index_add_(0, cells.reshape(-1), load.reshape(-1))
    return K, b


def cholesky_solve(A, b, w):
    """c with A c = b for a symmetric positive definite A of half-bandwidth w, by the header's right-looking Cholesky in A's own
    dtype: per column k, d = sqrt(A[k][k]); the column below divided by d and b[k] / d; A[k+i][k+j] -= L[k+i][k] L[k+j][k] and
    b[k+i] -= L[k+i][k] b[k]; backwards y = b[k] / d_k, b[k-j] -= L[k][k-j] y, b[k] left as the numerator; c = b / d.  Every
    product and difference is rounded by itself (numpy does not fuse).  None where a pivot is not positive."""
    A, b = A.numpy().copy(), b.numpy().copy()
    n = A.shape[0]
    for k in range(n):
        if not A[k, k] > 0:
            return None
        d = np.sqrt(A[k, k])
        hi = min(k + w, n - 1) + 1
        A[k + 1:hi, k] /= d
        b[k] /= d
        A[k, k] = d
        col = A[k + 1:hi, k]
        A[k + 1:hi, k + 1:hi] -= np.multiply.outer(col, col)
        b[k + 1:hi] -= col * b[k]
    for k in range(n - 1, -1, -1):
        lo = max(k - w, 0)
        b[lo:k] -= A[k, lo:k] * (b[k] / A[k, k])
    return torch.from_numpy(b / np.diagonal(A))


def solve_error(x, y, u, f, N):
    """e [N, N] = u_h - u at the interior nodes, 0 on the boundary; NaN everywhere where the Cholesky factor does not exist."""
    _, I, Bn = topology(N)
    K, b = assemble(x, y, f, N)
    uf = u.reshape(-1)
    rhs = b[I] - K[I][:, Bn] @ uf[Bn]
    if x.dtype == torch.float64:                         # the yardstick: which Cholesky rounds at 1e-16 is below everything measured
        L, info = torch.linalg.cholesky_ex(K[I][:, I])
        c = None if int(info) != 0 else torch.cholesky_solve(rhs[:, None], L)[:, 0]
    else:
        c = cholesky_solve(K[I][:, I], rhs, N - 2)
    if c is None:
        return torch.full_like(x, float('nan'))
    e = torch.zeros(N * N, dtype=x.dtype)
    e[I] = c - uf[I]
    return e.reshape(N, N)


def term(v, top, weight):
    return weight * (v / top) if bool(top > 0) else torch.zeros_like(v)


def monitor(x, y, g, reg, alpha, beta):
    """The monitor on the N x N node set given (it is its own mesh), both maxima over those nodes."""
    N = x.shape[0]
    u, f, Fn = fields(x, y, g)
    e = solve_error(x, y, u, f, N)
    if bool(torch.isnan(e).any()):
        return e
    E = e * e
    return (reg + term(E, E.max(), alpha)) + term(Fn, Fn.max(), beta)


def evaluate(phi, N, gx, gy, g, reg, alpha, beta, flip=None):
    """(x, y, r, lambda, m) of the potential phi [N, N], as ma_m2n_restatement.evaluate on the lane route."""
    n1 = float(N - 1)
    inv2h, invh2, inv4h2 = 0.5 * n1, n1 * n1, 0.25 * n1 * n1
    p = F.pad(phi[None, None], (1, 1, 1, 1), mode='reflect')[0, 0]          # even reflection about every edge node
    c, E, W, Nn, S = p[1:-1, 1:-1], p[2:, 1:-1], p[:-2, 1:-1], p[1:-1, 2:], p[1:-1, :-2]
    EN, ES, WN, WS = p[2:, 2:], p[2:, :-2], p[:-2, 2:], p[:-2, :-2]
    x, y = gx + (E - W) * inv2h, gy + (Nn - S) * inv2h
    a = 1.0 + ((E - 2.0 * c) + W) * invh2
    b = 1.0 + ((Nn - 2.0 * c) + S) * invh2
    cc = (((EN - ES) - WN) + WS) * inv4h2
    det = a * b - cc * cc
    lam = 0.5 * ((a + b) - torch.sqrt((a - b) * (a - b) + 4.0 * (cc * cc)))
    m = monitor(x, y, g, reg, alpha, beta)
    if flip is not None:
        m = m * flip
    return x, y, torch.log(m * det), lam, m


def ma(N, params, arith='fp64', cfl=0.2, tol=1e-4, max_steps=20000, perturb=None, also_at=None):
    """-> (xy [2, N, N], steps, res, status, lmin, m [N, N], xy_at): the iteration to its stopping step.  `lmin` is the smallest
    lambda met at any evaluation up to there, m the monitor of the last one.  With `also_at=j` the same trajectory is also read off
    after exactly j updates (xy_at: what tol = 0, max_steps = j would return; the updates go on past the stopping step if j lies
    beyond it), so that one run serves a converged comparison and a fixed-count one; without it xy_at is xy."""
    dtype = ARITH[arith]
    g, reg, alpha, beta = constants(params, dtype)
    gx, gy = grid(N, dtype)
    w1 = torch.ones(N, dtype=dtype)
    w1[0] = w1[-1] = 0.5
    w = w1[:, None] * w1[None, :]
    invh2 = torch.tensor(float((N - 1) * (N - 1)), dtype=dtype)
    dt = torch.tensor(cfl / float((N - 1) * (N - 1)), dtype=dtype)          # (float)(cfl / n1^2)
    tol_t = torch.tensor(tol, dtype=torch.float32).to(dtype)                # the kernel compares with the fp32 tol
    rng = None if perturb is None else torch.Generator().manual_seed(perturb)
    ulp = torch.tensor(2.0 ** -23, dtype=dtype)
    phi = torch.zeros(N, N, dtype=dtype)
    steps, lowest, stopped, xy_at = 0, float('inf'), None, None
    while True:
        flip = None if rng is None else 1.0 + (torch.randint(0, 2, (N, N), generator=rng).to(dtype) * 2.0 - 1.0) * ulp
        x, y, r, lam, m = evaluate(phi, N, gx, gy, g, reg, alpha, beta, flip)
        rbar = (w * r).sum() / invh2
        res = torch.maximum(r.max() - rbar, rbar - r.min())
        lmin = lam.min()
        if steps == also_at:
            xy_at = torch.stack([x, y])
        if stopped is None:
            lowest = min(lowest, lmin.item())
            status = None
            if not (lmin.item() > 0) or not bool(torch.isfinite(res)):
                status = NONCONVEX
            elif tol > 0 and bool(res <= tol_t):
                status = CONVERGED
            elif steps == max_steps:
                status = CAP
            if status is not None:
                stopped = (torch.stack([x, y]), steps, res.item(), status, lowest, m)
        if stopped is not None and (also_at is None or steps >= also_at):
            break
        phi = phi + (dt * torch.clamp(lmin, max=1.0)) * (r - rbar)
        steps += 1
    return stopped + (stopped[0] if also_at is None else xy_at,)
