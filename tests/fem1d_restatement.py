"""Test-side restatement of the 1-D FEM tails (Burgers steps, Poisson) in CPU torch, written from the formulas.

Everything is dense and literal by default: the hat functions with their inclusive interval test and the -1 at the node, the
trapezoid inner products over k points per interval, searchsorted point location.  Any dtype (fp32 / fp64) and autograd
in the mesh coordinates.  The GPU tails (g_adaptivity_amd.fem1d) are checked against this in fp64, with the fp32 run as
the noise scale.  banded=True swaps the O(N^2 k) mass assembly for the tridiagonal one (mass_bands), pinned to the dense
one in test_fem1d_host.py; the Poisson restatement has no mass matrix and needs no such switch.
"""
import torch


def aux(x, a, b):
    return ((x >= torch.minimum(a, b)) * 1.0) * ((x <= torch.maximum(a, b)) * 1.0) * (x - a) / (b - a)


def phim(x, mesh, n):
    N = mesh.shape[0]
    if n == 0:
        return aux(x, mesh[1], mesh[0])
    if n == N - 1:
        return aux(x, mesh[N - 2], mesh[N - 1])
    return aux(x, mesh[n - 1], mesh[n]) + aux(x, mesh[n + 1], mesh[n]) - ((x == mesh[n]) * 1.0)


def quad_points(mesh, k):
    """[N-1, k] points per interval: start + (diff * j) / (k-1)."""
    j = torch.arange(k, dtype=mesh.dtype)
    return mesh[:-1, None] + (torch.diff(mesh)[:, None] * j[None, :]) / (k - 1)


def inner_product(mesh, f, k):
    """Row m: trapezoid of f * phis over interval m-1 plus of f * reversed phis over interval m."""
    xq = quad_points(mesh, k)
    phis = torch.arange(k, dtype=mesh.dtype)[None, :] / (k - 1)
    fv = f(xq)
    left = torch.trapezoid(fv * phis, xq)
    right = torch.trapezoid(fv * torch.flip(phis, dims=[1]), xq)
    z = torch.zeros(1, dtype=mesh.dtype)
    return torch.cat([z, left]) + torch.cat([right, z])


def mass_matrix(mesh, k, banded=False):
    if banded:
        lo, di, up = mass_bands(mesh, k)
        return torch.diag(di) + torch.diag(up, 1) + torch.diag(lo, -1)
    return torch.stack([inner_product(mesh, lambda x, n=n: phim(x, mesh, n), k) for n in range(mesh.shape[0])], 1)


def _own_hats(mesh, xq):
    """phim of each interval's own two nodes at its k points: ([N-1, k] of node i, [N-1, k] of node i+1), element by
    element the arithmetic of phim."""
    N = mesh.shape[0]
    if N == 2:
        return phim(xq, mesh, 0), phim(xq, mesh, 1)
    a, b, c = mesh[:-2, None], mesh[1:-1, None], mesh[2:, None]          # nodes n-1, n, n+1 of the interior nodes n
    inner = lambda x: aux(x, a, b) + aux(x, c, b) - ((x == b) * 1.0)
    left = torch.cat([phim(xq[:1], mesh, 0), inner(xq[1:])])             # node i on interval i: i = 0 is the end node
    right = torch.cat([inner(xq[:-1]), phim(xq[-1:], mesh, N - 1)])      # node i+1 on interval i: i = N-2 is the end node
    return left, right


def mass_bands(mesh, k):
    """(lower [N-1], diagonal [N], upper [N-1]) of the mass matrix from the trapezoids of mass_matrix restricted to the two
    hats of each interval: O(N k), any dtype, autograd in the mesh.  What mass_matrix holds beyond these (a hat seen from an
    interval it does not touch: a rounding-level value at an interval end, or an overlap on a folded mesh) is left out, as
    the GPU kernel leaves it out."""
    xq = quad_points(mesh, k)
    phis = torch.arange(k, dtype=mesh.dtype)[None, :] / (k - 1)
    rev = torch.flip(phis, dims=[1])
    hl, hr = _own_hats(mesh, xq)
    z = torch.zeros(1, dtype=mesh.dtype)
    lo = torch.trapezoid(hl * phis, xq)                                  # M[i+1][i]
    up = torch.trapezoid(hr * rev, xq)                                   # M[i][i+1]
    di = torch.cat([z, torch.trapezoid(hr * phis, xq)]) + torch.cat([torch.trapezoid(hl * rev, xq), z])
    return lo, di, up


def stiffness_matrix(mesh, k=3):
    """The vectorised stiffness: trapezoids over k+1 points of the constant slope products."""
    N = mesh.shape[0]
    d = torch.diff(mesh)
    xq = mesh[:-1, None] + (torch.arange(k + 1, dtype=mesh.dtype)[None, :] * d[:, None]) / k
    L = (1 / d)[:, None].expand(-1, k + 1)
    R = -L
    off = torch.trapezoid(L * R, xq)
    diag = torch.trapezoid(L[:-1] ** 2, xq[:-1]) + torch.trapezoid(R[1:] ** 2, xq[1:])
    first, last = torch.trapezoid(L[0] ** 2, xq[0]), torch.trapezoid(R[-1] ** 2, xq[-1])
    A = torch.diag(torch.cat([first[None], diag, last[None]])) + torch.diag(off, 1) + torch.diag(off, -1)
    return A


def locate(mesh, p):
    return torch.clamp(torch.searchsorted(mesh.detach(), p.detach().contiguous(), right=False) - 1, 0, mesh.shape[0] - 1)


def fn_expansion(c, mesh, p):
    N = mesh.shape[0]
    slope = torch.cat([(c[1:] - c[:-1]) / (mesh[1:] - mesh[:-1]), torch.zeros(1, dtype=c.dtype)])
    I = locate(mesh, p)
    return c[I] + slope[I] * (p - mesh[I])


def dxfn_expansion(c, mesh, p):
    N = mesh.shape[0]
    dphi = 1 / (mesh[1:] - mesh[:-1])
    a = c[1:] * dphi - c[:-1] * dphi
    return a[torch.clamp(locate(mesh, p), max=N - 2)]


def gauss(x, centers, scales):
    out = torch.zeros_like(x)
    for c, s in zip(centers, scales):
        out = out + torch.exp(-(x - c) ** 2 / s ** 2)
    return out


def forcing(x, centers, scales):
    out = torch.zeros_like(x)
    for c, s in zip(centers, scales):
        out = out + -2 * torch.exp(-(x - c) ** 2 / s ** 2) * (s ** 2 - 2 * (x - c) ** 2) / s ** 4
    return out


def _with_bc_rows(Mat):
    Mat = Mat.clone()
    N = Mat.shape[0]
    Mat[0, :] = 0
    Mat[-1, :] = 0
    Mat[0, 0] = 1
    Mat[-1, -1] = 1
    return Mat


def project(mesh, centers, scales, amp, k_mass, k_load, banded=False):
    """Detached L2 projection of amp * gauss with identity boundary rows, RHS ends u0(0), u0(1)."""
    mesh = mesh.detach()
    u0 = lambda x: amp * gauss(x, centers, scales)
    M = _with_bc_rows(mass_matrix(mesh, k_mass, banded))
    rhs = inner_product(mesh, u0, k_load)
    one = torch.ones(1, dtype=mesh.dtype)
    rhs[0] = u0(0 * one)[0]
    rhs[-1] = u0(one)[0]
    return torch.linalg.solve(M, rhs).detach()


def burgers_step(mesh, u, tau, nu, k_load, points, bc=None, banded=False):
    M = mass_matrix(mesh, k_load, banded)
    A = stiffness_matrix(mesh, 3)
    F = inner_product(mesh, lambda x: fn_expansion(u, mesh, x) * dxfn_expansion(u, mesh, x), k_load)
    rhs = M @ u - tau * F
    rhs = torch.cat([(u[:1] if bc is None else bc[:1]), rhs[1:-1], (u[-1:] if bc is None else bc[1:])])
    Mat = _with_bc_rows(M + (tau * nu) * A)
    un1 = torch.linalg.solve(Mat, rhs)
    return un1, fn_expansion(un1, mesh, points)


def burgers(mesh, centers, scales, opt, n_steps, points, u0=None, fine=True, banded=False):
    """(u^T, sol, fine_sol) of the reference's Burgers loss computation on one mesh."""
    dt = mesh.dtype
    amp, tau, nu = opt['gauss_amplitude'], opt['tau'], opt['nu']
    kl, ev = opt['load_quad_points'], opt['eval_quad_points']
    u = project(mesh, centers, scales, amp, ev, kl, banded) if u0 is None else u0
    sol = None
    for _ in range(n_steps):
        u, sol = burgers_step(mesh, u, tau, nu, kl, points, banded=banded)
    fsol = None
    if fine:
        fm = torch.linspace(0, 1, opt['num_fine_mesh_points'], dtype=dt)
        uf = project(fm, centers, scales, amp, 10 * ev, kl, banded)
        with torch.no_grad():
            for _ in range(n_steps):
                uf, fsol = burgers_step(fm, uf, tau, nu, kl, points, banded=banded)
    return u, sol, fsol


def poisson(mesh, centers, scales, opt, points):
    """(coeffs [N] with the detached boundary values at the ends, sol) of torch_FEM_1D on one mesh."""
    A = stiffness_matrix(mesh, opt.get('stiff_quad_points', 3))
    A_int = -A[1:-1, 1:-1]
    bc1 = gauss(mesh[:1].detach(), centers, scales)
    bc2 = gauss(mesh[-1:].detach(), centers, scales)
    rhs = inner_product(mesh, lambda x: forcing(x, centers, scales), opt['load_quad_points'])[1:-1]
    adj = torch.zeros_like(rhs)
    adj = adj + torch.nn.functional.pad(bc1 * A[0, 1], (0, rhs.shape[0] - 1))
    adj = adj + torch.nn.functional.pad(A[-1, -2] * bc2, (rhs.shape[0] - 1, 0))
    c_int = torch.linalg.solve(A_int, rhs + adj)
    c = torch.cat([bc1, c_int, bc2])
    return c, fn_expansion(c, mesh, points)


def modular_loss(mesh, centers, scales, opt, points, banded=False):
    """The per-mesh loss of gradient_meshpoints_1D for opt['grad_type']."""
    gt = opt['grad_type']
    if gt == 'burgers_timestep_loss_direct_mse':
        _, sol, fsol = burgers(mesh, centers, scales, opt, opt['num_time_steps'], points, banded=banded)
        return ((sol - fsol) ** 2).mean()
    _, sol = poisson(mesh, centers, scales, opt, points)
    err = sol - gauss(points, centers, scales)
    if gt == 'PDE_loss_direct_mse':
        return (err ** 2).mean()
    return torch.trapezoid(err.abs() ** 2, points)
