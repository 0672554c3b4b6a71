"""Test-side restatement of the Burgers rollout evaluation (g_adaptivity_amd.evaluation_burgers) on the CPU, any dtype,
composed from the FEM restatement (project, burgers_step), the MMPDE5 restatement and the spline restatement.

One sample at a time, stage by stage as the reference's evaluate_model_fine_burgers_time_step:

    start     u0 = amp * gauss projected on the uniform grid, the fine mesh, the target mesh, the model's first mesh
    outer     l in range(num_eval_time_steps - 1): num_time_steps FEM steps on every mesh, then the mesh moves
    target    m = (mon_reg + (s''/mx)^2)^mon_power, s the spline of the fine solution on the lattice, mx the signed maximum
              of s'' over linspace(0, 1, num_fine_mesh_points); MMPDE5 from the current mesh; coefficients by the spline of
              (old mesh, coefficients) at the new nodes
    model     new mesh = model_fn(coefficients, mesh) (the test runs the model); coefficients by the same spline
    final     mean square difference to the fine solution after the last FEM step; the target mesh is relaxed once more after
              it (its step count is recorded), the state is not carried over and the model is not called again
"""
import torch

import fem1d_restatement as R
import mmpde5_restatement as M
import spline_restatement as S


def _floats(v):
    return [float(torch.as_tensor(a).reshape(-1)[0]) for a in v]


def monitor_arrays(sol_fine, pts, n, nf, opt, dtype):
    d2 = lambda q: S.spline(pts, sol_fine, q, 2, dtype)
    mx = d2(torch.linspace(0, 1, nf, dtype=dtype)).max()
    m = lambda q: (opt['mon_reg'] + (d2(q) / mx) ** 2.0) ** opt['mon_power']
    return m(torch.linspace(0, 1, 2 * n - 1, dtype=dtype))[1:2 * n - 1:2], m(torch.linspace(0, 1, n, dtype=dtype))


def rollout(pde_params, x_ma0, opt, n, dtype=torch.float64, mmpde5=None, model_fn=None):
    """{'L2_grid', 'L2_MA', 'L2_MLmodel' (with model_fn), 'steps' (per relaxation), 'x_MA'} of one sample.

    model_fn(u, x): the model's mesh for coefficients u on mesh x (both None for the first call, on the sample as loaded)."""
    mm = dict(cfl=0.05, tol=1e-6, max_steps=10000)
    mm.update(mmpde5 or {})
    c, s = _floats(pde_params['centers']), _floats(pde_params['scales'])
    amp, tau, nu, kl, ev = opt['gauss_amplitude'], opt['tau'], opt['nu'], opt['load_quad_points'], opt['eval_quad_points']
    nf, T, L = opt['num_fine_mesh_points'], opt['num_time_steps'], opt['num_eval_time_steps'] - 1
    pts = torch.linspace(0, 1, ev, dtype=dtype)
    grid, fine = torch.linspace(0, 1, n, dtype=dtype), torch.linspace(0, 1, nf, dtype=dtype)

    def steps(mesh, u):
        for _ in range(T):
            u, sol = R.burgers_step(mesh, u, tau, nu, kl, pts)
        return u, sol

    out = {}
    ug, uf = R.project(grid, c, s, amp, ev, kl), R.project(fine, c, s, amp, 10 * ev, kl)
    sol_fine = []
    for _ in range(L):
        ug, sol_g = steps(grid, ug)
        uf, sol_f = steps(fine, uf)
        sol_fine.append(sol_f)
    out['L2_grid'] = float(((sol_g - sol_f) ** 2).mean())

    x = torch.as_tensor(x_ma0).to(dtype)
    u = R.project(x, c, s, amp, ev, kl)
    out['steps'] = []
    for l in range(L):
        u, sol = steps(x, u)
        ms, m2 = monitor_arrays(sol_fine[l], pts, n, nf, opt, dtype)
        x_new, j, _ = M.mmpde5(x, ms, m2, dtype=dtype, **mm)
        out['steps'].append(j)
        if l < L - 1:                      # the last relaxation moves the mesh only: no FEM step follows it
            u = S.spline(x, u, x_new, 0, dtype)
        x = x_new
    out['L2_MA'] = float(((sol - sol_fine[-1]) ** 2).mean())
    out['x_MA'] = x

    if model_fn is not None:
        x = torch.as_tensor(model_fn(None, None)).to(dtype)
        u = R.project(x, c, s, amp, ev, kl)
        for l in range(L):
            u, sol = steps(x, u)
            if l == L - 1:
                break
            x_new = torch.as_tensor(model_fn(u, x)).to(dtype)
            u, x = S.spline(x, u, x_new, 0, dtype), x_new
        out['L2_MLmodel'] = float(((sol - sol_fine[-1]) ** 2).mean())
    return out
