#!/usr/bin/env python
"""Writes tests/golden/burgers_eval/: scipy's answers for a few spline data sets, and one to-convergence Burgers rollout
recorded from the fp64 (and fp32) test-side restatement, which is too slow to recompute in a test.  Needs scipy; CPU only.

    python tests/golden/make_burgers_eval_golden.py

spline_<name>.npz   x, y (fp32 data), q (fp32 queries: a lattice reaching slightly outside the data, plus every knot),
                    s0 = UnivariateSpline(x, y, s=0)(q), s2 = its .derivative(2)(q),
                    c0, c1, c2 = CubicSpline(x, y, bc_type='not-a-knot')(q, 0 / 1 / 2); all fp64
rollout_converged.npz   one sample of the small test config with the default MMPDE5 settings (tol 1e-6): centre, scale,
                    x_ma0 (the start target mesh, fp32), and per dtype L2_grid, L2_MA, steps (per relaxation), x_MA
"""
import os
import sys

import numpy as np
import torch
from scipy.interpolate import CubicSpline, UnivariateSpline

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import burgers_eval_restatement as BE  # noqa: E402
import mmpde5_restatement as M  # noqa: E402

OUT = os.path.join(HERE, 'burgers_eval')

ROLLOUT_OPT = {'mesh_dims': [11], 'num_fine_mesh_points': 20, 'eval_quad_points': 41, 'load_quad_points': 41, 'tau': 1 / 20.0,
               'nu': 1e-3, 'gauss_amplitude': 0.25, 'mon_reg': 0.1, 'mon_power': 0.2, 'num_time_steps': 1, 'num_eval_time_steps': 4}
ROLLOUT_SEED = 5


def graded(n, ratio=100.0):
    h = ratio ** (np.arange(n - 1) / max(n - 2, 1))
    x = np.concatenate([[0.0], np.cumsum(h)])
    return (x / x[-1]).astype(np.float32)


def data_sets():
    f = lambda x: (0.25 * np.exp(-(x - 0.45) ** 2 / 0.02) + 0.1 * np.sin(7 * x)).astype(np.float32)
    rng = np.random.default_rng(0)
    xr = np.sort(rng.uniform(0, 1, 21)).astype(np.float32)
    xr[0], xr[-1] = 0.0, 1.0
    return {'n4': np.array([0.0, 0.3, 0.55, 1.0], np.float32), 'n5': np.linspace(0, 1, 5, dtype=np.float32),
            'uniform_n101': np.linspace(0, 1, 101, dtype=np.float32), 'graded_n65': graded(65), 'random_n21': xr}, f


def main():
    os.makedirs(OUT, exist_ok=True)
    sets, f = data_sets()
    for name, x in sets.items():
        y = f(x)
        q = np.unique(np.concatenate([np.linspace(-0.01, 1.01, 57).astype(np.float32), x]))
        x64, y64, q64 = x.astype(np.float64), y.astype(np.float64), q.astype(np.float64)
        us, cs = UnivariateSpline(x64, y64, s=0), CubicSpline(x64, y64, bc_type='not-a-knot')
        np.savez(os.path.join(OUT, f'spline_{name}.npz'), x=x, y=y, q=q, s0=us(q64), s2=us.derivative(2)(q64),
                 c0=cs(q64), c1=cs(q64, 1), c2=cs(q64, 2))

    from g_adaptivity_amd import MeshDataset
    from g_adaptivity_amd.mmpde5 import monitor_1d, monitor_arrays_1d
    n = ROLLOUT_OPT['mesh_dims'][0]
    s = MeshDataset([n], 1, seed=ROLLOUT_SEED, num_gauss=1, burgers=True).samples[0]
    params = dict(s.pde_params, mon_reg=ROLLOUT_OPT['mon_reg'], mon_power=ROLLOUT_OPT['mon_power'])
    ms, m2 = monitor_arrays_1d(lambda t: monitor_1d(t.double(), params), n)
    x0, _, _ = M.mmpde5(torch.linspace(0, 1, n), ms, m2, dtype=torch.float64)
    x0 = x0.float()
    rec = {'center': np.asarray(s.pde_params['centers'][0], np.float32), 'scale': np.asarray(s.pde_params['scales'][0], np.float32),
           'x_ma0': x0.numpy()}
    for tag, dt in (('f64', torch.float64), ('f32', torch.float32)):
        r = BE.rollout(s.pde_params, x0, ROLLOUT_OPT, n, dtype=dt)
        rec.update({f'L2_grid_{tag}': r['L2_grid'], f'L2_MA_{tag}': r['L2_MA'], f'steps_{tag}': np.asarray(r['steps']),
                    f'x_MA_{tag}': r['x_MA'].double().numpy()})
        print(tag, r['L2_grid'], r['L2_MA'], r['steps'])
    np.savez(os.path.join(OUT, 'rollout_converged.npz'), **rec)


if __name__ == '__main__':
    main()
