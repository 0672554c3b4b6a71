#!/usr/bin/env python
"""Writes n27.npz and n34.npz (and n64.npz when asked): the 2-D modular loss, its gradient wrt the node coordinates and
the FEM coefficients of jittered n x n meshes from the test-side restatement (tests/modular2d_restatement.py: dense solve
of all nodes, autograd) in fp64 and in fp32, which tests/test_gpu_fem_window_grad.py compares the differentiable windowed
route with.  One call of the restatement takes 12 to 26 s of CPU at 27 and 34 a side and minutes at 64, too long to repeat
in every run of the suite.  The meshes and the Gaussians are the recipes of tests/test_gpu_modular2d.py
(_coords(n, 'jittered', seed=n + 1), _params(2, n)); the test rebuilds the same inputs and checks their checksum.  No GPU.

    python tests/golden/fem_window_grad/make_fem_window_grad_golden.py            # 27 and 34, both reductions
    python tests/golden/fem_window_grad/make_fem_window_grad_golden.py 64         # 64, 'mse' only

Per file: loss64_<kind>, loss32_<kind>, grad64_<kind> [n*n,2] (float64), grad32_<kind> (float32, the fp32 restatement's
own bits), coeffs64 / coeffs32 [n*n], coords_sum = x.double().sum(), for kind in ('mse', 'L2')."""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [TESTS, os.path.dirname(TESTS)]
import fem_restatement as R  # noqa: E402
import modular2d_restatement as M  # noqa: E402
from test_gpu_modular2d import _coords, _params  # noqa: E402

GAUSSIANS, N_LAT_MSE = 2, 101
KINDS = {27: ('mse', 'L2'), 34: ('mse', 'L2'), 64: ('mse',)}       # 64 x 64: one reduction, the rest is minutes each
N_LOSS = {'mse': N_LAT_MSE, 'L2': R.SIMPSON_N}


def make(n):
    x, m = _coords(n, 'jittered', seed=n + 1)
    p = _params(GAUSSIANS, n)
    out = {'n': n, 'gaussians': GAUSSIANS, 'n_lat_mse': N_LAT_MSE, 'n_lat_l2': R.SIMPSON_N,
           'coords_sum': np.float64(x.double().sum().item())}
    for dt, tag, store in ((torch.float64, '64', np.float64), (torch.float32, '32', np.float32)):
        args = (x.to(dt), m.cells, m.boundary_nodes, p['centers'], p['scales'])
        with torch.no_grad():
            A, rhs, _ = M._system(*args, R.SIMPSON_N)
            out['coeffs' + tag] = torch.linalg.solve(A, rhs.unsqueeze(1)).squeeze(1).numpy().astype(store)
        for kind in KINDS[n]:
            t0 = time.time()
            loss, g = M.direct(kind, *args, R.SIMPSON_N, N_LOSS[kind])
            out[f'loss{tag}_{kind}'] = np.float64(loss.double().item())
            out[f'grad{tag}_{kind}'] = g.numpy().astype(store)
            print(f"n={n} {kind} fp{tag}: loss {loss.item():.9e} |g|max {g.abs().max().item():.6e} ({time.time() - t0:.0f} s)", flush=True)
    for kind in KINDS[n]:
        dl = abs(out[f'loss32_{kind}'] - out[f'loss64_{kind}']) / abs(out[f'loss64_{kind}'])
        g64 = out[f'grad64_{kind}']
        dg = np.abs(out[f'grad32_{kind}'].astype(np.float64) - g64).max() / np.abs(g64).max()
        print(f"n={n} {kind}: fp32 restatement's deviation from fp64: loss {dl:.3e} gradient {dg:.3e}", flush=True)
    np.savez_compressed(os.path.join(HERE, f'n{n}.npz'), **out)


if __name__ == '__main__':
    for n in ([int(a) for a in sys.argv[1:]] or [27, 34]):
        make(n)
