#!/usr/bin/env python
"""Writes n26.npz and n81.npz: the test-side restatement (tests/modular2d_restatement.py: dense solve of all nodes) on jittered
meshes at the two documented size limits of the 2-D FEM tail, 26 x 26 (band='lds') and 81 x 81 (band='window'), in fp64 and
in fp32, which tests/test_gpu_fem_orderings.py compares both routes with.  The meshes and the Gaussians are the recipes of
tests/test_gpu_modular2d.py (_coords(n, 'jittered', seed=n + 1), _params(2, n)); the test rebuilds the same inputs and
checks their checksum.  No GPU.  Prints its run time and the fp32 restatement's deviation from fp64 per quantity.

    python tests/golden/fem_limits/make_fem_limits_golden.py            # both
    python tests/golden/fem_limits/make_fem_limits_golden.py 26         # one

n26.npz: coeffs64 [n*n] (float64), coeffs32 (float32, the fp32 restatement's own bits), loss64_mse, loss32_mse, grad64_mse
[n*n,2] (float64), grad32_mse (float32): the 'mse' loss on the 101 x 101 lattice with autograd through the dense solve.
n81.npz: coeffs64, coeffs32, loss64_mse, loss32_mse only: one dense solve of the 6561-square system per precision under
no_grad (no autograd graph through it), so the gradient at this size has no fp64 reference."""
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
WITH_GRADIENT = {26: True, 81: False}


def make(n):
    t_all = time.time()
    x, m = _coords(n, 'jittered', seed=n + 1)
    p = _params(GAUSSIANS, n)
    out = {'n': n, 'gaussians': GAUSSIANS, 'n_lat_mse': N_LAT_MSE, 'coords_sum': np.float64(x.double().sum().item())}
    for dt, tag, store in ((torch.float64, '64', np.float64), (torch.float32, '32', np.float32)):
        t0 = time.time()
        args = (x.to(dt), m.cells, m.boundary_nodes, p['centers'], p['scales'])
        with torch.no_grad():
            A, rhs, cells = M._system(*args, R.SIMPSON_N)
            c = torch.linalg.solve(A, rhs.unsqueeze(1)).squeeze(1)
            del A
            out['coeffs' + tag] = c.numpy().astype(store)
            if not WITH_GRADIENT[n]:
                pts = M.grid(N_LAT_MSE, dt)
                loss = torch.nn.functional.mse_loss(M.expand(c, pts, args[0], cells), R.u_true(pts, p['centers'], p['scales']))
        if WITH_GRADIENT[n]:
            loss, g = M.direct('mse', *args, R.SIMPSON_N, N_LAT_MSE)
            out[f'grad{tag}_mse'] = g.numpy().astype(store)
        out[f'loss{tag}_mse'] = np.float64(loss.double().item())
        print(f"n={n} mse fp{tag}: loss {loss.item():.9e} ({time.time() - t0:.0f} s)", flush=True)
    c64 = out['coeffs64']
    dc = np.abs(out['coeffs32'].astype(np.float64) - c64).max() / np.abs(c64).max()
    dl = abs(out['loss32_mse'] - out['loss64_mse']) / abs(out['loss64_mse'])
    line = f"n={n}: fp32 restatement's deviation from fp64: coeffs {dc:.3e} mse loss {dl:.3e}"
    if WITH_GRADIENT[n]:
        g64 = out['grad64_mse']
        line += f" mse gradient {np.abs(out['grad32_mse'].astype(np.float64) - g64).max() / np.abs(g64).max():.3e}"
    print(line, flush=True)
    np.savez_compressed(os.path.join(HERE, f'n{n}.npz'), **out)
    print(f"n={n}: {time.time() - t_all:.0f} s in all, {os.path.getsize(os.path.join(HERE, f'n{n}.npz'))} B", flush=True)


if __name__ == '__main__':
    for n in ([int(a) for a in sys.argv[1:]] or [26, 81]):
        make(n)
