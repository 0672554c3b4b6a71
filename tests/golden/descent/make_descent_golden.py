"""Records the CPU restatement runs that tests/test_gpu_descent.py compares against (tests/descent_restatement.py, fp32 and
fp64) in tests/golden/descent/descent.npz, with the inputs they ran on.  Run from the repository root:
    python tests/golden/descent/make_descent_golden.py
It refuses to record a 2-D parity case whose fp64 run tangles."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))
import descent_restatement as D  # noqa: E402

out = {}
for n in D.PARITY_2D['sizes']:
    x0, m, p = D.parity_case_2d(n)
    out[f'p2d_{n}_x0'] = x0.numpy()
    for tag, dt in (('32', torch.float32), ('64', torch.float64)):
        r = D.descend_2d(x0, m.cells, m.boundary_nodes, p['centers'], p['scales'], D.PARITY_2D['epochs'], D.PARITY_2D['lr'], dt)
        for k in ('x', 'coeffs', 'loss'):
            out[f'p2d_{n}_{k}{tag}'] = r[k].numpy()
        if dt == torch.float64:
            areas = [D.min_signed_area(mm, m.cells, x0).item() for mm in r['meshes']]
            assert min(areas) > 0, f"{n} x {n}: the fp64 descent tangles ({areas}); lower the Gaussians' sharpness"
            print(f"2-D {n} x {n}: min oriented determinant per epoch, in uniform cells: {[a * (n - 1) ** 2 for a in areas]}")

xs, params = D.case_1d()
c = D.CASE_1D
for x0, p, n in zip(xs, params, c['sizes']):
    out[f'p1d_{n}_x0'] = x0.numpy()
    for tag, dt in (('32', torch.float32), ('64', torch.float64)):
        r = D.descend_1d(x0, p, c['opt'], c['epochs'], c['lr'], dt)
        for k in ('x', 'coeffs', 'loss', 'sol'):
            out[f'p1d_{n}_{k}{tag}'] = r[k].numpy()
        if dt == torch.float64:
            assert bool((r['meshes'][:, 1:] > r['meshes'][:, :-1]).all()), f"1-D {n}: the fp64 descent crosses"
a = D.CASE_1D_ALL
for tag, dt in (('32', torch.float32), ('64', torch.float64)):
    r = D.descend_1d(torch.linspace(0, 1, a['n']), params[1], c['opt'], a['epochs'], a['lr'], dt, mesh_params='all')
    for k in ('x', 'loss'):
        out[f'all1d_{k}{tag}'] = r[k].numpy()
np.savez_compressed(os.path.join(HERE, 'descent.npz'), **out)
print('wrote', os.path.join(HERE, 'descent.npz'), len(out), 'arrays')
