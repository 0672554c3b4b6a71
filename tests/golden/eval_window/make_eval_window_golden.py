#!/usr/bin/env python
"""Writes yardstick.npz: the (L1, L2) error norms of jittered 27 x 27, 34 x 34 and 64 x 64 meshes from the test-side yardstick
(tests/eval_restatement.py: dense solve of all nodes, expansion on the 101 x 101 lattice) in fp64 and in fp32, which
tests/test_gpu_evaluation_window.py compares the windowed route with: 15 s, 24 s and minutes of CPU, too long to repeat in
every run of the suite.  The meshes and the Gaussians are the recipes of tests/test_gpu_modular2d.py
(_coords(n, 'jittered', seed=n + 1), _params(2, n)); the test rebuilds the same inputs and checks their checksum.  No GPU.

    python tests/golden/eval_window/make_eval_window_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [TESTS, os.path.dirname(TESTS)]
import eval_restatement as E  # noqa: E402
from test_gpu_modular2d import _coords, _params  # noqa: E402

SIZES, GAUSSIANS, N_EVAL = (27, 34, 64), 2, 101

if __name__ == '__main__':
    out = {'sizes': np.asarray(SIZES), 'gaussians': GAUSSIANS, 'n_eval': N_EVAL}
    for n in SIZES:
        x, m = _coords(n, 'jittered', seed=n + 1)
        p = _params(GAUSSIANS, n)
        e64 = E.errors_2d(x, m.cells, m.boundary_nodes, p['centers'], p['scales'], N_EVAL, torch.float64)
        e32 = E.errors_2d(x, m.cells, m.boundary_nodes, p['centers'], p['scales'], N_EVAL, torch.float32)
        print(n, 'fp64', e64, 'fp32', e32, flush=True)
        out[f'e64_n{n}'], out[f'e32_n{n}'] = np.asarray(e64, np.float64), np.asarray(e32, np.float64)
        out[f'coords_sum_n{n}'] = np.float64(x.double().sum().item())
    np.savez(os.path.join(HERE, 'yardstick.npz'), **out)
