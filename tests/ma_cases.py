"""The case table of the Monge-Ampere tests (tests/test_ma_host.py, tests/test_gpu_ma.py) and their restated results, computed
once per process and shared (nothing in them is written to afterwards).

Gaussians are drawn as `attach_random_fields` draws them: centres in U(0, 1)^2, scales in U(0.1, 0.5)^2, rounded to fp32.  The
seeds were chosen so that the fp64 restatement ALONE meets the conditions test_ma_host.py states for every case (it converges,
stays convex, keeps every triangle's orientation and brings the cell spread to at most half the uniform grid's); nothing
the kernel computes entered the choice.

  fixed     N = 3 (one interior node), 8 (exactly one wave), 9 (a wave plus 17 lanes), 11, 32 (16 full waves); 1 or 2
            Gaussians, one case with 8; `updates` is the step count of the tol = 0 comparison
  dataset   the Gaussians of a seeded `MeshDataset` sample at 11 x 11 and 15 x 15: the converged comparisons
  sym11     one centred Gaussian with equal scales: x = y^T and x mirrors
  narrow11  one Gaussian narrower than a cell: the status paths.  With cfl = 1 its first update already breaks convexity (the
            restatement's min lambda is -0.167 at the second evaluation, in fp32 and fp64); the cases above, with scales of
            0.1 to 0.5, lose it a few updates later
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import ma_restatement as R
from g_adaptivity_amd import MeshDataset

REG = {'mon_reg': 0.01, 'mon_power': 0.2}                 # the reference's 2-D run parameters; {} is MA2d's default monitor
CFL, TOL = 0.2, 1e-4


def drawn(seed, count):
    rng = np.random.default_rng(seed)
    centers = [rng.uniform(0.0, 1.0, 2).astype('f') for _ in range(count)]
    scales = [rng.uniform(0.1, 0.5, 2).astype('f') for _ in range(count)]
    return {'centers': centers, 'scales': scales}


def from_dataset(N, seed, index):
    return dict(MeshDataset([N, N], index + 1, seed=seed).samples[index].pde_params)


def _case(N, gaussians, monitor, updates=None):
    return SimpleNamespace(N=N, params=dict(gaussians, **monitor), updates=updates)


CASES = {
    'n3_g1': _case(3, drawn(3, 1), REG, 200),
    'n8_g2': _case(8, drawn(8, 2), REG, 200),
    'n9_g1': _case(9, drawn(9, 1), {}, 200),
    'n11_g2': _case(11, drawn(11, 2), REG, 200),
    'n11_g8': _case(11, drawn(118, 8), REG, 200),
    'n32_g2': _case(32, drawn(32, 2), REG, 500),
    'ds11': _case(11, from_dataset(11, 0, 0), REG),
    'ds15': _case(15, from_dataset(15, 1, 1), REG),
    'sym11': _case(11, {'centers': [[0.5, 0.5]], 'scales': [[0.25, 0.25]]}, REG),
    'narrow11': _case(11, {'centers': [[0.43, 0.61]], 'scales': [[0.06, 0.08]]}, REG),
}
FIXED = [k for k, c in CASES.items() if c.updates]
CONVERGING = ['ds11', 'ds15']
PERTURB_SEED = 2024

_DTYPES = {'fp64': torch.float64, 'fp32': torch.float32}


@functools.lru_cache(maxsize=None)
def converged(name, precision, perturbed=False):
    """(xy, steps, res, status, lmin) of the restatement run to tol = 1e-4."""
    c = CASES[name]
    return R.ma(c.N, c.params, dtype=_DTYPES[precision], cfl=CFL, tol=TOL, perturb=PERTURB_SEED if perturbed else None)


@functools.lru_cache(maxsize=None)
def fixed(name, precision, perturbed=False, updates=None):
    """The same after exactly `updates` updates (tol = 0); the case's own count unless one is given."""
    c = CASES[name]
    return R.ma(c.N, c.params, dtype=_DTYPES[precision], cfl=CFL, tol=0.0, max_steps=updates or c.updates,
                perturb=PERTURB_SEED if perturbed else None)


def noise(name, updates=None):
    """(z64, max(|z32 - z64|, |z32' - z32|)) after a fixed number of updates: what fp32 arithmetic, and an expf / logf / powf
    that rounds the monitor the other way, cost this case.  No stopping decision enters it."""
    z64, z32, z32p = fixed(name, 'fp64', False, updates)[0], fixed(name, 'fp32', False, updates)[0], fixed(name, 'fp32', True, updates)[0]
    return z64, max((z32.double() - z64).abs().max().item(), (z32p.double() - z32.double()).abs().max().item())
