"""The case table of the strided Monge-Ampere tests (tests/test_ma_strided_host.py, tests/test_gpu_ma_strided.py) and their
restated results, computed once per process and shared (nothing in them is written to afterwards).

  fixed     tol = 0, 300 updates, Gaussians `ma_cases.drawn(1000 + N, g)`; one case per K = ceil(N^2 / 1024) and per edge of it:
            N = 8 (one wave, K = 1), 32 (16 full waves, K = 1), 33 (K = 2, the second slot holds 65 nodes), 45 (K = 2, nearly
            full; one Gaussian, MA2d's default monitor), 46 (K = 3), 64 (K = 4, full), 65 (K = 5; 8 Gaussians), 81 (K = 7)
  route     the lane route's own cases at N = 11 and 32 (`ma_cases`), for the contract between the two routes
  ds33      a seeded `MeshDataset` sample at 33 x 33, run to tol = 1e-4 here (about 10 s of CPU for the three runs)
  ds64      one at 64 x 64: about 30 s of CPU, so its yardstick is the fixture tests/golden/ma_strided/ds64.npz, written by
            tests/golden/ma_strided/make_ma_strided_golden.py

The yardstick is the fp64 restatement (`ma_restatement.ma(dtype=torch.float64)`).  noise = max(|z_mixed - z64|,
|z_mixed' - z_mixed|) with the mixed restatement of `ma_strided_restatement` and its 1 +- 2^-23 monitor perturbation: what the
route's own arithmetic, and an expf / logf / powf that rounds the other way, cost the case.  Nothing the kernel computes
entered a case or a bar.
"""
import functools
import os
from types import SimpleNamespace

import numpy as np
import torch

import ma_cases as K
import ma_restatement as R
import ma_strided_restatement as S

REG, CFL, TOL, PERTURB_SEED = K.REG, K.CFL, K.TOL, K.PERTURB_SEED
UPDATES = 300
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ma_strided', 'ds64.npz')


def _case(N, gaussians, monitor, updates=None):
    return SimpleNamespace(N=N, params=dict(gaussians, **monitor), updates=updates)


def _fixed(N, g, monitor=REG):
    return _case(N, K.drawn(1000 + N, g), monitor, UPDATES)


CASES = {
    'n8_g2': _fixed(8, 2),
    'n32_g2': _fixed(32, 2),
    'n33_g2': _fixed(33, 2),
    'n45_g1': _fixed(45, 1, {}),
    'n46_g2': _fixed(46, 2),
    'n64_g2': _fixed(64, 2),
    'n65_g8': _fixed(65, 8),
    'n81_g2': _fixed(81, 2),
    'route11': K.CASES['n11_g2'],
    'route32': K.CASES['n32_g2'],
}
FIXED = [k for k in CASES if k.startswith('n')]
ROUTE = ['route11', 'route32']


@functools.lru_cache(maxsize=None)
def case(name):
    """CASES plus the two dataset cases, which need the package (and so are built on demand)."""
    if name == 'ds33':
        return _case(33, K.from_dataset(33, 2, 0), REG)
    if name == 'ds64':
        return _case(64, K.from_dataset(64, 0, 0), REG)
    return CASES[name]


def slots(N):
    """K of the strided route: nodes per lane."""
    nodes = N * N
    T = min((nodes + 63) // 64 * 64, 1024)
    return (nodes + T - 1) // T


@functools.lru_cache(maxsize=None)
def fixed64(name, updates=None):
    """(xy, steps, res, status, lmin) of the fp64 restatement after exactly `updates` updates (the case's own by default)."""
    c = case(name)
    return R.ma(c.N, c.params, dtype=torch.float64, cfl=CFL, tol=0.0, max_steps=updates or c.updates)


@functools.lru_cache(maxsize=None)
def fixed_mixed(name, perturbed=False, updates=None):
    c = case(name)
    return S.ma(c.N, c.params, cfl=CFL, tol=0.0, max_steps=updates or c.updates, perturb=PERTURB_SEED if perturbed else None)


def noise_of(z64, zm, zmp):
    return max((zm.double() - z64).abs().max().item(), (zmp.double() - zm.double()).abs().max().item())


@functools.lru_cache(maxsize=None)
def noise(name):
    """(z64, noise) after the case's fixed number of updates.  No stopping decision enters it."""
    z64 = fixed64(name)[0]
    return z64, noise_of(z64, fixed_mixed(name)[0], fixed_mixed(name, True)[0])


@functools.lru_cache(maxsize=None)
def converged64(name):
    c = case(name)
    return R.ma(c.N, c.params, dtype=torch.float64, cfl=CFL, tol=TOL, max_steps=40000)


@functools.lru_cache(maxsize=None)
def converged_mixed(name, perturbed=False):
    """The mixed restatement to tol, and (last entry) its x, y after as many updates as the fp64 run made."""
    c = case(name)
    return S.ma(c.N, c.params, cfl=CFL, tol=TOL, max_steps=40000, perturb=PERTURB_SEED if perturbed else None,
                also_at=converged64(name)[1])


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """What the converged comparisons need: SimpleNamespace(z64, j64, jm, jmp, noise), noise at the fp64 stopping step.
    ds33 is computed here, ds64 read from the fixture."""
    if name == 'ds64':
        f = np.load(GOLDEN)
        c = case(name)
        phi = torch.from_numpy(f['phi64'])
        gx, gy = R.grid(c.N, torch.float64)
        x, y, r, lam = R.evaluate(phi, c.N, gx, gy, *R.inputs(c.params, torch.float64))
        j64, jm, jmp = (int(v) for v in f['steps'])
        return SimpleNamespace(z64=torch.stack([x, y]), j64=j64, jm=jm, jmp=jmp, noise=float(f['noise']))
    z64, j64 = converged64(name)[:2]
    m, mp = converged_mixed(name), converged_mixed(name, True)
    return SimpleNamespace(z64=z64, j64=j64, jm=m[1], jmp=mp[1], noise=noise_of(z64, m[-1], mp[-1]))
