"""The case table of the M2N 'slow' monitor tests (tests/test_ma_m2n_slow_host.py, tests/test_gpu_ma_m2n_slow.py) and their restated
results, computed once per process and shared (nothing in them is written to afterwards).  It mirrors tests/ma_m2n_cases.py.

Gaussians are drawn as `ma_cases.drawn` draws them.  THE SEEDS WERE CHOSEN FROM THE fp64 RESTATEMENT ALONE
(tests/ma_m2n_slow_restatement.py): it keeps every fixed-count case convex and brings the converging cases to tol with every
triangle's orientation kept; nothing a kernel computes entered the choice.  They are the seeds of tests/ma_m2n_cases.py where
that table has the size; 16, 23 and 24 a side are new here and took the first seed tried, their own side.

Two parameter triples (mon_reg, alpha, beta): LOW = (0.01, 1.0, 1.0) and RUN = (0.1, 1.0, 1.5), the pairs of ma_m2n_cases with
alpha 1, the reference's default.

  fixed       N = 3 (one interior node, no rank-1 update), 8 (exactly one wave), 9 (a wave plus 17 lanes), 11 with 2 and with 8
              Gaussians, 16 (four full waves), 23 (the reference's largest mesh), 24 (the limit: 9 full waves, 60 944 bytes of
              LDS); `updates` is the step count of the tol = 0 comparison
  converging  the Gaussians of a seeded `MeshDataset` sample at 11 x 11 and 15 x 15 with RUN
  sym11       one centred Gaussian with equal scales.  The cut of every quad joins v1 and v3, so the triangulation, and with it E,
              maps to itself under (i, j) -> (j, i) and under the point reflection, not under a mirror in one direction:
              x = y^T and x = 1 - x reflected in both directions hold, `x mirrors` of the 'fast' table does not
  nonconvex15 the two Gaussians of ma_m2n_cases' nonconvex15 with LOW.  Under 'slow' cfl = 0.2 keeps them convex; NONCONVEX_CFL =
              0.5 loses convexity at the first update (min lambda -1.04 at the second evaluation, in fp32 and fp64 alike), and
              cfl = 0.05 runs on: NONCONVEX means "lower cfl"
"""
import functools
from types import SimpleNamespace

import ma_cases as K
import ma_m2n_restatement as M
import ma_m2n_slow_restatement as S

from g_adaptivity_amd import _native_mesh

CFL, TOL, PERTURB_SEED = K.CFL, K.TOL, K.PERTURB_SEED
MAX_SIDE = _native_mesh.MA_M2N_SLOW_MAX_SIDE
SLOW = {'mesh_type': 'M2N', 'fast_M2N_monitor': 'slow'}
LOW = dict(SLOW, mon_reg=0.01, M2N_alpha=1.0, M2N_beta=1.0)
RUN = dict(SLOW, mon_reg=0.1, M2N_alpha=1.0, M2N_beta=1.5)


def _case(N, gaussians, monitor, updates=None):
    return SimpleNamespace(N=N, params=dict(gaussians, **monitor), updates=updates)


CASES = {
    'n3_g1': _case(3, K.drawn(3, 1), LOW, 200),
    'n8_g2': _case(8, K.drawn(8, 2), RUN, 200),
    'n9_g1': _case(9, K.drawn(9, 1), LOW, 200),
    'n11_g2': _case(11, K.drawn(11, 2), RUN, 200),
    'n11_g8': _case(11, K.drawn(118, 8), LOW, 200),
    'n16_g2': _case(16, K.drawn(16, 2), RUN, 150),
    'n23_g2': _case(23, K.drawn(23, 2), LOW, 100),
    'nmax_g2': _case(MAX_SIDE, K.drawn(MAX_SIDE, 2), RUN, 60),
    'ds11': _case(11, K.from_dataset(11, 0, 0), RUN),
    'ds15': _case(15, K.from_dataset(15, 1, 1), RUN),
    'sym11': _case(11, {'centers': [[0.5, 0.5]], 'scales': [[0.25, 0.25]]}, RUN),
    'nonconvex15': _case(15, K.drawn(15, 2), LOW),
}
FIXED = [k for k, c in CASES.items() if c.updates]
CONVERGING = ['ds11', 'ds15']
NONCONVEX_CFL = 0.5


def fast_params(params):
    """The same Gaussians, mon_reg and beta under the 'fast' monitor."""
    return dict({k: v for k, v in params.items() if k != 'M2N_alpha'}, fast_M2N_monitor='fast')


_AT_FP64_STEP = {}


@functools.lru_cache(maxsize=None)
def converged(name, arith, perturbed=False):
    """(xy, steps, res, status, lmin, m) of the restatement run to tol = 1e-4.  An fp32 run is also read off at the fp64 run's
    stopping step, for `noise` there: one trajectory, not two."""
    c = CASES[name]
    at = None if arith == 'fp64' else converged(name, 'fp64')[1]
    out = S.ma(c.N, c.params, arith=arith, cfl=CFL, tol=TOL, perturb=PERTURB_SEED if perturbed else None, also_at=at)
    _AT_FP64_STEP[name, arith, perturbed] = out[6]
    return out[:6]


@functools.lru_cache(maxsize=None)
def fixed(name, arith, perturbed=False, updates=None):
    """The same after exactly `updates` updates (tol = 0); the case's own count unless one is given."""
    c = CASES[name]
    return S.ma(c.N, c.params, arith=arith, cfl=CFL, tol=0.0, max_steps=c.updates if updates is None else updates,
                perturb=PERTURB_SEED if perturbed else None)[:6]


def mesh_after(name, arith, perturbed=False, updates=None):
    """The restated mesh after exactly `updates` updates (tol = 0).  At the fp64 stopping step of a converging case it is read off
    the converged runs' own trajectories (a stopping test only ends a trajectory), so nothing is run twice."""
    if updates is not None and CASES[name].updates is None and converged(name, 'fp64')[1] == updates:
        converged(name, arith, perturbed)
        return _AT_FP64_STEP[name, arith, perturbed]
    return fixed(name, arith, perturbed, updates)[0]


@functools.lru_cache(maxsize=None)
def noise(name, updates=None):
    """(z64, max(|z32 - z64|, |z32' - z32|)) after a fixed number of updates, z32 the restatement in fp32 and z32' the same with
    the monitor perturbed.  No stopping decision enters it."""
    z64, z, zp = mesh_after(name, 'fp64', False, updates), mesh_after(name, 'fp32', False, updates), mesh_after(name, 'fp32', True, updates)
    return z64, max((z.double() - z64).abs().max().item(), (zp.double() - z.double()).abs().max().item())


@functools.lru_cache(maxsize=None)
def gap_to_fast(name, updates=None):
    """max |z_slow - z_fast| of the two fp64 restatements after the same number of updates with the same Gaussians, mon_reg and
    beta: how far a kernel that ignored E would be from the yardstick."""
    c = CASES[name]
    z_fast = M.ma(c.N, fast_params(c.params), arith='fp64', cfl=CFL, tol=0.0, max_steps=c.updates if updates is None else updates)[0]
    return (mesh_after(name, 'fp64', False, updates) - z_fast).abs().max().item()


@functools.lru_cache(maxsize=None)
def monitor_noise(name):
    """(m64, |m32 - m64| max) of the restated monitor on the uniform grid: 0 updates."""
    m64, m32 = fixed(name, 'fp64', False, 0)[5], fixed(name, 'fp32', False, 0)[5]
    return m64, (m32.double() - m64).abs().max().item()
