"""The case table of the M2N-monitor Monge-Ampere tests (tests/test_ma_m2n_host.py, tests/test_gpu_ma_m2n.py) and their restated
results, computed once per process and shared (nothing in them is written to afterwards).  It mirrors tests/ma_cases.py.

Gaussians are drawn as `ma_cases.drawn` draws them, with that table's seeds.  THE SEEDS WERE CHOSEN FROM THE fp64 RESTATEMENT
ALONE (tests/ma_m2n_restatement.py): it keeps every fixed-count case convex, and brings the converging cases to tol with every
triangle's orientation kept and the cell spread at most half the uniform grid's; nothing a kernel computes entered the choice.

Two parameter pairs (mon_reg, beta): LOW = (0.01, 1.0), a monitor contrast of 100, and RUN = (0.1, 1.5), the reference's run
parameters' mon_reg with its default beta.

  fixed       N = 3 (one interior node), 8 (exactly one wave), 9 (a wave plus 17 lanes), 11, 32 (16 full waves); 1, 2 and 8
              Gaussians, the pairs alternating; `updates` is the step count of the tol = 0 comparison (200; 500 at 32)
  strided     fixed counts beyond the lane route: 33 (K = 2 nodes per lane, 300 updates), 64 (K = 4, 200), 81 (K = 7, 100);
              Gaussians `ma_cases.drawn(1000 + N, 2)` as in tests/ma_strided_cases.py.  Fixed counts only: the CPU side stays
              at seconds
  converging  the Gaussians of a seeded `MeshDataset` sample at 11 x 11 and 15 x 15 with RUN
  sym11       one centred Gaussian with equal scales: x = y^T and x mirrors (its u_xy is antisymmetric under either, F is not)
  nonconvex15 two Gaussians on 15 x 15 with mon_reg = 0.01: cfl = 0.2 loses convexity at the first update (min lambda -0.18 at
              the second evaluation, in fp32 and fp64 alike): NONCONVEX means "lower cfl"
"""
import functools
from types import SimpleNamespace

import ma_cases as K
import ma_m2n_restatement as M

CFL, TOL, PERTURB_SEED = K.CFL, K.TOL, K.PERTURB_SEED
M2N = {'mesh_type': 'M2N', 'fast_M2N_monitor': 'fast'}
LOW = dict(M2N, mon_reg=0.01, M2N_beta=1.0)
RUN = dict(M2N, mon_reg=0.1, M2N_beta=1.5)


def _case(N, gaussians, monitor, updates=None):
    return SimpleNamespace(N=N, params=dict(gaussians, **monitor), updates=updates)


CASES = {
    'n3_g1': _case(3, K.drawn(3, 1), LOW, 200),
    'n8_g2': _case(8, K.drawn(8, 2), RUN, 200),
    'n9_g1': _case(9, K.drawn(9, 1), LOW, 200),
    'n11_g2': _case(11, K.drawn(11, 2), RUN, 200),
    'n11_g8': _case(11, K.drawn(118, 8), LOW, 200),
    'n32_g2': _case(32, K.drawn(32, 2), RUN, 500),
    'n33_g2': _case(33, K.drawn(1033, 2), RUN, 300),
    'n64_g2': _case(64, K.drawn(1064, 2), LOW, 200),
    'n81_g2': _case(81, K.drawn(1081, 2), RUN, 100),
    'ds11': _case(11, K.from_dataset(11, 0, 0), RUN),
    'ds15': _case(15, K.from_dataset(15, 1, 1), RUN),
    'sym11': _case(11, {'centers': [[0.5, 0.5]], 'scales': [[0.25, 0.25]]}, RUN),
    'nonconvex15': _case(15, K.drawn(15, 2), LOW),
}
FIXED = [k for k, c in CASES.items() if c.updates and c.N <= 32]           # both routes
FIXED_STRIDED = [k for k, c in CASES.items() if c.updates and c.N > 32]     # route='strided' only
CONVERGING = ['ds11', 'ds15']
ARITH_OF_ROUTE = {'lane': 'fp32', 'strided': 'mixed'}


def slots(N):
    """K of the strided route: nodes per lane."""
    nodes = N * N
    T = min((nodes + 63) // 64 * 64, 1024)
    return (nodes + T - 1) // T


@functools.lru_cache(maxsize=None)
def converged(name, arith, perturbed=False):
    """(xy, steps, res, status, lmin) of the restatement run to tol = 1e-4."""
    c = CASES[name]
    return M.ma(c.N, c.params, arith=arith, cfl=CFL, tol=TOL, perturb=PERTURB_SEED if perturbed else None)


@functools.lru_cache(maxsize=None)
def fixed(name, arith, perturbed=False, updates=None):
    """The same after exactly `updates` updates (tol = 0); the case's own count unless one is given."""
    c = CASES[name]
    return M.ma(c.N, c.params, arith=arith, cfl=CFL, tol=0.0, max_steps=updates or c.updates, perturb=PERTURB_SEED if perturbed else None)


@functools.lru_cache(maxsize=None)
def noise(name, route, updates=None):
    """(z64, max(|z - z64|, |z' - z|)) after a fixed number of updates, z the restatement in the route's arithmetic and z' the
    same with the monitor perturbed: what the route's arithmetic, and an expf / logf / sqrtf or a quotient that rounds the other
    way, cost this case.  No stopping decision enters it."""
    a = ARITH_OF_ROUTE[route]
    z64, z, zp = fixed(name, 'fp64', False, updates)[0], fixed(name, a, False, updates)[0], fixed(name, a, True, updates)[0]
    return z64, max((z.double() - z64).abs().max().item(), (zp.double() - z.double()).abs().max().item())
