"""The case table of the tabulated-monitor Monge-Ampere tests (tests/test_ma_table_host.py, tests/test_gpu_ma_table.py) and their
restated results, computed once per process and shared (nothing in them is written to afterwards).

Every case is (N, a table, an update count); the table is what the kernel gets, built here on the CPU in fp64 and rounded to
fp32 by the callers.  Gaussians are `ma_cases.drawn(seed, count)` with the seeds of `ma_cases` / `ma_strided_cases`, monitors
carry `ma_cases.REG` (mon_reg = 0.01, mon_power = 0.2).

  sizes     lane: N = 3 (one interior node), 8 (exactly one wave), 9 (a wave plus 17 lanes), 11, 32 (16 full waves);
            strided: N = 11, 32 (K = 1), 33 (K = 2), 81 (K = 7); `ma_strided_cases.UPDATES` = 300 updates at 32 and above
  tables    T = 2, T = N, T = 17 on N = 11 (unrelated sizes), T = 101
  monitors  `monitor_table` of one and of two Gaussians; `monitor_from_nodal` of the same u (the sum of the Gaussians on the
            lattice); the linear table 1 + x + 2 y; the constant table (test by test: it makes no update)
  ds11, ds15  the Gaussians of `ma_cases`' dataset cases with T = 33: the converged comparisons
  sym11     one centred Gaussian with equal scales, T = 33 (the lattice is symmetric too)

The yardstick is the fp64 restatement (`ma_table_restatement.ma(arith='fp64')`).  `noise` is defined as in `ma_cases.noise`:
max(|z - z64|, |z' - z|) with z the restatement in the route's own arithmetic and z' the same with the monitor rounded the
other way at every node and step.  Nothing the kernels compute entered a case or a bar.
"""
import functools
from types import SimpleNamespace

import torch

import ma_cases as K
import ma_strided_cases as SK
import ma_table_restatement as TR
from g_adaptivity_amd.monge_ampere import monitor_from_nodal, monitor_table

REG, CFL, TOL, PERTURB_SEED = K.REG, K.CFL, K.TOL, K.PERTURB_SEED
UPDATES = SK.UPDATES
ARITH_OF_ROUTE = {'lane': 'fp32', 'strided': 'mixed'}
ROUTES = ('lane', 'strided')


def lattice(T, dtype=torch.float64):
    lin = torch.arange(T, dtype=dtype) / (T - 1)
    return torch.meshgrid(lin, lin, indexing='ij')


def analytic(gaussians, T):
    """`monitor_table` of the Gaussians with REG."""
    return monitor_table(dict(gaussians, **REG), T)


def nodal(gaussians, T):
    """`monitor_from_nodal` of u = the sum of the Gaussians on the T x T lattice, with REG."""
    x, y = lattice(T)
    u = torch.zeros_like(x)
    for c, s in zip(gaussians['centers'], gaussians['scales']):
        u = u + torch.exp(-(x - float(c[0])) ** 2 / float(s[0]) ** 2 - (y - float(c[1])) ** 2 / float(s[1]) ** 2)
    return monitor_from_nodal(u, **REG)


def linear(T):
    x, y = lattice(T)
    return 1.0 + x + 2.0 * y


def constant(T, value=1.5):
    return torch.full((T, T), value, dtype=torch.float64)


def _case(N, table, updates=None, routes=ROUTES, params=None):
    return SimpleNamespace(N=N, table=table, T=table.shape[0], updates=updates, routes=routes, params=params)


CASES = {
    'n3_t2_lin': _case(3, linear(2), 200, ('lane',)),
    'n8_tN_g2': _case(8, analytic(K.drawn(8, 2), 8), 200, ('lane',)),
    'n9_t101_g1': _case(9, analytic(K.drawn(9, 1), 101), 200, ('lane',)),
    'n11_t17_g2': _case(11, analytic(K.drawn(11, 2), 17), 200),
    'n11_tN_nodal2': _case(11, nodal(K.drawn(11, 2), 11), 200),
    'n11_t101_nodal1': _case(11, nodal(K.drawn(9, 1), 101), 200),
    'n11_t2_lin': _case(11, linear(2), 200),
    'n32_t101_g2': _case(32, analytic(K.drawn(32, 2), 101), UPDATES),
    'n32_tN_nodal2': _case(32, nodal(K.drawn(32, 2), 32), UPDATES),
    'n33_t17_g2': _case(33, analytic(K.drawn(1033, 2), 17), UPDATES, ('strided',)),
    'n33_tN_nodal2': _case(33, nodal(K.drawn(1033, 2), 33), UPDATES, ('strided',)),
    'n81_t101_g2': _case(81, analytic(K.drawn(1081, 2), 101), UPDATES, ('strided',)),
    'n81_t2_lin': _case(81, linear(2), UPDATES, ('strided',)),
}
FIXED = [(n, r) for n, c in CASES.items() for r in c.routes]
CONVERGING = ['ds11', 'ds15']
CONVERGING_T = 33


@functools.lru_cache(maxsize=None)
def case(name):
    """CASES plus those that need a dataset sample (built on demand): params are the analytic monitor's, for `cell_spread`."""
    if name in ('ds11', 'ds15', 'sym11'):
        c = K.CASES[name]
        return _case(c.N, monitor_table(c.params, CONVERGING_T), params=c.params)
    return CASES[name]


def slots(N):
    return SK.slots(N)


@functools.lru_cache(maxsize=None)
def converged(name, arith, perturbed=False, also_at=None):
    """(xy, steps, res, status, lmin, xy_at) of the restatement run to tol = 1e-4."""
    c = case(name)
    return TR.ma(c.N, c.table, arith=arith, cfl=CFL, tol=TOL, perturb=PERTURB_SEED if perturbed else None, also_at=also_at)


@functools.lru_cache(maxsize=None)
def fixed(name, arith, perturbed=False, updates=None):
    """The same after exactly `updates` updates (tol = 0); the case's own count unless one is given."""
    c = case(name)
    return TR.ma(c.N, c.table, arith=arith, cfl=CFL, tol=0.0, max_steps=updates or c.updates, perturb=PERTURB_SEED if perturbed else None)


@functools.lru_cache(maxsize=None)
def noise(name, route='lane', updates=None):
    """(z64, max(|z - z64|, |z' - z|)) after a fixed number of updates: what the route's arithmetic, and a logf or an
    interpolation that rounds the monitor the other way, cost this case.  No stopping decision enters it."""
    a = ARITH_OF_ROUTE[route]
    z64, z, zp = fixed(name, 'fp64', False, updates)[0], fixed(name, a, False, updates)[0], fixed(name, a, True, updates)[0]
    return z64, max((z.double() - z64).abs().max().item(), (zp.double() - z.double()).abs().max().item())
