"""Recorded bits of the seven Monge-Ampere kernels, from the MI355X (tests/golden/ma_routes/ma_routes.npz).

    python tools/make_ma_golden.py [--out tests/golden/ma_routes/ma_routes.npz] [--force]

The fixture was recorded from the build of commit b25be46ae7df0ec10fa23521781ce2fe0dde1f18, the parent of the commit that put
one statement of the shared iteration (mesh_csrc/ma_iteration.h) and one host-side batch check (mesh_csrc/ma_host.h) behind the
kernels: tests/test_gpu_ma_recorded_bits.py asserts that every later build gives the same bits.
The kernels use no atomics and every reduction runs in a fixed order, so equality is exact.  Only the public API is called
(`ma_batch`, `ma_table_batch`).

Seven kernels (KERNELS), three launches each (LAUNCHES):
  cap        a mixed batch, tol = 0, max_steps = 30: every mesh ends as CAP after 30 updates
               lane kernels (ma, M2N fast, table)  sides 3 (one interior node), 5 (no Gaussians: the grid), 8 (exactly one
                                                   wave), 9 (a second wave with 17 nodes), 11, 32 (all 16 waves)
               slow                                sides 3 (one unknown, band 0), 4 (the first real band), 9, 24 (the LDS limit)
               strided kernels                     sides 3, 9, 33 (K = 2, 65 nodes in the last slot), 81 (K = 7: the full select chains)
             0, 1, 2 and 8 Gaussians per mesh (8 fills the constants area; under M2N the last one carries u_xy); tables of
             T = 2, T = N and T = 101 mixed in the batch
  tol        a small batch run to the default tol = 1e-4 under max_steps = 20000: sides 3, 9, 11 (lane), 3, 11 (slow), 9, 33
             (strided); every mesh ends as CONVERGED
  nonconvex  one 9 x 9 mesh that ends as NONCONVEX: cfl = 1 with a narrow Gaussian (ma, M2N fast, M2N slow), a table with the
             entry under node (4, 4) set to 0 (table kernels)
Gaussians are `ma_cases.drawn` with that module's seeds where it has the size.  A table is `rational_table` of the mesh's own
Gaussians: additions, products and quotients of fp64 alone, so it is the same on every machine and is not stored.  What is
stored of the inputs (sides, Gaussians, monitor constants, table sides) the test reads from the fixture.

The fixture has a directory of its own, as the other recorded fixtures have.  An existing fixture is not overwritten without
--force: re-recording it from a build under test proves nothing.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if os.path.abspath(p) not in sys.path:
        sys.path.insert(0, os.path.abspath(p))

DEFAULT_OUT = os.path.join(ROOT, 'tests', 'golden', 'ma_routes', 'ma_routes.npz')
MAX_BYTES = 256 * 1024
KERNELS = ('ma_lane', 'm2n_lane', 'slow', 'table_lane', 'ma_strided', 'm2n_strided', 'table_strided')
LAUNCHES = ('cap', 'tol', 'nonconvex')
CONVERGED, CAP, NONCONVEX = 0, 1, 2
WANTED = {'cap': CAP, 'tol': CONVERGED, 'nonconvex': NONCONVEX}
SOLVER = {'cap': dict(cfl=0.2, tol=0.0, max_steps=30), 'tol': dict(cfl=0.2, tol=1e-4, max_steps=20000),
          'nonconvex': dict(cfl=1.0, tol=1e-4, max_steps=20000)}
TABLE_NONCONVEX = dict(cfl=0.2, tol=1e-4, max_steps=20000)               # the table's zero entry ends it, not the step
NARROW = {'centers': [[0.43, 0.61]], 'scales': [[0.06, 0.08]]}           # ma_cases' narrow11
MA, M2N_LOW, M2N_RUN = (0.01, 0.2, 0.0), (0.01, 1.0, 1.0), (0.1, 1.0, 1.5)   # (mon_reg, mon_power, -) or (mon_reg, alpha, beta)
OUTPUTS = ('coords', 'steps', 'residual', 'status')


def drawn(seed, count):
    """`ma_cases.drawn`."""
    rng = np.random.default_rng(seed)
    centers = [rng.uniform(0.0, 1.0, 2).astype('f') for _ in range(count)]
    scales = [rng.uniform(0.1, 0.5, 2).astype('f') for _ in range(count)]
    return {'centers': centers, 'scales': scales}


NONE = {'centers': [], 'scales': []}
# side -> Gaussians, per route family and launch; (side, Gaussians, table side) where a table kernel reads them
LANE = {'cap': [(3, drawn(3, 1), 2), (5, NONE, 2), (8, drawn(8, 2), 8), (9, drawn(9, 1), 101), (11, drawn(118, 8), 11), (32, drawn(32, 2), 101)],
        'tol': [(3, drawn(3, 1), 2), (9, drawn(9, 1), 9), (11, drawn(11, 2), 101)],
        'nonconvex': [(9, NARROW, 9)]}
SLOW = {'cap': [(3, drawn(3, 1), 0), (4, NONE, 0), (9, drawn(118, 8), 0), (24, drawn(24, 2), 0)],
        'tol': [(3, drawn(3, 1), 0), (11, drawn(11, 2), 0)],
        'nonconvex': [(9, NARROW, 0)]}
STRIDED = {'cap': [(3, drawn(3, 1), 2), (9, NONE, 9), (33, drawn(1033, 2), 101), (81, drawn(1081, 8), 2)],
           'tol': [(9, drawn(9, 1), 101), (33, drawn(1033, 2), 33)],
           'nonconvex': [(9, NARROW, 9)]}
FAMILY = {'ma_lane': LANE, 'm2n_lane': LANE, 'table_lane': LANE, 'slow': SLOW, 'ma_strided': STRIDED, 'm2n_strided': STRIDED,
          'table_strided': STRIDED}


def entries():
    return [f'{k}_{l}' for k in KERNELS for l in LAUNCHES]


def monitor_constants(kernel, b):
    """The monitor's three constants of mesh b: the M2N pairs alternate over the batch, as in tests/ma_m2n_cases.py."""
    if kernel.startswith('ma_') or kernel.startswith('table_'):
        return MA
    return M2N_LOW if b % 2 == 0 else M2N_RUN


def inputs():
    """What the fixture stores of the inputs, per entry: sides [B], Gaussian counts [B], centres and scales [B, 8, 2] (zero
    beyond a mesh's count), the monitor's constants [B, 3] and the table sides [B] (0 where no table is read)."""
    out = {}
    for kernel in KERNELS:
        for launch in LAUNCHES:
            meshes = FAMILY[kernel][launch]
            B = len(meshes)
            centers, scales = np.zeros((B, 8, 2), np.float32), np.zeros((B, 8, 2), np.float32)
            for b, (_, g, _) in enumerate(meshes):
                for k, (c, s) in enumerate(zip(g['centers'], g['scales'])):
                    centers[b, k], scales[b, k] = np.asarray(c, np.float32), np.asarray(s, np.float32)
            e = f'{kernel}_{launch}'
            out[f'{e}_in_sides'] = np.array([m[0] for m in meshes], np.int32)
            out[f'{e}_in_ng'] = np.array([len(m[1]['centers']) for m in meshes], np.int32)
            out[f'{e}_in_centers'], out[f'{e}_in_scales'] = centers, scales
            out[f'{e}_in_mon'] = np.array([monitor_constants(kernel, b) for b in range(B)], np.float32)
            out[f'{e}_in_T'] = np.array([m[2] if kernel.startswith('table_') else 0 for m in meshes], np.int32)
    return out


def rational_table(T, centers, scales, zero=None):
    """1 + sum over the Gaussians of 4 / (1 + ((x - c0) / s0)^2 + ((y - c1) / s1)^2) on the T x T lattice, in fp64 with
    additions, products and quotients alone (each correctly rounded: the same bits everywhere), then one entry set to 0."""
    lin = torch.arange(T, dtype=torch.float64) / (T - 1)
    x, y = torch.meshgrid(lin, lin, indexing='ij')
    m = torch.ones_like(x)
    for c, s in zip(centers, scales):
        dx, dy = (x - float(c[0])) / float(s[0]), (y - float(c[1])) / float(s[1])
        m = m + 4.0 / ((1.0 + dx * dx) + dy * dy)
    if zero is not None:
        m[zero] = 0.0
    return m


def mesh_params(kernel, inp, e, b):
    ng = int(inp[f'{e}_in_ng'][b])
    p = {'centers': [list(map(float, c)) for c in inp[f'{e}_in_centers'][b][:ng]],
         'scales': [list(map(float, s)) for s in inp[f'{e}_in_scales'][b][:ng]]}
    c0, c1, c2 = (float(v) for v in inp[f'{e}_in_mon'][b])
    if kernel.startswith('ma_'):
        return dict(p, mon_reg=c0, mon_power=c1)
    if kernel == 'slow':
        return dict(p, mesh_type='M2N', fast_M2N_monitor='slow', mon_reg=c0, M2N_alpha=c1, M2N_beta=c2)
    return dict(p, mesh_type='M2N', fast_M2N_monitor='fast', mon_reg=c0, M2N_beta=c2)


def run(kernel, launch, inp, dev):
    """One entry's launch through the public API -> the result tuple."""
    from g_adaptivity_amd.monge_ampere import ma_batch, ma_table_batch
    e = f'{kernel}_{launch}'
    sides = [int(n) for n in inp[f'{e}_in_sides']]
    route = 'strided' if kernel.endswith('_strided') else 'lane'
    if kernel.startswith('table_'):
        tables = [rational_table(int(T), inp[f'{e}_in_centers'][b][:int(inp[f'{e}_in_ng'][b])], inp[f'{e}_in_scales'][b],
                                 (4, 4) if launch == 'nonconvex' else None) for b, T in enumerate(inp[f'{e}_in_T'])]
        return ma_table_batch(sides, tables, route=route, device=dev, **(TABLE_NONCONVEX if launch == 'nonconvex' else SOLVER[launch]))
    params = [mesh_params(kernel, inp, e, b) for b in range(len(sides))]
    return ma_batch(sides, params, route=route, device=dev, m2n_solve='p1' if kernel == 'slow' else None, **SOLVER[launch])


def compute(inp, dev):
    """Every recorded result from the stored inputs, as a dict of numpy arrays named '<kernel>_<launch>_<what>'; coords (and
    the slow kernel's monitor) are the meshes' [2, N, N] ([N, N]) arrays flattened and joined in batch order."""
    out = {}
    for kernel in KERNELS:
        for launch in LAUNCHES:
            res, e = run(kernel, launch, inp, dev), f'{kernel}_{launch}'
            out[f'{e}_coords'] = torch.cat([c.reshape(-1) for c in res.coords])
            out[f'{e}_steps'], out[f'{e}_residual'], out[f'{e}_status'] = res.steps, res.residual, res.status
            if kernel == 'slow':
                out[f'{e}_monitor'] = torch.cat([m.reshape(-1) for m in res.monitor])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def names():
    return [f'{e}_{w}' for e in entries() for w in OUTPUTS + (('monitor',) if e.startswith('slow_') else ())]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=DEFAULT_OUT)
    ap.add_argument('--force', action='store_true', help='overwrite an existing fixture')
    args = ap.parse_args()
    if os.path.exists(args.out) and not args.force:
        sys.exit(f"{os.path.normpath(args.out)} exists; --force overwrites it (only from a build that is not under test)")
    assert torch.cuda.is_available(), "the fixture is recorded on the MI355X"
    inp = inputs()
    res = compute(inp, torch.device('cuda:0'))
    assert sorted(res) == sorted(names())
    for kernel in KERNELS:
        for launch in LAUNCHES:
            e = f'{kernel}_{launch}'
            print(f"  {e:24s} sides {inp[f'{e}_in_sides'].tolist()} steps {res[f'{e}_steps'].tolist()} status {res[f'{e}_status'].tolist()} "
                  f"residual {res[f'{e}_residual'].tolist()}")
            assert (res[f'{e}_status'] == WANTED[launch]).all(), f"{e}: status {res[f'{e}_status'].tolist()}, {WANTED[launch]} wanted"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **inp, **res)
    size = os.path.getsize(args.out)
    print(f"{len(res)} arrays, {size} bytes -> {os.path.normpath(args.out)}")
    assert size <= MAX_BYTES, f"{size} bytes; the fixture stays at or below {MAX_BYTES}"


if __name__ == '__main__':
    main()
