"""Golden data of the MMPDE5 target-mesh generator, recorded from the reference's own modules (CPU only).

    python tools/make_mmpde5_golden.py --reference /path/to/g-adaptivity [--out tests/golden/mmpde5] [--only NAME ...]

Loads `classical_meshing/ma_mesh_1d.py` and `ma_mesh_2d.py` from the reference checkout at run time (their Firedrake-side
imports are replaced by empty modules: the MMPDE5 functions need none of them), runs the cases below and writes one
`<name>.npz` per case (in a directory of their own: other tests read every .npz directly under tests/golden): the start coordinates, the two monitor arrays the reference's right-hand side reads (its own
`m` on the half-step grid at the odd indices and on the nodes), the final coordinates, the step count `j` and the wall time
of the reference call.  Nothing of the reference's text is kept: the fixtures hold numbers only.
"""
import argparse
import importlib.util
import os
import sys
import time
import types

import numpy as np
import torch


class _Empty(types.ModuleType):
    __all__ = []

    def __getattr__(self, k):
        if k.startswith('__'):
            raise AttributeError(k)
        return None


def load_reference(root):
    for name in ('firedrake', 'movement', 'firedrake_difFEM', 'firedrake_difFEM.solve_poisson', 'src', 'src.utils_eval'):
        sys.modules.setdefault(name, _Empty(name))
    mods = []
    for fname in ('ma_mesh_1d.py', 'ma_mesh_2d.py'):
        spec = importlib.util.spec_from_file_location('ref_' + fname[:-3], os.path.join(root, 'classical_meshing', fname))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


GAUSS_1D = {'centers': [[0.5]], 'scales': [[0.1]]}
GAUSS_1D_TWO = {'centers': [[0.3], [0.75]], 'scales': [[0.1], [0.15]]}
GAUSS_2D = {'centers': [[0.3, 0.6], [0.7, 0.35]], 'scales': [[0.2, 0.25], [0.15, 0.3]]}

# name -> (kind, N, params)
CASES = {
    '1d_n21_reg0p1': ('1d', 21, dict(GAUSS_1D, mon_power=0.2, mon_reg=0.1)),
    '1d_n21_reg0p01': ('1d', 21, dict(GAUSS_1D, mon_power=0.2, mon_reg=0.01)),
    '1d_n21_power_only': ('1d', 21, dict(GAUSS_1D_TWO, mon_power=0.25)),
    '2d_n11': ('2d', 11, dict(GAUSS_2D, mon_power=0.2)),
    '2d_n15': ('2d', 15, dict(GAUSS_2D, mon_power=0.2)),
    'burgers_n17': ('burgers', 17, {}),
}


def burgers_monitor(x):
    """The callable of the Burgers-form case: a front at x = 0.4 (any positive function of the grid would do)."""
    return (0.1 + 1.0 / torch.cosh((x - 0.4) / 0.1) ** 2) ** 0.2


def burgers_start(n):
    xi = torch.linspace(0, 1, n)
    return xi + 0.35 * xi * (1 - xi) * (0.5 - xi)            # monotone, non-uniform, end points fixed


def _params_arrays(params):
    out = {}
    for k, v in params.items():
        out['param_' + k] = np.asarray(v, dtype=np.float64)
    return out


def run_case(name, ref1d, ref2d):
    kind, n, params = CASES[name]
    lin, fine = torch.linspace(0, 1, n), torch.linspace(0, 1, 2 * n - 1)
    if kind == '2d':
        x0, y0 = torch.meshgrid(lin, lin, indexing='ij')
        xf, yf = torch.meshgrid(fine, fine, indexing='ij')
        ms = ref2d.m(xf, yf, params)[1:2 * n - 1:2, 1:2 * n - 1:2]
        m2 = ref2d.m(x0, y0, params)
        t = time.time()
        x, y, j, _ = ref2d.MMPDE5_2d(x0.clone(), y0.clone(), n, params)
        wall = time.time() - t
        extra = {'y0': y0.numpy(), 'y': y.numpy()}
    elif kind == '1d':
        x0 = lin
        ms = ref1d.m(fine, params)[1:2 * n - 1:2]
        m2 = ref1d.m(lin, params)
        t = time.time()
        x, j, _ = ref1d.MMPDE5_1d(x0.clone(), n, params)
        wall = time.time() - t
        extra = {}
    else:
        x0 = burgers_start(n)
        ms = burgers_monitor(fine)[1:2 * n - 1:2]
        m2 = burgers_monitor(lin)
        t = time.time()
        x, j, _ = ref1d.MMPDE5_1d_burgers(burgers_monitor, x0.clone(), n)
        wall = time.time() - t
        extra = {}
    assert x.dtype == torch.float32 and j < 10000, (name, x.dtype, j)
    out = {'dim': np.int32(2 if kind == '2d' else 1), 'n': np.int32(n), 'x0': x0.numpy(), 'ms': ms.numpy(), 'm2': m2.numpy(),
           'x': x.numpy(), 'j': np.int32(j), 'ref_seconds': np.float64(wall)}
    out.update(extra)
    out.update(_params_arrays(params))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reference', required=True, help='checkout of the reference project')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'mmpde5'))
    ap.add_argument('--only', nargs='*', default=None)
    ap.add_argument('--threads', type=int, default=1)
    args = ap.parse_args()
    torch.set_num_threads(args.threads)
    ref1d, ref2d = load_reference(args.reference)
    for name in args.only or CASES:
        res = run_case(name, ref1d, ref2d)
        path = os.path.join(args.out, f'{name}.npz')
        np.savez(path, **res)
        print(f"{name}: j = {int(res['j'])}, reference wall time {float(res['ref_seconds']):.2f} s -> {os.path.normpath(path)}", flush=True)


if __name__ == '__main__':
    main()
