"""Recorded restatement results for the converged-run test of the strided MMPDE5 route (tests/test_gpu_mmpde5_strided.py).

    python tools/make_mmpde5_strided_golden.py [--out tests/golden/mmpde5_strided]

Runs the CPU restatement (tests/mmpde5_restatement.py) in fp32 and fp64 on one 33 x 33 case, to convergence, and writes
`2d_n33_cfl0p5.npz`: the start mesh, the two monitor arrays, the solver arguments, the stopping steps `j32` / `j64`, the fp64
coordinates `z64` at their own stop and `err32` = max |z32 - z64|.  About 9 s of CPU; the test reads the file and runs only
the GPU.  Nothing but this project's own code is involved.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))
import mmpde5_restatement as R  # noqa: E402

from g_adaptivity_amd.mmpde5 import monitor_2d, monitor_arrays_2d  # noqa: E402

N = 33
PARAMS = {'centers': [[0.3, 0.6], [0.7, 0.4]], 'scales': [[0.2, 0.25], [0.3, 0.15]]}      # the default monitor: mon_power 0.2
SOLVER = {'cfl': 0.5, 'tol': 1e-5, 'max_steps': 40000}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(HERE, '..', 'tests', 'golden', 'mmpde5_strided'))
    args = ap.parse_args()
    torch.set_num_threads(1)
    lin = torch.linspace(0, 1, N)
    z0 = torch.stack(torch.meshgrid(lin, lin, indexing='ij'))
    ms, m2 = monitor_arrays_2d(lambda a, b: monitor_2d(a, b, PARAMS), N)
    z32, j32, m32 = R.mmpde5(z0, ms, m2, **SOLVER)
    z64, j64, m64 = R.mmpde5(z0, ms, m2, dtype=torch.float64, **SOLVER)
    assert m32 <= SOLVER['tol'] and m64 <= SOLVER['tol'], (m32, m64)
    err32 = (z32.double() - z64).abs().max().item()
    path = os.path.join(args.out, '2d_n33_cfl0p5.npz')
    os.makedirs(args.out, exist_ok=True)
    np.savez(path, n=np.int32(N), z0=z0.numpy(), ms=ms.numpy(), m2=m2.numpy(), cfl=np.float64(SOLVER['cfl']),
             tol=np.float64(SOLVER['tol']), max_steps=np.int32(SOLVER['max_steps']), j32=np.int32(j32), j64=np.int32(j64),
             z64=z64.numpy(), err32=np.float64(err32), centers=np.asarray(PARAMS['centers']), scales=np.asarray(PARAMS['scales']))
    print(f"33 x 33, cfl {SOLVER['cfl']}, tol {SOLVER['tol']}: j32 = {j32}, j64 = {j64}, max |z32 - z64| = {err32:.3e} "
          f"-> {os.path.normpath(path)}")


if __name__ == '__main__':
    main()
