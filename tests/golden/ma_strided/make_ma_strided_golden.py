#!/usr/bin/env python
"""Writes ds64.npz: the yardstick of the converged 64 x 64 Monge-Ampere comparison in tests/test_gpu_ma_strided.py, about a
minute of CPU and so too long to repeat in every run of the suite.  The case is `ma_strided_cases.case('ds64')`: the Gaussians
of `MeshDataset([64, 64], 1, seed=0).samples[0]`, mon_reg = 0.01, mon_power = 0.2, cfl = 0.2, tol = 1e-4.

  phi64   the fp64 restatement's potential at its stopping step (x, y follow from one `ma_restatement.evaluate`)
  steps   the stopping steps of the fp64, the mixed and the perturbed mixed restatement
  noise   max(|z_mixed - z64|, |z_mixed' - z_mixed|) after exactly steps[0] updates
  gauss   the case's Gaussians [G, 4] in fp32: the test checks that it rebuilt the same inputs

No GPU.
    python tests/golden/ma_strided/make_ma_strided_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [TESTS, os.path.dirname(TESTS)]
import ma_restatement as R  # noqa: E402
import ma_strided_cases as SK  # noqa: E402
import ma_strided_restatement as S  # noqa: E402

if __name__ == '__main__':
    c = SK.case('ds64')
    inp = R.inputs(c.params, torch.float64)
    gx, gy = R.grid(c.N, torch.float64)
    w1 = torch.ones(c.N, dtype=torch.float64)
    w1[0] = w1[-1] = 0.5
    w = w1[:, None] * w1[None, :]
    dt = torch.tensor(SK.CFL / float((c.N - 1) ** 2), dtype=torch.float64)
    # ma_restatement.ma's fp64 loop again, keeping phi (it returns only x and y)
    phi, steps = torch.zeros(c.N, c.N, dtype=torch.float64), 0
    while True:
        x, y, r, lam = R.evaluate(phi, c.N, gx, gy, *inp)
        rbar = (w * r).sum() / float((c.N - 1) ** 2)
        res = torch.maximum(r.max() - rbar, rbar - r.min())
        assert lam.min().item() > 0 and steps < 40000
        if bool(res <= torch.tensor(SK.TOL, dtype=torch.float32).double()):
            break
        phi = phi + (dt * torch.clamp(lam.min(), max=1.0)) * (r - rbar)
        steps += 1
    z64 = torch.stack([x, y])
    print('fp64', steps, res.item(), flush=True)
    m = S.ma(c.N, c.params, cfl=SK.CFL, tol=SK.TOL, max_steps=40000, also_at=steps)
    print('mixed', m[1], m[2], flush=True)
    mp = S.ma(c.N, c.params, cfl=SK.CFL, tol=SK.TOL, max_steps=40000, perturb=SK.PERTURB_SEED, also_at=steps)
    print("mixed'", mp[1], mp[2], flush=True)
    noise = SK.noise_of(z64, m[-1], mp[-1])
    print('noise', noise, 'min lambda', m[4], 'spread', R.uniform_spread(c.N, c.params), '->', R.cell_spread(z64, c.params))
    np.savez(os.path.join(HERE, 'ds64.npz'), phi64=phi.numpy(), steps=np.asarray([steps, m[1], mp[1]], np.int64),
             noise=np.float64(noise), gauss=inp[0].float().numpy())
