#!/usr/bin/env python
"""The Poisson error-reduction tables (`evaluate_model_fine`) of an untrained GNN next to the reference's network-free
baselines: the fixed mesh and backFEM, the gradient descent of the mesh nodes on the FEM error (`src/params.py:73-104`).

    python examples/evaluate_baselines.py                        # 2-D, 11 x 11: GNN, fixed_mesh_2D, backFEM_2D
    python examples/evaluate_baselines.py --dim 1 --mesh 21       # 1-D
    python examples/evaluate_baselines.py --time                 # ms per sample of the descent, one call against the Python loop
    python examples/evaluate_baselines.py --forward wave --adjoint wave   # the evaluation and backFEM_2D's descent on the
                                                                 # wave-parallel FEM kernels: the same tables (2-D)

`--time` measures `mesh_descent_2d` (1-D: `mesh_descent_1d`), every epoch enqueued by one call, against the loop it replaces,
written with the public functions (`modular_loss_2d`, 1-D `gradient_meshpoints_1D`, plus a torch update): at batch 1 and at
the dataset's size, both variants in this process, medians of repeated windows after a warm-up (docs/measurements.md).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g_adaptivity_amd import (MeshDataset, collate, evaluate_model_fine, get_model, hot_path_opt, mesh_descent_1d,   # noqa: E402
                              mesh_descent_2d)
from g_adaptivity_amd.descent import LAUNCHES_PER_EPOCH_1D, LAUNCHES_PER_EPOCH_2D   # noqa: E402
from g_adaptivity_amd.fem import modular_loss_2d   # noqa: E402
from g_adaptivity_amd.fem1d import gradient_meshpoints_1D   # noqa: E402
from g_adaptivity_amd.mesh_graph import MeshData   # noqa: E402


def summary(name, df, df_time) -> str:
    col = lambda t, k: np.asarray(t[k], dtype=float)
    return (f"{name:>14}  L1 red. {np.nanmean(col(df, 'L1_reduction_MLmodel')):9.2f} %   L2 red. "
            f"{np.nanmean(col(df, 'L2_reduction_MLmodel')):9.2f} %   (MMPDE5: {np.nanmean(col(df, 'L1_reduction_MA')):7.2f} % / "
            f"{np.nanmean(col(df, 'L2_reduction_MA')):7.2f} %)   {1e3 * np.nanmean(col(df_time, 'MLmodel_time')):9.3f} ms / sample")


def _windows(fn, dev, warmup, windows, reps):
    """Median and spread (min, max) in ms per call over `windows` windows of `reps` calls, after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(windows):
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize(dev)
        out.append(1e3 * (time.perf_counter() - t) / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def time_descent(dim, data, opt, batch, windows, reps):
    dev = data.x_comp.device
    epochs, lr = int(opt['epochs']), float(opt['lr'])
    x0, params = data.x_comp, data.pde_params
    if dim == 2:
        n = x0.shape[0] // batch
        tri = [data.cells.shape[0] // batch] * batch         # topology on the host for both variants: it is looked up, not rebuilt
        args = (data.cells.cpu(), data.boundary_nodes.cpu(), [n] * batch, params)
        interior = ~data.boundary_nodes
        routes = dict(forward=opt.get('fem_forward', 'lane'), adjoint=opt.get('fem_adjoint', 'lane'))
        one_call = lambda: mesh_descent_2d(x0, *args, epochs, lr, tri_counts=tri, **routes)

        def loop():
            x = x0.clone()
            for _ in range(epochs):
                _, gx = modular_loss_2d(x, *args, 9, 'simpson', tri_counts=tri, **routes)
                x[interior] = x[interior] - lr * gx[interior]
            return x
        per_epoch = LAUNCHES_PER_EPOCH_2D
    else:
        n = x0.shape[0] // batch
        one_call = lambda: mesh_descent_1d(x0, [n] * batch, params, opt, epochs, lr)
        o = dict(opt, grad_type='PDE_loss_direct_L2')
        d = MeshData(pde_params=params, _num_graphs=batch)
        inner = torch.ones(n, dtype=torch.bool, device=dev)
        inner[0] = inner[-1] = False
        inner = inner.repeat(batch)

        def loop():
            x = x0.clone()
            for _ in range(epochs):
                _, gx = gradient_meshpoints_1D(o, d, x)
                x[inner] = x[inner] - lr * gx[inner]
            return x
        per_epoch = LAUNCHES_PER_EPOCH_1D
    same = torch.equal(one_call().x, loop()) if dim == 2 else bool(((one_call().x - loop()).abs().max() <= 1e-6).item())
    for name, fn in (('one call', one_call), ('python loop', loop)):
        med, lo, hi = _windows(fn, dev, 2, windows, reps)
        print(f"  batch {batch:>3}  {name:>11}: {med / batch:9.3f} ms / sample  (median of {windows} windows of {reps}; "
              f"{lo / batch:.3f} .. {hi / batch:.3f}; {med / epochs * 1e3:.1f} us / epoch)")
    print(f"  batch {batch:>3}  same meshes: {same}; the one call issues {per_epoch} launches per epoch and none from Python")


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--dim', type=int, choices=(1, 2), default=2)
    ap.add_argument('--mesh', type=int, default=None, help='nodes per dimension (default 11 in 2-D, 21 in 1-D; 2-D: at most 26)')
    ap.add_argument('--num_test', type=int, default=25)
    ap.add_argument('--epochs', type=int, default=None, help="the descent's epochs (default: the reference's, 200 in 2-D, 10 in 1-D)")
    ap.add_argument('--batch_size', type=int, default=1, help='model batch of the evaluation')
    ap.add_argument('--time', action='store_true', help='time the descent instead of printing the tables')
    ap.add_argument('--forward', choices=('lane', 'wave'), default='lane',
                    help="2-D: the load vector and lattice evaluation of the error norms and of the descent's epochs (opt['fem_forward'])")
    ap.add_argument('--adjoint', choices=('lane', 'wave'), default='lane',
                    help="2-D: the two lattice walks of the backward in the descent's epochs (opt['fem_adjoint'])")
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    mesh = a.mesh or (11 if a.dim == 2 else 21)
    dims, suffix = [mesh] * a.dim, f'{a.dim}D'
    common = dict(mesh_dims=dims, device='cuda:0', solver='torch_FEM', evaler='analytical', eval_quad_points=101,
                  fem_forward=a.forward, fem_adjoint=a.adjoint)
    over = {} if a.epochs is None else {'epochs': a.epochs}
    test = MeshDataset(dims, a.num_test, seed=1, target='mmpde5')
    if a.time:
        opt = hot_path_opt(model='backFEM_' + suffix, **common, **over)
        routes = f", forward '{a.forward}', adjoint '{a.adjoint}'" if a.dim == 2 else ''
        print(f"backFEM_{suffix}, {mesh} nodes per dimension, {opt['epochs']} epochs, lr {opt['lr']}{routes}")
        for batch in (1, a.num_test):
            time_descent(a.dim, collate(test.samples[:batch]).to(opt['device']), opt, batch, a.windows, a.reps)
        sys.exit(0)
    for name in ('GNN', 'fixed_mesh_' + suffix, 'backFEM_' + suffix):
        extra = dict(hidden_dim=8, num_layers=4) if name == 'GNN' else {}
        if name.startswith('fixed_mesh'):
            extra['loss_type'] = 'mesh_loss'
        opt = hot_path_opt(model=name, **{**common, **extra, **(over if name.startswith('backFEM') else {})})
        torch.manual_seed(0)
        model = get_model(opt, test)
        model = model.to(opt['device']).eval()
        df, df_time = evaluate_model_fine(model, test, opt, batch_size=a.batch_size)
        print(summary(name + (' (untrained)' if name == 'GNN' else ''), df, df_time))
