#!/usr/bin/env python
"""Training with loss_type='pde_loss' (`src/run_GNN.py:108-110`): the mesh is trained on the error of a differentiable P1
FEM solve on the moved mesh, the reference's own `GNN` config (`src/params.py:107-111`: hidden 8, 4 layers, dt 0.1, l1,
training meshes 15 and 20).  Prints the loss per epoch and ms per step, split into GNN forward / backward and FEM tail
forward / backward.

`--step captured` trains with `GraphedTrainStep` instead: the iteration is captured once per batch topology and replayed, with
the new batch's fields, target and Gaussians fed in and no host synchronisation inside an epoch; it prints the loss per epoch
and ms per step from HIP events around whole epochs.  `--adjoint wave` runs the backward's two lattice walks with a wave per
node and per triangle (opt['fem_adjoint']); the gradients are the same, bit for bit.  `--forward wave` runs the forward's load
vector with a wave per node and its evaluation with a wave per chunk of the lattice (opt['fem_forward'], `--band lds` only);
coeffs and sol are the same, bit for bit.

    python examples/train_pde_loss.py --epochs 3 --num_train 32 --batch_size 8
    python examples/train_pde_loss.py --step captured --adjoint wave --mesh 11 --batch_size 1
    python examples/train_pde_loss.py --step captured --adjoint wave --forward wave --mesh 11 --batch_size 1
    python examples/train_pde_loss.py --mesh 64 --band window --num_train 4 --batch_size 2   # beyond 26 x 26: the windowed route
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g_adaptivity_amd import GNN, GraphedTrainStep, MeshDataset, collate, fem_poisson, hot_path_opt, l1_loss   # noqa: E402
from g_adaptivity_amd.optim import FlatAdam   # noqa: E402


def train_captured(model, batches, a, n):
    """The same training as one replayed hipGraph per step: nothing waits for the device inside an epoch."""
    step = GraphedTrainStep(model, FlatAdam(model.parameters(), lr=a.lr, capturable=True), loss_fn=l1_loss)
    step(batches[0])                                         # the capture (its warm-up iterations are undone) and one step
    for epoch in range(a.epochs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        tot = torch.zeros((), device=batches[0].x_comp.device)
        t0.record()
        for dd in batches:
            tot += step(dd)                                  # the static loss tensor: accumulated on the device
        t1.record()
        t1.synchronize()
        print(f"mesh {n}x{n} epoch {epoch}: loss {tot.item() / len(batches):.5f} | ms/step {t0.elapsed_time(t1) / len(batches):.3f} "
              f"(captured, adjoint {a.adjoint}, forward {a.forward})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--num_train', type=int, default=32)
    ap.add_argument('--batch_size', type=int, default=8)
    ap.add_argument('--mesh_dims_train', type=int, nargs='+', default=[15, 20])
    ap.add_argument('--mesh', type=int, default=None, help="one training mesh size instead of --mesh_dims_train")
    ap.add_argument('--band', choices=['lds', 'window'], default='lds',
                    help="FEM route (opt['fem_band']): 'lds' keeps the banded factor in LDS (meshes up to 26 x 26), 'window' streams "
                         "it through a workspace (up to 81 x 81)")
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--step', choices=['eager', 'captured'], default='eager',
                    help="'eager': the host-driven loop with its per-phase split; 'captured': GraphedTrainStep with FlatAdam(capturable=True)")
    ap.add_argument('--adjoint', choices=['lane', 'wave'], default='lane',
                    help="the backward's lattice walks (opt['fem_adjoint']): a lane or a wave per node and per triangle, the same bits")
    ap.add_argument('--forward', choices=['lane', 'wave'], default='lane',
                    help="the forward's load vector and evaluation (opt['fem_forward']): a lane per node and five lattice points per "
                         "lane, or a wave per node and per chunk of the lattice (--band lds only), the same bits")
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    for n in ([a.mesh] if a.mesh else a.mesh_dims_train):
        opt = hot_path_opt(mesh_dims=[n, n], hidden_dim=8, num_layers=4, time_step=0.1, loss_type='pde_loss', loss_fn='l1',
                           device=str(dev), fem_band=a.band, fem_adjoint=a.adjoint, fem_forward=a.forward)
        ds = MeshDataset([n, n], a.num_train, seed=n, pde_loss_fields=True)
        torch.manual_seed(0)
        model = GNN(ds, opt).to(dev).train()
        batches = [collate(ds.samples[i:i + a.batch_size]).to(dev) for i in range(0, len(ds), a.batch_size)]
        if a.step == 'captured':
            train_captured(model, batches, a, n)
            continue
        optim = torch.optim.Adam(model.parameters(), lr=a.lr)
        ev = lambda: torch.cuda.Event(enable_timing=True)
        for epoch in range(a.epochs):
            tot, t = 0.0, {'gnn_fwd': 0.0, 'fem_fwd': 0.0, 'fem_bwd': 0.0, 'gnn_bwd': 0.0, 'step': 0.0}
            for dd in batches:
                e = [ev() for _ in range(6)]
                optim.zero_grad()
                e[0].record()
                # the model's pde_loss forward split in its two halves: x_phys, then the FEM tail (GNN.forward does both)
                model.opt['loss_type'] = 'mesh_loss'
                x_phys = model(dd)
                model.opt['loss_type'] = 'pde_loss'
                e[1].record()
                xd = x_phys.detach().requires_grad_(True)
                counts = torch.bincount(dd.batch.cpu()).tolist()
                coeffs, sol = fem_poisson(xd, dd.cells, dd.boundary_nodes, counts, dd.pde_params, model.quad_points, band=a.band,
                                          adjoint=a.adjoint, forward=a.forward)
                loss = l1_loss(sol.view(-1, 1), dd.u_true_fine_tensor.view(-1, 1))
                e[2].record()
                loss.backward()
                e[3].record()
                x_phys.backward(xd.grad)
                e[4].record()
                optim.step()
                e[5].record()
                torch.cuda.synchronize()
                for k, (i, j) in zip(t, [(0, 1), (1, 2), (2, 3), (3, 4), (0, 5)]):
                    t[k] += e[i].elapsed_time(e[j]) / len(batches)
                tot += loss.item() / len(batches)
            print(f"mesh {n}x{n} epoch {epoch}: loss {tot:.5f} | ms/step {t['step']:.2f} (GNN fwd {t['gnn_fwd']:.2f}, "
                  f"FEM fwd {t['fem_fwd']:.2f}, FEM bwd {t['fem_bwd']:.2f}, GNN bwd {t['gnn_bwd']:.2f})", flush=True)


if __name__ == '__main__':
    main()
