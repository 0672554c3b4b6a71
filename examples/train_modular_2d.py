#!/usr/bin/env python
"""Training with loss_type='modular' in 2-D (`src/run_GNN.py:113-118`): the model moves the mesh, gradient_meshpoints_2D
returns the FEM loss of each moved mesh and its gradient wrt the node coordinates, and the model is trained on the
pseudo-loss sum(x_phys * x_grads) with Adam.  GRAND_plus, hidden 8, 11 x 11 meshes, grad_type PDE_loss_direct_mse and
batch 1 by default (the reference's defaults).  Prints the loss per epoch.

    python examples/train_modular_2d.py --epochs 5 --num_train 8 --batch_size 1
    python examples/train_modular_2d.py --forward wave                                   # the wave-parallel FEM forward (--band lds)
    python examples/train_modular_2d.py --mesh_dim 64 --band window --num_train 2       # beyond 26 x 26: the windowed route
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g_adaptivity_amd import GNN, MeshDataset, collate, gradient_meshpoints_2D, hot_path_opt   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=5)
    ap.add_argument('--num_train', type=int, default=8)
    ap.add_argument('--batch_size', type=int, default=1)
    ap.add_argument('--mesh_dim', type=int, default=11)
    ap.add_argument('--grad_type', default='PDE_loss_direct_mse',
                    choices=['PDE_loss_direct_mse', 'PDE_loss_direct_L2', 'PDE_loss_adjoint_L2'])
    ap.add_argument('--band', choices=['lds', 'window'], default='lds',
                    help="FEM route (opt['fem_band']): 'lds' keeps the banded factor in LDS (meshes up to 26 x 26), 'window' streams "
                         "it through a workspace (up to 81 x 81)")
    ap.add_argument('--forward', choices=['lane', 'wave'], default='lane',
                    help="the forward's load vector and evaluation (opt['fem_forward']): 'wave' is the wave-parallel form on "
                         "--band lds, the same bits")
    ap.add_argument('--lr', type=float, default=1e-3)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    n = a.mesh_dim
    opt = hot_path_opt(mesh_dims=[n, n], conv_type='GRAND_plus', hidden_dim=8, num_layers=4, time_step=0.1,
                       loss_type='modular', grad_type=a.grad_type, eval_quad_points=101, load_quad_points=101, device=str(dev),
                       fem_band=a.band, fem_forward=a.forward)
    ds = MeshDataset([n, n], a.num_train, seed=n)
    torch.manual_seed(0)
    model = GNN(ds, opt).to(dev).train()
    optim = torch.optim.Adam(model.parameters(), lr=a.lr)
    batches = [collate(ds.samples[i:i + a.batch_size]).to(dev) for i in range(0, len(ds), a.batch_size)]
    for epoch in range(a.epochs):
        tot = torch.zeros((), device=dev)
        for data in batches:
            optim.zero_grad()
            x_phys = model(data)
            loss, x_grads = gradient_meshpoints_2D(opt, data, x_phys.detach())   # run_GNN.py:115-118
            (x_phys * x_grads).sum().backward()
            optim.step()
            tot += loss / len(batches)
        print(f"mesh {n}x{n} {a.grad_type} epoch {epoch}: loss {tot.item():.6e}", flush=True)


if __name__ == '__main__':
    main()
