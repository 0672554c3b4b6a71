#!/usr/bin/env python
"""The reference's 1-D Burgers experiment (`src/params.py:136-159`) end to end on the GPU: 21-node interval meshes,
conv_type='GRAND', hidden 8, loss_type='modular' with grad_type='burgers_timestep_loss_direct_mse' (tau 1/20, nu 0.001,
40-node fine mesh, one time step in training, 20 in evaluation).

Training (`src/run_GNN.py:115-120`): GNN forward, gradient_meshpoints_1D (the differentiable FEM tail), the pseudo-loss
sum(x_phys * x_grads) backward, Adam.  Prints the loss per epoch and ms per step, split into GNN and FEM tail.

Evaluation (`src/utils_eval_Burgers.py:262-300`): the 20-step rollout on the uniform and on the ML mesh, the model
re-invoked after every step with the evolved coefficients; the state moves to the new mesh by linear interpolation
(fn_expansion, the reference's commented-out alternative to its host spline).  Prints the final MSE of both meshes
against the fine solution.

    python examples/train_burgers.py --epochs 20
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g_adaptivity_amd import (GNN, MeshDataset, collate, fn_expansion, get_Burgers_initial_coeffs, gradient_meshpoints_1D,  # noqa: E402
                              hot_path_opt, torch_FEM_Burgers_1D)

FEM_OPT = {'gauss_amplitude': 0.25, 'tau': 1 / 20.0, 'nu': 0.001, 'load_quad_points': 101, 'eval_quad_points': 101,
           'stiff_quad_points': 3, 'num_fine_mesh_points': 40, 'num_time_steps': 1, 'num_eval_time_steps': 20,
           'mesh_dims': [21], 'grad_type': 'burgers_timestep_loss_direct_mse'}


def rollout(model, d, dev, ml: bool):
    """Final-time MSE of the mesh's solution against the fine solution after num_eval_time_steps steps."""
    o = FEM_OPT
    n, nf = o['mesh_dims'][0], o['num_fine_mesh_points']
    q = torch.linspace(0, 1, o['eval_quad_points'], device=dev)
    fine = torch.linspace(0, 1, nf, device=dev)
    with torch.no_grad():
        mesh = model(d).view(-1) if ml else torch.linspace(0, 1, n, device=dev)
        u, uf = get_Burgers_initial_coeffs(fine, nf, mesh, n, d.pde_params, o['load_quad_points'], o)
        for _ in range(o['num_eval_time_steps']):
            u, _, sol, _, _ = torch_FEM_Burgers_1D(o, mesh, q, n, u)
            uf, _, sol_f, _, _ = torch_FEM_Burgers_1D(o, fine, q, nf, uf)
            if ml:
                d.uu_tensor = u.clone()
                new = model(d).view(-1)
                u, mesh = fn_expansion(u, mesh, new, n), new
        return ((sol - sol_f) ** 2).mean().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=20)
    ap.add_argument('--num_train', type=int, default=20)
    ap.add_argument('--num_test', type=int, default=5)
    ap.add_argument('--batch_size', type=int, default=1)
    ap.add_argument('--lr', type=float, default=1e-3)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    ds = MeshDataset([21], a.num_train, seed=0, num_gauss=1, burgers=True)
    test = MeshDataset([21], a.num_test, seed=1, num_gauss=1, burgers=True)
    torch.manual_seed(0)
    model = GNN(ds, hot_path_opt(mesh_dims=[21], conv_type='GRAND', hidden_dim=8, gnn_inc_feat_f=False, device=str(dev))).to(dev)
    optim = torch.optim.Adam(model.parameters(), lr=a.lr)
    batches = [collate(ds.samples[i:i + a.batch_size]).to(dev) for i in range(0, len(ds), a.batch_size)]
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for epoch in range(a.epochs):
        model.train()
        tot, t = [], {'gnn': 0.0, 'fem': 0.0, 'step': 0.0}
        for dd in batches:
            e = [ev() for _ in range(4)]
            optim.zero_grad()
            e[0].record()
            x_phys = model(dd).view(-1)
            e[1].record()
            loss, x_grads = gradient_meshpoints_1D(FEM_OPT, dd, x_phys.detach())
            e[2].record()
            (x_phys * x_grads).sum().backward()
            optim.step()
            e[3].record()
            tot.append(loss)
            torch.cuda.synchronize()
            t['gnn'] += (e[0].elapsed_time(e[1]) + e[2].elapsed_time(e[3])) / len(batches)
            t['fem'] += e[1].elapsed_time(e[2]) / len(batches)
            t['step'] += e[0].elapsed_time(e[3]) / len(batches)
        print(f"epoch {epoch}: loss {torch.stack(tot).mean().item():.6e} | ms/step {t['step']:.3f} "
              f"(GNN fwd+bwd+Adam {t['gnn']:.3f}, FEM tail {t['fem']:.3f})", flush=True)
    model.eval()
    t0 = time.perf_counter()
    uni = [rollout(model, collate([s]).to(dev), dev, False) for s in test.samples]
    mlm = [rollout(model, collate([s]).to(dev), dev, True) for s in test.samples]
    print(f"evaluation ({FEM_OPT['num_eval_time_steps']} steps, {len(test.samples)} samples, {time.perf_counter() - t0:.2f} s): "
          f"MSE vs fine, uniform mesh {sum(uni) / len(uni):.4e}, ML mesh {sum(mlm) / len(mlm):.4e}", flush=True)


if __name__ == '__main__':
    main()
