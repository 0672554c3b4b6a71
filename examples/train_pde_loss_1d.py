#!/usr/bin/env python
"""Training with loss_type='pde_loss' in 1-D (`src/run_GNN.py:108-110`, `src/GNN.py:319-325`: torch_FEM_1D per mesh), the
reference's `GNN` config (`src/params.py:107-111`: hidden 8, 4 layers, dt 0.1, l1; `mesh_dims = [15]`).  The model is built with
opt['pde_loss_1d'].  Prints the loss per epoch and ms per step from HIP events around whole epochs, the median over the epochs
after the first with its min-max, and the evaluation tables (`evaluate_model_fine`) at the end.

`--step eager`: the host-driven loop (`GraphedTrainStep.eager`: the same iteration as plain launches).  `--step captured`: the
iteration captured once per batch shape and replayed, with the new batch's fields, target and Gaussians fed in.
`--tail split`: the Poisson solve, the loss launch and the adjoint solve (three launches); `--tail fused`:
gadapt_fem_poisson1d_loss, one launch, the same gradient bit for bit (opt['fem1d_tail']; captured steps only take it).

    python examples/train_pde_loss_1d.py --epochs 5 --num_train 64 --batch_size 8
    python examples/train_pde_loss_1d.py --step captured --tail fused --mesh 15 --batch_size 1
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g_adaptivity_amd import GNN, GraphedTrainStep, MeshDataset, collate, hot_path_opt, l1_loss   # noqa: E402
from g_adaptivity_amd.evaluation import evaluate_model_fine   # noqa: E402
from g_adaptivity_amd.optim import FlatAdam   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=5)
    ap.add_argument('--num_train', type=int, default=64)
    ap.add_argument('--batch_size', type=int, default=8)
    ap.add_argument('--mesh', type=int, default=15, help="nodes per mesh (the reference's mesh_dims = [15])")
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--step', choices=['eager', 'captured'], default='eager',
                    help="'eager': the iteration as plain launches; 'captured': one replayed hipGraph per step")
    ap.add_argument('--tail', choices=['split', 'fused'], default='split',
                    help="opt['fem1d_tail']: the FEM tail of a captured step as three launches or as one (the same gradient bits)")
    ap.add_argument('--no_eval', action='store_true', help="skip the evaluation tables")
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    n = a.mesh
    opt = hot_path_opt(mesh_dims=[n], hidden_dim=8, num_layers=4, time_step=0.1, loss_type='pde_loss', loss_fn='l1', pde_loss_1d=True,
                       fem1d_tail=a.tail, device=str(dev))
    ds = MeshDataset([n], a.num_train, seed=n, pde_loss_fields=True)
    torch.manual_seed(0)
    model = GNN(ds, opt).to(dev).train()
    batches = [collate(ds.samples[i:i + a.batch_size]).to(dev) for i in range(0, len(ds), a.batch_size)]
    step = GraphedTrainStep(model, FlatAdam(model.parameters(), lr=a.lr, capturable=True), loss_fn=l1_loss)
    run = step if a.step == 'captured' else step.eager
    run(batches[0])                                          # captured: the capture (its warm-up is undone) and one step
    how = f"{a.step}, tail {a.tail if a.step == 'captured' else 'split'}"
    per_step = []
    for epoch in range(a.epochs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        tot = torch.zeros((), device=dev)
        t0.record()
        for dd in batches:
            tot += run(dd)                                   # (the captured step's static loss tensor: accumulated on the device)
        t1.record()
        t1.synchronize()
        per_step.append(t0.elapsed_time(t1) / len(batches))
        print(f"mesh {n} epoch {epoch}: loss {tot.item() / len(batches):.5f} | ms/step {per_step[-1]:.4f} ({how})", flush=True)
    timed = per_step[1:] or per_step
    print(f"mesh {n} batch {a.batch_size} ({how}): ms/step median {statistics.median(timed):.4f} "
          f"(min {min(timed):.4f}, max {max(timed):.4f}) over {len(timed)} epochs of {len(batches)} steps", flush=True)
    if not a.no_eval:
        df, df_time = evaluate_model_fine(model, ds, dict(opt), batch_size=a.batch_size)
        print(df if hasattr(df, 'to_string') else {k: [round(float(v), 6) for v in vals] for k, vals in df.items()})
        print(df_time if hasattr(df_time, 'to_string') else {k: [round(float(v), 6) for v in vals] for k, vals in df_time.items()})


if __name__ == '__main__':
    main()
