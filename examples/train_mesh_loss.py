#!/usr/bin/env python
"""The reference's training loop (`src/run_GNN.py:66-154`, loss_type='mesh_loss') on the MI355X-native model.

Same shape as the reference: DataLoader -> for epoch / for batch: zero_grad, model(data), loss_fn(out, data.x_phys),
backward, optimizer.step; best-state tracking.  Differences: synthetic Firedrake-free dataset (mesh_graph.MeshDataset),
`GNN` from g_adaptivity_amd, and the flat-bucket Adam (drop-in for torch.optim.Adam).

    python examples/train_mesh_loss.py --mesh 32 --num_train 64 --batch_size 16 --epochs 3
"""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g_adaptivity_amd import GNN, DeviceMeshLoader, GraphedTrainStep, MeshDataset, MeshLoader, hot_path_opt, l1_loss, mse_loss, unit_gradient   # noqa: E402
from g_adaptivity_amd.optim import FlatAdam                                      # noqa: E402


def main(opt, dataset, log=print):
    """Returns (model, per-epoch losses, steady-state meshes/s of the last epoch).

    opt['graphed'] (default True): the iteration is a `GraphedTrainStep` - captured once per batch size, replayed on every new
    batch, the loader gathering straight into the captured step's input buffers.  False: the same iteration as eager launches,
    line by line the reference's loop."""
    shuffle = not opt.get('overfit_num')
    graphed = opt.get('graphed', True) and opt.get('device_loader', True) and opt.get('native_loss', True)
    torch.manual_seed(opt.get("seed", 0))             # reproducible initial weights (the reference draws a random seed: run_pipeline.py:52-54)
    model = GNN(dataset, opt).to(opt["device"])
    if opt.get('native_loss', True):       # loss and d loss/d out in one launch
        loss_fn = mse_loss if opt['loss_fn'] == 'mse' else l1_loss
    else:
        loss_fn = F.mse_loss if opt['loss_fn'] == 'mse' else F.l1_loss
    optimizer = FlatAdam(model.parameters(), lr=opt['lr'], weight_decay=opt['decay'], capturable=graphed)
    model.train()
    # (GADAPT_FUSED=0: the captured autograd iteration instead of the fused 13-launch one - A/B runs)
    step = GraphedTrainStep(model, optimizer, loss_fn=loss_fn, fused=os.environ.get('GADAPT_FUSED', '1') != '0') if graphed else None
    if opt.get('device_loader', True):     # samples stacked on the GPU, batches assembled there (no per-step host collation)
        loader = DeviceMeshLoader(dataset, batch_size=opt['batch_size'], shuffle=shuffle, device=opt['device'],
                                  fields=('x_comp', 'x_phys', 'f_tensor', 'uu_tensor'),
                                  into=step.static_batch if graphed else None)
    else:                                  # the reference's shape: CPU collation + .to(device) per step
        loader = MeshLoader(dataset, batch_size=opt['batch_size'], shuffle=shuffle)
    loss_list, best_loss, best_dict, rate = [], float('inf'), None, None
    for epoch in range(opt['epochs']):
        epoch_loss = torch.zeros((), device=opt['device'])
        model.epoch = epoch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, data in enumerate(loader):
            data.idx = i
            if graphed:
                loss = step(data)                            # zero_grad + forward + loss + backward + Adam: one graph replay
            else:
                optimizer.zero_grad()
                data = data.to(opt['device'])
                out = model(data)
                loss = loss_fn(out, data.x_phys)
                if opt.get('native_loss', True):
                    loss.backward(gradient=unit_gradient(loss.device))   # = loss.backward(), root gradient not re-created per step
                else:
                    loss.backward()
                optimizer.step()
            epoch_loss += loss.detach()                      # no .item() per batch: one sync per epoch
        loss_list.append(float(epoch_loss))                  # (synchronises)
        rate = len(dataset) / (time.perf_counter() - t0)
        log(f"epoch {epoch} loss {loss_list[-1]:.6e}  {rate:,.0f} meshes/s")
        if loss_list[-1] < best_loss:
            best_loss = loss_list[-1]
            best_dict = {k: v.clone() for k, v in model.state_dict().items()}   # a real copy (the reference's is shallow)
    model.load_state_dict(best_dict)
    return model, loss_list, rate


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--mesh', type=int, default=32)
    ap.add_argument('--num_train', type=int, default=64)
    ap.add_argument('--batch_size', type=int, default=16)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--hidden_dim', type=int, default=64)
    ap.add_argument('--num_layers', type=int, default=4)
    ap.add_argument('--cpu_loader', action='store_true', help='collate on the host every step, as the reference does')
    ap.add_argument('--torch_loss', action='store_true')
    ap.add_argument('--eager', action='store_true', help='eager launches instead of the captured training step')
    ap.add_argument('--target', choices=('noise', 'mmpde5', 'monge_ampere'), default='noise',
                    help="x_phys of the samples: the noise stand-in, the reference's MMPDE5 meshes (one batched GPU call; --mesh <= 32, "
                         "or <= 81 with --mmpde5_route strided), or Monge-Ampere meshes, the reference's default 2-D target "
                         "(finite differences, one batched GPU call; --mesh <= 32, or <= 81 with --ma_route strided)")
    ap.add_argument('--mmpde5_route', choices=('lane', 'strided'), default='lane', help="route of the MMPDE5 generator (--target mmpde5)")
    ap.add_argument('--mmpde5_cfl', type=float, default=None, help='RK4 step of MMPDE5 is cfl / N^3 (default: the reference 0.05)')
    ap.add_argument('--mmpde5_max_steps', type=int, default=None, help='step cap of MMPDE5 (default: the reference 10000)')
    ap.add_argument('--ma_route', choices=('lane', 'strided'), default='lane',
                    help="route of the Monge-Ampere generator (--target monge_ampere): 'lane' to 32 a side, 'strided' (fp64 potential) to 81")
    ap.add_argument('--ma_cfl', type=float, default=None, help='pseudo-time step of Monge-Ampere is cfl h^2 (default 0.2)')
    ap.add_argument('--ma_max_steps', type=int, default=None,
                    help='update cap of Monge-Ampere (default 20000; 64 x 64 wanted up to 25 500, 81 x 81 up to 32 000)')
    ap.add_argument('--ma_monitor', choices=('ma', 'M2N'), default='ma',
                    help="monitor of the Monge-Ampere targets: the reference's mesh_type 'ma', or 'M2N' with fast_M2N_monitor = 'fast' "
                         "(mon_reg + beta F / max F over the moving nodes) or, with --m2n_monitor slow, 'slow'")
    ap.add_argument('--m2n_monitor', choices=('fast', 'slow'), default='fast',
                    help="fast_M2N_monitor of --ma_monitor M2N.  'slow' adds alpha (u_h - u)^2 / max from a P1 Poisson solve on the moving "
                         "mesh inside every update (m2n_solve='p1': lane route, up to 24 a side); 'superslow' is not built")
    ap.add_argument('--m2n_alpha', type=float, default=1.0, help="alpha of the M2N 'slow' monitor (the reference's default 1.0)")
    ap.add_argument('--ma_mon_reg', type=float, default=None,
                    help="mon_reg of the Monge-Ampere monitor: 'ma' then uses (mon_reg + |H|)^0.2 in place of (1 + |H|)^0.2; "
                         "'M2N' needs it (default 0.1, the reference's run parameters)")
    ap.add_argument('--m2n_beta', type=float, default=1.5, help="beta of the M2N monitor (the reference's default 1.5)")
    ap.add_argument('--ma_monitor_source', choices=('analytic', 'uu'), default='analytic',
                    help="what drives the Monge-Ampere monitor: the Gaussians' analytic Hessian (default), or second differences of "
                         "each sample's own uu_tensor, read from a table (monitor_from_nodal, ma_table_batch; --ma_monitor ma only)")
    ap.add_argument('--uu', choices=('exact', 'fem'), default='exact',
                    help="uu_tensor of the samples: u_true at the nodes (default), or the coarse P1 Poisson solve the reference stores "
                         "(windowed band solve above 26 a side)")
    ap.add_argument('--glob_feat', action='store_true',
                    help="per-mesh CNN features of f and uu on every node (gnn_inc_glob_feat_f / _uu, the reference's argparse default)")
    ap.add_argument('--glob_feat_kernel', choices=('torch', 'hip', 'auto'), default='torch',
                    help="what computes them: the Conv modules, the one-launch HIP kernels (2-D images up to 23 x 23 at hidden 8, 16 x 16 at 16, "
                         "11 x 11 at 32, 7 x 7 at 64; an error beyond), or HIP where it fits")
    a = ap.parse_args()
    opt = hot_path_opt(mesh_dims=[a.mesh, a.mesh], hidden_dim=a.hidden_dim, num_layers=a.num_layers, batch_size=a.batch_size,
                       gnn_inc_glob_feat_f=a.glob_feat, gnn_inc_glob_feat_uu=a.glob_feat, glob_feat_kernel=a.glob_feat_kernel,
                       epochs=a.epochs, device='cuda:0', loss_fn='mse', lr=1e-3, show_mesh_evol_plots='False',
                       device_loader=not a.cpu_loader, native_loss=not a.torch_loss, graphed=not a.eager,
                       mmpde5_route=a.mmpde5_route, ma_route=a.ma_route)
    if a.target == 'monge_ampere':
        solver = {'route': opt['ma_route']}
        solver.update({k: v for k, v in (('cfl', a.ma_cfl), ('max_steps', a.ma_max_steps)) if v is not None})
        if a.ma_monitor == 'M2N':                  # the monitor travels in target_params, next to the solver's keywords
            monitor = {'mesh_type': 'M2N', 'fast_M2N_monitor': a.m2n_monitor, 'mon_reg': 0.1 if a.ma_mon_reg is None else a.ma_mon_reg,
                       'M2N_beta': a.m2n_beta}
            if a.m2n_monitor == 'slow':            # opt-in: the P1 solve inside the kernel
                monitor['M2N_alpha'] = a.m2n_alpha
                solver['m2n_solve'] = 'p1'
        else:
            monitor = {} if a.ma_mon_reg is None else {'mon_reg': a.ma_mon_reg, 'mon_power': 0.2}
        if a.ma_monitor_source != 'analytic':      # absent, the dataset takes today's path
            monitor['monitor_source'] = a.ma_monitor_source
    else:
        monitor = {}
        solver = {'route': opt['mmpde5_route']}
        solver.update({k: v for k, v in (('cfl', a.mmpde5_cfl), ('max_steps', a.mmpde5_max_steps)) if v is not None})
    ds = MeshDataset(opt['mesh_dims'], a.num_train, seed=0, target=a.target,
                     target_params=dict(monitor, solver=solver) if a.target != 'noise' else None,
                     **({} if a.uu == 'exact' else {'uu': a.uu, 'uu_params': {'fem_band': 'window' if a.mesh > 26 else 'lds'}}))
    t0 = time.time()
    model, losses, rate = main(opt, ds)
    torch.cuda.synchronize()
    print(f"{a.epochs} epochs x {a.num_train} meshes in {time.time() - t0:.2f} s; last epoch {rate:,.0f} meshes/s "
          f"({'graphed step' if opt['graphed'] and not a.cpu_loader and not a.torch_loss else 'eager launches'}); losses {losses}")
