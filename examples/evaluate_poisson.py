#!/usr/bin/env python
"""The reference's headline tables (`src/utils_eval.py:106-267`, evaluate_model_fine) on the MI355X, without Firedrake: per test
sample the FEM error on the uniform grid, on the classical MMPDE5 target mesh and on the model's mesh, and the percentage
error reduction of the last two, with the model's time per sample.

    python examples/evaluate_poisson.py                         # 2-D, 11 x 11, trains briefly first
    python examples/evaluate_poisson.py --dim 1 --mesh 21
    python examples/evaluate_poisson.py --state model.pt         # a saved state_dict instead of the brief training
    python examples/evaluate_poisson.py --mesh 64 --band window  # beyond 26 x 26: the windowed band solve
    python examples/evaluate_poisson.py --forward wave           # the wave-parallel load vector and evaluation: the same tables
    python examples/evaluate_poisson.py --mesh 64 --band window --mmpde5_route strided --mmpde5_cfl 0.5 --mmpde5_max_steps 40000
                                                                 # ... with real MMPDE5 targets beyond 32 x 32
    python examples/evaluate_poisson.py --target monge_ampere    # the MA columns on Monge-Ampere meshes (2-D, at most 32 x 32)
    python examples/evaluate_poisson.py --mesh 64 --band window --target monge_ampere --ma_route strided --ma_max_steps 40000
    python examples/evaluate_poisson.py --target monge_ampere --ma_monitor M2N --ma_mon_reg 0.1 --m2n_beta 1.5   # the M2N 'fast' monitor
    python examples/evaluate_poisson.py --target monge_ampere --ma_monitor M2N --m2n_monitor slow --m2n_alpha 1.0   # the 'slow' one
                                                                 # ... beyond 32 x 32: the fp64-potential route, up to 81 x 81
    python examples/evaluate_poisson.py --mesh 11 --target monge_ampere --uu fem --ma_monitor_source uu
                                                                 # the MA columns of a mover that knows only the coarse P1 solution
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g_adaptivity_amd import GNN, MeshDataset, MeshLoader, eval_grid_MMPDE_MA, evaluate_model_fine, hot_path_opt   # noqa: E402


def describe(table) -> str:
    """`DataFrame.describe()`, or the same summary rows from a dict of numpy arrays where pandas is not installed."""
    if hasattr(table, 'describe'):
        return str(table.describe())
    names = list(table)
    stats = [('count', lambda v: float(np.isfinite(v).sum())), ('mean', np.nanmean), ('std', lambda v: np.nanstd(v, ddof=1)),
             ('min', np.nanmin), ('50%', np.nanmedian), ('max', np.nanmax)]
    lines = [' ' * 6 + ''.join(f"{n:>22}" for n in names)]
    for label, fn in stats:
        lines.append(f"{label:<6}" + ''.join(f"{fn(np.asarray(table[n], dtype=float)):>22.6e}" for n in names))
    return '\n'.join(lines)


def train_briefly(model, dataset, opt, epochs):
    model.train()
    optim = torch.optim.Adam(model.parameters(), lr=opt['lr'])
    for _ in range(epochs):
        for data in MeshLoader(dataset, batch_size=opt['batch_size'], shuffle=False):
            data = data.to(opt['device'])
            optim.zero_grad()
            F.mse_loss(model(data).view_as(data.x_phys), data.x_phys).backward()
            optim.step()
    return model.eval()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--dim', type=int, choices=(1, 2), default=2)
    ap.add_argument('--mesh', type=int, default=11, help="nodes per dimension (2-D: at most 26, with --band window 81)")
    ap.add_argument('--band', choices=('lds', 'window'), default='lds',
                    help="FEM route of the 2-D evaluation: 'lds' keeps the banded factor in LDS, 'window' streams it (opt['fem_band'])")
    ap.add_argument('--forward', choices=('lane', 'wave'), default='lane',
                    help="the load vector and lattice evaluation of the 2-D error norms (opt['fem_forward']): a lane per node and five "
                         "lattice points per lane, or a wave per node and per chunk of the lattice (--band lds only); the same norms, "
                         "bit for bit")
    ap.add_argument('--mmpde5_route', choices=('lane', 'strided'), default='lane',
                    help="MMPDE5 targets: 'lane' stops at 32 a side in 2-D (beyond it the noise stand-in is used), 'strided' at 81")
    ap.add_argument('--mmpde5_cfl', type=float, default=None, help='RK4 step of MMPDE5 is cfl / N^3 (default: the reference 0.05)')
    ap.add_argument('--mmpde5_max_steps', type=int, default=None, help='step cap of MMPDE5 (default: the reference 10000)')
    ap.add_argument('--target', choices=('mmpde5', 'monge_ampere'), default='mmpde5',
                    help="the classical target behind the MA columns: MMPDE5 (default), or the finite-difference Monge-Ampere solve "
                         "that stands for the reference's default 2-D target (2-D, --mesh <= 32, or <= 81 with --ma_route strided)")
    ap.add_argument('--ma_route', choices=('lane', 'strided'), default='lane',
                    help="Monge-Ampere targets: 'lane' (fp32 potential) stops at 32 a side, 'strided' (fp64 potential) at 81")
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
                         "(sides above 26 take --band window)")
    ap.add_argument('--num_train', type=int, default=32)
    ap.add_argument('--num_test', type=int, default=16)
    ap.add_argument('--epochs', type=int, default=20)
    ap.add_argument('--batch_size', type=int, default=1, help='model batch of the evaluation (1: the latency the reference times)')
    ap.add_argument('--state', default=None, help='state_dict to load instead of training')
    a = ap.parse_args()
    dims = [a.mesh] * a.dim
    opt = hot_path_opt(mesh_dims=dims, hidden_dim=8, num_layers=4, batch_size=8, device='cuda:0', lr=1e-2, loss_type='mesh_loss',
                       solver='torch_FEM', evaler='analytical', eval_quad_points=101, load_quad_points=101,
                       fem_band=a.band, fem_forward=a.forward, mmpde5_route=a.mmpde5_route, ma_route=a.ma_route)
    # the default route of the batched MMPDE5 generator stops at 32 nodes a side in 2-D: beyond it the "MA" columns are those of
    # the stand-in target unless --mmpde5_route strided is given (81 a side)
    target = 'mmpde5' if a.dim == 1 or a.mesh <= (81 if opt['mmpde5_route'] == 'strided' else 32) else 'noise'
    solver = {'route': opt['mmpde5_route']}
    solver.update({k: v for k, v in (('cfl', a.mmpde5_cfl), ('max_steps', a.mmpde5_max_steps)) if v is not None})
    target_params = {'solver': solver} if target == 'mmpde5' else None
    if a.target == 'monge_ampere':                 # the reference's own 2-D configuration: 2-D, its own monitor defaults
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
        if a.ma_monitor_source != 'analytic':      # absent, the datasets take today's path
            monitor['monitor_source'] = a.ma_monitor_source
        target, target_params = 'monge_ampere', dict(monitor, solver=solver)
    uu = {} if a.uu == 'exact' else {'uu': a.uu, 'uu_params': {'fem_band': a.band}}
    test = MeshDataset(dims, a.num_test, seed=1, target=target, target_params=target_params, **uu)
    torch.manual_seed(0)
    model = GNN(test, opt).to(opt['device'])
    if a.state:
        model.load_state_dict(torch.load(a.state, map_location=opt['device']))
    else:
        train_briefly(model, MeshDataset(dims, a.num_train, seed=0, target=target, target_params=target_params, **uu), opt, a.epochs)
    eval_grid_MMPDE_MA(test, opt)                  # grid and target errors once; further checkpoints reuse them
    df, df_time = evaluate_model_fine(model, test, opt, batch_size=a.batch_size)
    print(describe(df))
    print(describe(df_time))
