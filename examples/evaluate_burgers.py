#!/usr/bin/env python
"""The reference's Burgers evaluation (`src/utils_eval_Burgers.py`) on the GPU for the 1-D Burgers config of `src/params.py:136-159`
(21-node meshes, 40-node fine mesh, 101 lattice points, tau 1/20, nu 0.001): the one-step table and the rollout table of a
seeded, untrained (or `--checkpoint`) model, then the same tables for a second model to show what the stored grid / fine /
classical rollouts save.

    python examples/evaluate_burgers.py --num_test 8 --batch_size 8
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g_adaptivity_amd import (GNN, MeshDataset, evaluate_model_fine_burgers, evaluate_model_fine_burgers_time_step,  # noqa: E402
                              hot_path_opt)

OPT = {'gauss_amplitude': 0.25, 'tau': 1 / 20.0, 'nu': 0.001, 'load_quad_points': 101, 'eval_quad_points': 101, 'stiff_quad_points': 3,
       'num_fine_mesh_points': 40, 'num_time_steps': 1, 'num_eval_time_steps': 20, 'mesh_dims': [21], 'mon_reg': 0.1, 'mon_power': 0.2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--num_test', type=int, default=8)
    ap.add_argument('--batch_size', type=int, default=1)
    ap.add_argument('--checkpoint', default=None, help='state_dict of the GNN to evaluate')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    test = MeshDataset([21], a.num_test, seed=1, num_gauss=1, burgers=True, target='mmpde5',
                       target_params={'mon_reg': OPT['mon_reg'], 'mon_power': OPT['mon_power']})
    opt = dict(OPT, device=str(dev))
    for seed in (0, 1):
        torch.manual_seed(seed)
        model = GNN(test, hot_path_opt(mesh_dims=[21], conv_type='GRAND', hidden_dim=8, gnn_inc_feat_f=False, device=str(dev))).to(dev).eval()
        if a.checkpoint and seed == 0:
            model.load_state_dict(torch.load(a.checkpoint, map_location=dev))
        for name, fn in (('one step', evaluate_model_fine_burgers), ('rollout', evaluate_model_fine_burgers_time_step)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            df, df_time = fn(model, test, opt, batch_size=a.batch_size)
            print(f"model {seed}, {name}: {len(test)} samples in {time.perf_counter() - t0:.2f} s", flush=True)
            for table in (df, df_time):
                print(table.to_string() if hasattr(table, 'to_string') else table, flush=True)


if __name__ == '__main__':
    main()
