"""MI355X-native message-passing hot path of g-adaptivity (GNN.py / GRAND_plus.py).

Public surface mirrors the reference modules:
    from g_adaptivity_amd import GNN, get_conv, GRAND_plusConv, GRAND_conv
    from g_adaptivity_amd import mse_loss, l1_loss          # the training loop's loss_fn, one launch each
    from g_adaptivity_amd import torch_FEM_2D, fem_poisson   # loss_type='pde_loss': the differentiable P1 FEM tail
    from g_adaptivity_amd import gradient_meshpoints_1D, burgers_1d, fem_poisson_1d   # the 1-D modular loss (Burgers, Poisson)
    from g_adaptivity_amd import gradient_meshpoints_2D    # the 2-D modular loss (Poisson)
    from g_adaptivity_amd import MMPDE5_1d, MMPDE5_2d, mmpde5_batch   # the classical MMPDE5 target meshes, batched
    from g_adaptivity_amd import MA2d, deform_mesh_ma2d, ma_batch   # Monge-Ampere target meshes (2-D), finite differences, batched
    from g_adaptivity_amd import evaluate_model_fine, eval_grid_MMPDE_MA, poisson_eval_errors   # the Poisson error-reduction tables
    from g_adaptivity_amd import evaluate_model_fine_burgers, evaluate_model_fine_burgers_time_step   # the Burgers one-step and rollout tables
    from g_adaptivity_amd import cubic_spline_1d            # batched not-a-knot cubic splines (scipy's UnivariateSpline(s=0))
    from g_adaptivity_amd import backFEM_2D, backFEM_1D, Fixed_Mesh_2D, Fixed_Mesh_1D, get_model   # the network-free baselines
    from g_adaptivity_amd import mesh_descent_2d, mesh_descent_1d   # their loop: SGD of the mesh nodes on the FEM error, one call
The arithmetic lives in `libgadapt_hip.so` (csrc/, C-ABI in include/gadapt_hip.h) and, for the FEM tail,
`libgadapt_fem.so` (fem_csrc/, include/gadapt_fem.h); the MMPDE5 generator in `libgadapt_mesh.so` (mesh_csrc/, include/gadapt_mesh.h).
"""
from .baselines import Fixed_Mesh_1D, Fixed_Mesh_2D, backFEM_1D, backFEM_2D, get_model
from .conv import GAT_conv, GAT_plus, GCN_conv, GRAND_conv, GRAND_plusConv, TRANS_conv
from .descent import DescentResult, mesh_descent_1d, mesh_descent_2d
from .evaluation import (calculate_error_reduction, eval_grid_MMPDE_MA, evaluate_error_np, evaluate_error_np_2d, evaluate_model_fine,
                         poisson_eval_errors)
from .evaluation_burgers import burgers_project, evaluate_model_fine_burgers, evaluate_model_fine_burgers_time_step
from .fem import fem_poisson, gradient_meshpoints_2D, torch_FEM_2D
from .fem1d import (burgers_1d, fem_poisson_1d, fn_expansion, get_Burgers_initial_coeffs, gradient_meshpoints_1D, torch_FEM_1D,
                    torch_FEM_Burgers_1D)
from .functional import l1_loss, mse_loss, unit_gradient
from .gnn import GNN, MLP, build_conv_list, get_conv, get_dec, get_enc, get_mlp, get_nonlin
from .graph import GraphCache, MeshGraph, prepare_edge_index
from .mesh_graph import (DeviceMeshLoader, MeshData, MeshDataset, MeshLoader, Mixed_DataLoader, MixedMeshDataset, collate, interval_mesh,
                         square_mesh, synthetic_batch)
from .mmpde5 import (MMPDE5_1d, MMPDE5_1d_burgers, MMPDE5_2d, deform_mesh_mmpde1d, deform_mesh_mmpde2d, mmpde5_batch, monitor_1d,
                     monitor_2d)
from .monge_ampere import (MA2d, MAResult, MASlowResult, attach_ma_targets, deform_mesh_ma2d, ma_batch, ma_table_batch, monitor_from_nodal,
                           monitor_m2n, monitor_m2n_slow, monitor_ma, monitor_table)
from .params import hot_path_opt, model_defaults
from .spline import cubic_spline_1d
from .training import GraphedTrainStep

__all__ = ['GNN', 'MLP', 'get_conv', 'build_conv_list', 'get_enc', 'get_dec', 'get_mlp', 'get_nonlin',
           'GRAND_plusConv', 'GRAND_conv', 'TRANS_conv', 'GAT_plus', 'GAT_conv', 'GCN_conv', 'MeshGraph', 'GraphCache', 'prepare_edge_index',
           'MeshData', 'MeshDataset', 'MeshLoader', 'DeviceMeshLoader', 'MixedMeshDataset', 'Mixed_DataLoader', 'collate', 'interval_mesh', 'square_mesh',
           'synthetic_batch', 'hot_path_opt', 'GraphedTrainStep', 'mse_loss', 'l1_loss', 'unit_gradient',
           'fem_poisson', 'torch_FEM_2D', 'burgers_1d', 'fem_poisson_1d', 'gradient_meshpoints_1D', 'torch_FEM_Burgers_1D',
           'get_Burgers_initial_coeffs', 'fn_expansion', 'torch_FEM_1D', 'gradient_meshpoints_2D',
           'mmpde5_batch', 'monitor_1d', 'monitor_2d', 'MMPDE5_1d', 'MMPDE5_2d', 'MMPDE5_1d_burgers', 'deform_mesh_mmpde1d',
           'deform_mesh_mmpde2d', 'ma_batch', 'ma_table_batch', 'monitor_table', 'monitor_from_nodal', 'monitor_ma', 'monitor_m2n', 'monitor_m2n_slow', 'MA2d', 'MAResult', 'MASlowResult', 'deform_mesh_ma2d', 'attach_ma_targets', 'poisson_eval_errors', 'eval_grid_MMPDE_MA', 'evaluate_model_fine', 'evaluate_error_np',
           'evaluate_error_np_2d', 'calculate_error_reduction', 'cubic_spline_1d', 'evaluate_model_fine_burgers',
           'evaluate_model_fine_burgers_time_step', 'burgers_project', 'backFEM_2D', 'backFEM_1D', 'Fixed_Mesh_2D', 'Fixed_Mesh_1D',
           'get_model', 'mesh_descent_2d', 'mesh_descent_1d', 'DescentResult', 'model_defaults']
