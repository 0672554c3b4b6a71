"""The `opt` keys the hot path reads, with the reference's defaults.

The reference threads one plain dict `opt` through every constructor
(`src/params.py:199-303` argparse defaults, then `run_params` overrides
`src/params.py:106-134`).  Only the keys listed in SURVEY.md §5 ("Config /
flags") matter to the model; `hot_path_opt` returns exactly those so callers
(tests, bench, a reference-style training loop) can build models without the
reference's argparse front end.
"""
from __future__ import annotations

BASELINE_MODEL_NAMES = ('fixed_mesh_1D', 'fixed_mesh_2D', 'backFEM_1D', 'backFEM_2D')


def model_defaults(model: str, mesh_dims=None) -> dict:
    """The reference's per-model settings for the network-free baselines (`src/params.py:73-104`); {} for any other model."""
    if model == 'fixed_mesh_1D':                 # params.py:73-76 (its loss_type line is a comparison: nothing is set)
        return {'solver': 'firedrake', 'evaler': 'analytical'}
    if model == 'fixed_mesh_2D':                 # params.py:78-81
        return {'solver': 'firedrake', 'evaler': 'analytical', 'loss_type': 'mesh_loss'}
    if model == 'backFEM_1D':                    # params.py:83-96: the more nodes, the smaller lr must be to stop crossing
        out = {'loss_type': 'pde_loss', 'solver': 'torch_FEM', 'evaler': 'analytical', 'mesh_params': 'internal', 'epochs': 10}
        lr = {11: 0.05, 21: 0.01, 51: 0.001}.get(int(mesh_dims[0])) if mesh_dims else None
        if lr is not None:
            out['lr'] = lr
        return out
    if model == 'backFEM_2D':                    # params.py:98-104
        return {'loss_type': 'pde_loss', 'evaler': 'analytical', 'solver': 'torch_FEM', 'epochs': 200, 'lr': 0.2,
                'load_quad_points': 101}
    return {}


def hot_path_opt(**overrides) -> dict:
    opt = {
        # mesh / data
        'mesh_dims': [11, 11],              # params.py:37
        'data_type': 'randg',               # params.py:30
        'fix_boundary': True,               # params.py:67
        'eval_quad_points': 101,            # params.py:68
        # not a reference key: the FEM route of the evaluation (evaluate_model_fine, eval_grid_MMPDE_MA) and of the differentiable
        # tails (pde_loss, the 2-D modular loss, torch_FEM_2D).  'lds': the banded factor resident in LDS, 2-D meshes up to
        # 26 x 26; 'window': the windowed band solve, up to 81 x 81
        'fem_band': 'lds',
        # not a reference key: the form of the two lattice walks in the backward of those tails.  'lane': a lane per node and per
        # triangle; 'wave': a wave each (gadapt_fem_backward_wave), the same gradient bit for bit.  backFEM_2D's mesh descent
        # reads it too (mesh_descent_2d(adjoint=...), gadapt_fem_descend_wave)
        'fem_adjoint': 'lane',
        # not a reference key: the form of the load vector and the lattice evaluation in the forward of those tails, on
        # fem_band='lds'.  'lane': a lane per node and five lattice points per lane; 'wave': a wave per node and per chunk of the
        # lattice (gadapt_fem_forward_wave), the same coeffs, factor and sol bit for bit.  'wave' with fem_band='window' is refused.
        # The evaluation (evaluate_model_fine, eval_grid_MMPDE_MA: poisson_eval_errors(forward=...), gadapt_fem_eval_errors_wave)
        # and backFEM_2D's mesh descent (mesh_descent_2d(forward=...)) read it too, with the same error norms and meshes
        'fem_forward': 'lane',
        # not a reference key: loss_type='pde_loss' on 1-D Poisson models (torch_FEM_1D per mesh, fem1d.gnn_pde_tail_1d).  False:
        # such a model is refused, as before the tail was built
        'pde_loss_1d': False,
        # not a reference key: how training.GraphedTrainStep runs that tail.  'split': the solve, the loss launch and the adjoint
        # solve (three launches); 'fused': gadapt_fem_poisson1d_loss, one launch, with the package's l1_loss / mse_loss only
        'fem1d_tail': 'split',
        # not a reference key: the route of the MMPDE5 target meshes that the examples build (`target_params={'solver':
        # {'route': ...}}` of the datasets).  'lane': one node per lane, 2-D meshes up to 32 x 32; 'strided': up to 81 x 81
        'mmpde5_route': 'lane',
        # not a reference key: the route of the Monge-Ampere target meshes that the examples build, passed on in the same way.
        # 'lane': one node per lane and an fp32 potential, up to 32 x 32; 'strided': an fp64 potential, up to 81 x 81
        'ma_route': 'lane',
        # features
        'gnn_inc_feat_f': True,             # params.py:114
        'gnn_inc_feat_uu': True,            # params.py:115
        'gnn_inc_glob_feat_f': False,       # params.py:116
        'gnn_inc_glob_feat_uu': False,      # params.py:117
        'gnn_normalize': False,             # params.py:118
        'global_feat_dim': 8,               # params.py:133
        # not a reference key: what computes the global CNN features.  'torch': the Conv modules (MIOpen); 'hip': the one-launch
        # kernels of features.global_cnn (images whose LDS copies fit 64 KB, else an error); 'auto': 'hip' where it fits
        'glob_feat_kernel': 'torch',
        # model
        'conv_type': 'GRAND_plus',          # params.py:121
        'gat_plus_type': 'GAT_res_lap',     # params.py:122
        'enc': 'identity', 'dec': 'identity',
        'residual': True,                   # params.py:127
        'share_conv': True,                 # params.py:128
        'non_lin': 'identity',              # params.py:129
        'num_layers': 4,                    # params.py:130
        'time_step': 0.1,                   # params.py:131
        'hidden_dim': 8,                    # params.py:132
        'learn_step': False,                # params.py:267
        'self_loops': False,                # params.py:264
        'softmax_temp_type': None,          # params.py:265
        'softmax_temp': 2.0,                # params.py:266
        'reg_skew': False,                  # params.py:269
        'dropout': 0.0,                     # params.py:287
        # training
        'loss_type': 'mesh_loss',           # params.py:289 (run_params sets pde_loss: 2-D Poisson, g_adaptivity_amd/fem.py)
        'loss_fn': 'mse',
        'lr': 0.001, 'decay': 0.0,
        'device': 'cpu',
        # params.py:298 declares the string "True"; the pipeline's tf_sweep_args (params.py:172-177, run_pipeline.py:96-100)
        # turns it into the bool True before any model is built, and a bool makes GRAND_plusConv keep
        # stored_ei / stored_alpha (GRAND_plus.py:253).  Pass the string 'False' (or any non-bool) to skip that.
        'show_mesh_evol_plots': True,
        # not a reference key: False materialises the zero-padded encoder output, the full last-layer output and the padded
        # top gradient (the literal GNN.py:270,299 data flow) instead of their compact forms
        'compact_slots': True,
    }
    if overrides.get('model') in BASELINE_MODEL_NAMES:     # read only when a baseline is named; explicit overrides still win
        opt.update(stiff_quad_points=3, load_quad_points=101)                            # params.py:69-70
        opt.update(model_defaults(overrides['model'], overrides.get('mesh_dims', opt['mesh_dims'])))
    opt.update(overrides)
    return opt
