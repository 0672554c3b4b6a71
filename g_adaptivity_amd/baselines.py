"""The reference's network-free baselines: `backFEM_2D`, `backFEM_1D`, `Fixed_Mesh_2D`, `Fixed_Mesh_1D`, and `get_model`.

`--model` of the reference takes six values (`src/params.py:241`, `src/run_pipeline.py:20-31`): GNN, MLP, fixed_mesh_1D,
fixed_mesh_2D, backFEM_1D, backFEM_2D.  `Fixed_Mesh_*` returns the unmoved grid; `backFEM_*` moves the mesh points
themselves by gradient descent on the FEM error (`firedrake_difFEM/difFEM_2d.py:688-731`, `difFEM_1d.py:295-334`).  They are
what the tables of `evaluate_model_fine` are read against.  Here a whole batch descends at once (`descent.mesh_descent_2d`,
`mesh_descent_1d`: every epoch enqueued by one call), each sample on its own Gaussians, from `data.x_comp` - the uniform
mesh the reference's loops start from.

All four are `nn.Module`s without parameters, stamp `end_MLmodel` after waiting for the stream as `GNN.forward` does, and
keep `loss_list` / `mesh_list` of their last call.
"""
from __future__ import annotations

import time

import torch
from torch import nn

from .descent import mesh_descent_1d, mesh_descent_2d
from .fem import _modular_batch, fem_poisson, simpson_points_per_dim
from .fem1d import _split_params

__all__ = ['backFEM_2D', 'backFEM_1D', 'Fixed_Mesh_2D', 'Fixed_Mesh_1D', 'get_model', 'BASELINE_MODELS']


class _Baseline(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.num_meshpoints = opt['mesh_dims'][0]
        self.end_MLmodel = None
        self.loss_list, self.mesh_list = [], []

    def _stamp(self, t: torch.Tensor):
        if t.is_cuda and not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream(t.device).synchronize()       # the stamp is read as a latency (utils_eval.py:201)
        self.end_MLmodel = time.time()


def _batch_1d(data, n_nodes: int):
    """(node_counts, pde_params per mesh) of a 1-D sample or collated batch."""
    batch = getattr(data, 'batch', None)
    if batch is None:
        return [n_nodes], _split_params(data.pde_params, 1)
    B = int(data.num_graphs)
    return torch.bincount(batch.detach().cpu(), minlength=B).tolist(), _split_params(data.pde_params, B)


class backFEM_2D(_Baseline):
    """SGD of the interior mesh points on the Simpson L2 error of the P1 Poisson solve (`train_step_adjoint`), `opt['epochs']`
    steps of `opt['lr']`, every sample of the batch at once.  `forward(data)` -> (coeffs [N,1], coords [N,2], None).

    coeffs are those of the last epoch's solve, on the mesh before the last step, as the reference returns them.
    `loss_list` is [E,B] and `mesh_list` [E,N,2] of the last call (device tensors), `first_tangled` / `min_area` its
    tangling watch (`descent.DescentResult`).  Quadrature: torchquad's points per dimension of `load_quad_points` for the
    load vector and the loss (101 -> 9, the built rule).  opt['fem_forward'] / opt['fem_adjoint'] = 'wave' run the epochs on the
    wave-parallel kernels (`mesh_descent_2d(forward=..., adjoint=...)`), the same meshes bit for bit."""

    def __init__(self, opt):
        super().__init__(opt)
        self.lr = opt['lr']
        self.epochs = opt['epochs']

    def forward(self, data):
        x0 = data.x_comp
        n = simpson_points_per_dim(self.opt.get('load_quad_points', 101))
        cells, boundary, node_counts, tri_counts, params = _modular_batch(self.opt, data, x0.shape[0])
        res = mesh_descent_2d(x0, cells, boundary, node_counts, params, int(self.epochs), float(self.lr), n_lat=n, n_load=n,
                              keep_meshes=True, tri_counts=tri_counts, forward=self.opt.get('fem_forward', 'lane'),
                              adjoint=self.opt.get('fem_adjoint', 'lane'))
        self.loss_list, self.mesh_list = res.loss_hist, res.mesh_hist
        self.first_tangled, self.min_area = res.first_tangled, res.min_area
        self._stamp(res.x)
        return (None if res.coeffs is None else res.coeffs.unsqueeze(1)), res.x, None


class backFEM_1D(_Baseline):
    """SGD of the 1-D mesh points on the trapezoid L2 error of the Poisson solve (`train_step_vec`); `opt['mesh_params']` is
    'internal' (the ends stay) or 'all' (every node moves, then rescale and clip).  `forward(data)` ->
    (coeffs [N], coords shaped as data.x_comp, sol [B,P]): coeffs (the end values included) and sol are the last epoch's,
    on the mesh before the last step."""

    def __init__(self, opt):
        super().__init__(opt)
        self.eval_quad_points = opt.get('eval_quad_points', 101)
        self.lr = opt['lr']
        self.epochs = opt['epochs']
        self.plot_evol_flag = False

    def forward(self, data):
        x0 = data.x_comp
        node_counts, params = _batch_1d(data, x0.shape[0])
        res = mesh_descent_1d(x0, node_counts, params, self.opt, int(self.epochs), float(self.lr),
                              mesh_params=self.opt.get('mesh_params', 'internal'), keep_meshes=True)
        self.loss_list, self.mesh_list = res.loss_hist, res.mesh_hist
        self.first_tangled, self.min_area = res.first_tangled, res.min_area
        self._stamp(res.x)
        return res.coeffs, res.x.view(x0.shape), res.sol


class Fixed_Mesh_2D(_Baseline):
    """The unmoved grid.  loss_type 'mesh_loss': `forward(data)` -> data.x_comp.  'pde_loss': (coeffs [N,1], x_comp, sol),
    the Poisson solve on x_comp (`fem_poisson`) evaluated on the eval_quad_points^2 lattice.

    The reference builds that lattice with `np.meshgrid` and its default 'xy' indexing (`difFEM_2d.py:716-720`), so its sol
    lists the point (x_j, y_i) at i * n + j: per mesh the transpose of `fem_poisson`'s 'ij' result.  That is what this
    returns ([B * n * n], mesh by mesh)."""

    def __init__(self, opt):
        super().__init__(opt)
        self.n, self.m = opt['mesh_dims'][0], opt['mesh_dims'][1]
        self.num_meshpoints = self.n * self.m
        q = torch.linspace(0, 1, int(opt.get('eval_quad_points', 101)))
        self.quad_points = list(torch.meshgrid(q, q, indexing='ij'))

    def forward(self, data):
        mesh_points = data.x_comp
        loss_type = self.opt['loss_type']
        if loss_type == 'mesh_loss':
            self._stamp(mesh_points)
            return mesh_points
        if loss_type != 'pde_loss':
            raise NotImplementedError(f"Fixed_Mesh_2D: loss_type={loss_type!r}")
        cells, boundary, node_counts, tri_counts, params = _modular_batch(self.opt, data, mesh_points.shape[0])
        with torch.no_grad():
            coeffs, sol = fem_poisson(mesh_points, cells, boundary, node_counts, params, self.quad_points, tri_counts=tri_counts)
        nq = self.quad_points[0].shape[0]
        sol = sol.view(len(node_counts), nq, nq).transpose(1, 2).reshape(-1)
        self._stamp(sol)
        return coeffs, mesh_points, sol


class Fixed_Mesh_1D(_Baseline):
    """The unmoved 1-D grid.  loss_type 'mesh_loss': data.x_comp; 'pde_loss': None, as the reference's `pass` returns."""

    def forward(self, data):
        mesh_points = data.x_comp
        self._stamp(mesh_points)
        if self.opt['loss_type'] == 'mesh_loss':
            return mesh_points
        return None


BASELINE_MODELS = {'fixed_mesh_1D': Fixed_Mesh_1D, 'backFEM_1D': backFEM_1D, 'fixed_mesh_2D': Fixed_Mesh_2D, 'backFEM_2D': backFEM_2D}


def get_model(opt, dataset=None):
    """The model `opt['model']` names (`run_pipeline.get_model`, `run_GNN.get_model`): one of the four baselines, built from
    `opt` alone, else `MLP(dataset, opt)` for 'MLP' and `GNN(dataset, opt)` otherwise (untrained: training is the caller's)."""
    name = opt.get('model', 'GNN')
    if name in BASELINE_MODELS:
        return BASELINE_MODELS[name](opt)
    from .gnn import GNN, MLP
    if dataset is None:
        raise ValueError(f"get_model: model {name!r} needs the dataset")
    return (MLP if name == 'MLP' else GNN)(dataset, opt)
