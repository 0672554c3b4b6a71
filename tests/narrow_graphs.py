"""Case builders for the narrow route's fp64 anchors (tests/test_narrow_graphs_host.py, tests/test_gpu_narrow_graphs.py).

The narrow route (DESIGN.md sections 4 and 5) runs GRAND_plus at hidden 64 on [N,4] slots wherever the wide forward takes the graph.
The cases below are the graphs and option sets the route accepts but that no clean square `MeshDataset` batch with default options
produces: ragged in- and out-rows (out-rows past the ELL-8 table: the CSR loops of the source passes), in-rows of 7, a fixed
temperature, mixed mesh sizes, the 512-row window, the eight-wave geometry on a ragged node count, and 1-D meshes.

Every case is a row of `CASES`; `build(case_id)` returns the seeded batch, the fp32 oracle and its fp64 twin with their `mse_loss`
backward done - computed once per process and shared (nothing in it is written to afterwards).  `edit_edges` edits the collated batch
itself (`edge_index` and the three per-edge masks together), so the oracle and `GNN.forward`, which both start from those fields, see
the same graph.
"""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from helpers import oracle_fp64_twin, rel_err
from g_adaptivity_amd import MeshDataset, MixedMeshDataset, collate, hot_path_opt
from oracle.pyg_restatement import OracleGNN

EDGE_MASKS = ('to_boundary_edge_mask', 'to_corner_nodes_mask', 'diff_boundary_edges_mask')
PARAMETERS = ('lin_query.weight', 'lin_query.bias', 'lin_key.weight')
COORD_TOL = 1e-5
GRAD_TOL = 1e-4
QUIET = 0.5 * GRAD_TOL                      # a case is quiet when the fp32 oracle stays below this on every parameter


def edit_edges(data, drop=None, add=None):
    """The batch with edges dropped (`drop`: bool [E], True = remove) and then appended (`add` = (src, dst), two equal-length index
    lists) - `edge_index` and the three per-edge masks together; added edges get False in every mask."""
    d = data.clone()
    e = d.edge_index.shape[1]
    keep = torch.ones(e, dtype=torch.bool) if drop is None else ~torch.as_tensor(drop, dtype=torch.bool)
    assert keep.shape == (e,)
    src, dst = ([], []) if add is None else add
    extra = torch.tensor([list(src), list(dst)], dtype=d.edge_index.dtype).reshape(2, -1)
    assert extra.numel() == 0 or (0 <= int(extra.min()) and int(extra.max()) < d.x_comp.shape[0])
    d.edge_index = torch.cat([d.edge_index[:, keep], extra], dim=1).contiguous()
    for m in EDGE_MASKS:
        old = getattr(d, m)
        assert old.shape == (e,)
        setattr(d, m, torch.cat([old[keep], torch.zeros(extra.shape[1], dtype=old.dtype)]))
    return d


def ragged_edits(data):
    """The edits of the `ragged` case on a collated 20 x 20 batch of 4 (nodes 42, 90, 104, 106, ... are interior nodes of mesh 0, 611 of
    mesh 1): in-rows of 0 (42, 611), 1 (90), 7 (106, and the eight targets of 210), 8 (206); out-rows of 0 (130) and 14 (210)."""
    src, dst = data.edge_index
    drop = (dst == 42) | (dst == 611) | ((dst == 90) & (src != 89)) | (src == 130)
    fan = [164, 166, 168, 170, 244, 246, 248, 250]
    return edit_edges(data, drop=drop, add=([204, 208, 104] + [210] * len(fan), [206, 206, 106] + fan))


# id -> what the case is and what it claims.  `deg_t` / `deg_s`: (min, max) in- / out-degree of the graph the conv layers see;
# `big`: the wide forward's 512-row window (wide_deg['t'] == 0, wide_big_deg > 0); `half`: the four-wave geometry (wide_half_deg > 0);
# `ell_s`: the out-rows fit the ELL-8 table (wide_deg['s'] > 0); `half_max`: the value of graph.WIDE_HALF_MAX_NODES the case runs under
# (None: the module's).
def _case(dims, batch, layers, seed, deg_t, deg_s, nodes, big=False, half=True, ell_s=True, half_max=None, edits=None, scale=1.0,
          mixed=None, **opt):
    return SimpleNamespace(dims=tuple(dims), batch=batch, layers=layers, seed=seed, deg_t=deg_t, deg_s=deg_s, nodes=nodes, big=big, half=half,
                           ell_s=ell_s, half_max=half_max, edits=edits, scale=scale, mixed=mixed, opt=opt)


CASES = {
    'ragged': _case((20, 20), 4, 3, 6, (0, 8), (0, 14), 1600, ell_s=False, edits=ragged_edits),
    'loops7': _case((23, 23), 3, 3, 0, (3, 7), (3, 7), 1587, fix_boundary=False, self_loops=True),
    'temp2': _case((23, 23), 3, 3, 0, (1, 6), (2, 6), 1587, softmax_temp_type='fixed', softmax_temp=2.0),
    'rebase-ragged': _case((20, 20), 4, 3, 6, (0, 8), (0, 14), 1600, ell_s=False, edits=ragged_edits, scale=4.0),
    'mixed': _case((23, 23), 6, 3, 1, (1, 6), (2, 6), 12450, mixed=[23, 40, 64]),
    'big65': _case((65, 65), 1, 2, 3, (1, 6), (2, 6), 4225, big=True, half=False),
    'big100': _case((100, 100), 1, 2, 2, (1, 6), (2, 6), 10000, big=True, half=False),
    'eight-wave': _case((23, 23), 7, 3, 0, (1, 6), (2, 6), 3703, half=False, half_max=0),
    'eight-wave-64': _case((64, 64), 9, 2, 4, (1, 6), (2, 6), 36864, half=False),
    '1d-21': _case((21,), 13, 3, 0, (1, 2), (1, 2), 273),
    '1d-21-burgers': _case((21,), 13, 3, 1, (1, 2), (1, 2), 273, gnn_inc_feat_f=False),
    '1d-65-open': _case((65,), 5, 3, 1, (1, 2), (1, 2), 325, fix_boundary=False),
}
IDS = list(CASES)


def target_of(data):
    return data.x_phys if data.x_phys.dim() == 2 else data.x_phys.unsqueeze(-1)


@functools.lru_cache(maxsize=None)
def build(case_id):
    """The case's options, dataset, batch, fp32 oracle and fp64 twin (both after forward + `mse_loss` backward), the outputs `ref` /
    `ref64` and `noise`: {parameter: fp32 oracle against fp64, normwise}."""
    c = CASES[case_id]
    opt = hot_path_opt(mesh_dims=list(c.dims), hidden_dim=64, num_layers=c.layers, conv_type='GRAND_plus', **c.opt)
    ds = MixedMeshDataset(c.mixed, c.batch, seed=c.seed) if c.mixed else MeshDataset(c.dims, c.batch, seed=c.seed)
    data = collate(ds.samples)
    if c.edits is not None:
        data = c.edits(data)
    torch.manual_seed(c.seed)
    oracle = OracleGNN(ds, dict(opt))
    if c.scale != 1.0:                                           # scores spread far enough for the softmax to re-base
        with torch.no_grad():
            oracle.conv_layers[0].lin_query.weight.mul_(c.scale)
            oracle.conv_layers[0].lin_key.weight.mul_(c.scale)
    tgt = target_of(data)
    ref = oracle(data)
    loss = F.mse_loss(ref, tgt)
    loss.backward()
    o64, ref64 = oracle_fp64_twin(oracle, ds, opt, data, tgt)
    g32, g64 = (dict(m.conv_layers[0].named_parameters()) for m in (oracle, o64))
    noise = {k: rel_err(g32[k].grad, g64[k].grad)[0] for k in PARAMETERS}
    losses = {}
    for name, fn in (('mse', F.mse_loss), ('l1', F.l1_loss)):
        with torch.no_grad():
            losses[name] = (fn(ref, tgt).item(), fn(ref64, tgt.double()).item())
    return SimpleNamespace(case=c, opt=opt, ds=ds, data=data, tgt=tgt, oracle=oracle, o64=o64, ref=ref.detach(), ref64=ref64.detach(),
                           g32={k: g32[k].grad for k in PARAMETERS}, g64={k: g64[k].grad for k in PARAMETERS}, noise=noise, losses=losses)


def degrees(graph):
    """((min, max) in-degree, (min, max) out-degree) of a MeshGraph."""
    dt = (graph.rowptr_t[1:] - graph.rowptr_t[:-1]).cpu()
    ds_ = (graph.rowptr_s[1:] - graph.rowptr_s[:-1]).cpu()
    return (int(dt.min()), int(dt.max())), (int(ds_.min()), int(ds_.max()))
