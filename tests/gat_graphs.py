"""Case builders and the fp64 restatement for the fused GAT_plus block (tests/test_gat_graphs_host.py, tests/test_gpu_gat_graphs.py).

`functional.gat_plus_block` runs `conv_type='GAT_plus'` as one block op over the kernels of csrc/gadapt_gat.inc.  Its backward has a
launch plan that depends on the node count alone: with SLOTS = 256 / LPN nodes per workgroup (256, 128, 64, 64, 32, 16 at C = 4, 8,
16, 32, 64, 128) the source pass runs on `rows = min(round_up_8(ceil(n / SLOTS)), 1024)` workgroups (`s_blocks()`), each walking
`per_blk = ceil(ceil(n / SLOTS) / rows)` node groups and writing one partial row, and `reduce_kernel` sums the `rows` partial rows -
in a four-accumulator loop once `rows >= 104`.  The cases below are the smallest graphs at which each of those paths runs, plus the
graphs the operator had never met: union-jack meshes (in-rows of 9 beside rows of 3..6), mixed mesh sizes, 1-D chains, widely spread
scores.

A graph is a tuple of parts - ('sq', k) a k x k `square_mesh`, ('uj', k) a `union_jack(k)`, ('chain', m) m nodes in a row,
('random', n) the random graph of `test_gat_plus_block_on_any_graph` - laid one after the other like a collated batch.  Every case is
a row of `CASES` with its literal claims; `build(case_id)` returns the graph and the seeded inputs, `reference(case_id, S, dtype)` the
restatement's outputs - both computed once per process and shared (nothing in them is written to afterwards).
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from fem_meshes import union_jack
from helpers import make_case, rel_err
from g_adaptivity_amd import MeshGraph, MixedMeshDataset, collate, hot_path_opt
from g_adaptivity_amd.mesh_graph import square_mesh
from oracle.pyg_restatement import _NONLIN, OracleGNN, gat_plus

COORD_TOL = 1e-5                            # floor of x_L and alpha
GRAD_TOL = 1e-4                             # floor of d x0, d att_src, d att_dst
QUIET = 0.5 * GRAD_TOL                      # a model-route case is quiet when the fp32 oracle stays below this on every parameter
QUANTITIES = ('x_L', 'alpha', 'd x0', 'd att_src', 'd att_dst')
FLOORS = dict(zip(QUANTITIES, (COORD_TOL, COORD_TOL, GRAD_TOL, GRAD_TOL, GRAD_TOL)))
NON_LINS = ('identity', 'relu', 'tanh', 'sigmoid', 'leaky_relu', 'elu', 'selu')
L, DT = 3, 0.1
S_MAX_BLOCKS = 1024


def lanes_per_node(c):
    return c // 8 if c >= 32 else c // 4


def plan(n, c):
    """(rows, per_blk, n_blocks) of the launch plan, restated: `s_blocks()`, `bwd_s_kernel`'s `per_blk`, `block_forward`'s `n_blocks`."""
    slots = 256 // lanes_per_node(c)
    groups = -(-n // slots)
    rows = min((groups + 7) // 8 * 8, S_MAX_BLOCKS)
    return rows, -(-groups // rows), -(-n * lanes_per_node(c) // 256)


# ---- graphs -------------------------------------------------------------------------------------------------------------------------

def chain_edges(m):
    """m nodes in a row, edges (i, i+1) in both directions; one node: no edge."""
    i = torch.arange(m - 1)
    return torch.cat([torch.stack([i, i + 1]), torch.stack([i + 1, i])], dim=1)


@functools.lru_cache(maxsize=None)
def square_edges(k):
    return square_mesh(k).edge_index.clone()


@functools.lru_cache(maxsize=None)
def union_jack_edges(k):
    """The edges of `union_jack(k)`'s triangles, both directions, sorted and deduplicated as `square_mesh` does it."""
    cells = union_jack(k)[1].numpy()
    pairs = np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [0, 2]]], 0)
    pairs = np.unique(np.concatenate([pairs, pairs[:, ::-1]], 0), axis=0)
    return torch.from_numpy(pairs.T.copy())


def random_edges(n):
    """The graph of `test_gat_plus_block_on_any_graph` on n nodes: 4000 random edges, node 3 sends to 100..139, nodes 200..229 send
    to node 11, node 17 keeps no in-edge; self-loops removed."""
    assert n >= 230
    gen = torch.Generator().manual_seed(5)
    ei = torch.randint(0, n, (2, 4000), generator=gen)
    ei = torch.cat([ei, torch.tensor([[3] * 40, list(range(100, 140))]), torch.tensor([list(range(200, 230)), [11] * 30])], dim=1)
    return ei[:, (ei[1] != 17) & (ei[0] != ei[1])]


PART_NODES = {'sq': lambda k: k * k, 'uj': lambda k: k * k, 'chain': lambda m: m, 'random': lambda n: n}
PART_EDGES = {'sq': square_edges, 'uj': union_jack_edges, 'chain': chain_edges, 'random': random_edges}


def graph_of(parts):
    """(edge_index [2,E], n, the first node of every part and n at the end) of the parts laid one after the other."""
    ptr, eis = [0], []
    for kind, size in parts:
        eis.append(PART_EDGES[kind](size) + ptr[-1])
        ptr.append(ptr[-1] + PART_NODES[kind](size))
    return torch.cat(eis, dim=1).contiguous(), ptr[-1], ptr


def squares(*ks):
    return tuple(('sq', k) for k in ks)


def filled(n, *ks):
    """Square meshes of the given sides and a chain after them that brings the graph to exactly n nodes."""
    rest = n - sum(k * k for k in ks)
    assert rest >= 2
    return squares(*ks) + (('chain', rest),)


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# `rows` = the partial rows (= source-pass workgroups), `per_blk` node groups per workgroup, `n_blocks` = ceil(n LPN / 256),
# `deg` = (min, max) in-degree of the self-looped graph, `shared`: also run with one shared pair of vectors (S = 1: `reduce_kernel`
# accumulates the layers' sums), `scale` multiplies att_src and att_dst, `lone` = a node whose only in-edge is its self-loop.
def _case(c, parts, n, rows, per_blk, n_blocks, deg, shared=False, scale=1.0, lone=None):
    return SimpleNamespace(c=c, parts=tuple(parts), n=n, rows=rows, per_blk=per_blk, n_blocks=n_blocks, deg=deg, shared=shared, scale=scale,
                           lone=lone)


CASES = {
    # reduce_kernel at C = 128 (16 nodes per workgroup): tail loop only / unrolled trip for row lanes 0..7 only / one unrolled trip and
    # no tail / both
    'reduce-96': _case(128, filled(1536, 22, 22, 22), 1536, 96, 1, 96, (2, 7), shared=True),
    'reduce-104': _case(128, filled(1537, 22, 22, 22), 1537, 104, 1, 97, (2, 7), shared=True),
    'reduce-128': _case(128, filled(2048, 22, 22, 22, 22), 2048, 128, 1, 128, (2, 7), shared=True),
    'reduce-136': _case(128, filled(2049, 22, 22, 22, 22), 2049, 136, 1, 129, (2, 7), shared=True),
    # rows 104 at every lane split
    'reduce-c64': _case(64, filled(3073, 40, 38), 3073, 104, 1, 97, (2, 7)),
    'reduce-c32': _case(32, filled(6145, 64, 45), 6145, 104, 1, 97, (2, 7)),
    'reduce-c16': _case(16, filled(6145, 64, 45), 6145, 104, 1, 97, (2, 7)),
    'reduce-c8': _case(8, filled(12289, 64, 64, 63), 12289, 104, 1, 97, (2, 7)),
    'reduce-c4': _case(4, filled(24577, 64, 64, 64, 64, 64, 63), 24577, 104, 1, 97, (2, 7)),
    # the cap of 1024 workgroups, then two and three node groups per workgroup
    'cap-1016': _case(128, filled(16256, 64, 64, 64, 62), 16256, 1016, 1, 1016, (2, 7)),
    'cap-1024': _case(128, filled(16384, 64, 64, 64, 63), 16384, 1024, 1, 1024, (2, 7)),
    'two-groups': _case(128, filled(16385, 64, 64, 64, 63), 16385, 1024, 2, 1025, (2, 7), shared=True),      # 513 busy, 511 write zeros
    'three-groups': _case(128, filled(32769, 64, 64, 64, 64, 64, 64, 64, 63), 32769, 1024, 3, 2049, (2, 7)),
    'two-groups-c64': _case(64, squares(*[64] * 9), 36864, 1024, 2, 1152, (3, 7)),                         # the benchmarked width
    # one workgroup; the grid rounded up to 8 blocks, and xcd_block past n_blocks
    'tiny-c4': _case(4, (('chain', 3),), 3, 8, 1, 1, (2, 3)),
    'tiny-c128': _case(128, (('chain', 3),), 3, 8, 1, 1, (2, 3)),
    'blocks-8': _case(64, filled(256, 15), 256, 8, 1, 8, (2, 7)),
    'blocks-9': _case(64, filled(257, 15), 257, 16, 1, 9, (2, 7)),
    # rows of 9 (valence 8 and the self-loop: the CSR loops) beside rows of 3..6 (the unrolled path) in one wave
    'union-jack-c8': _case(8, (('uj', 12),) * 3, 432, 8, 1, 4, (3, 9)),
    'union-jack-c64': _case(64, (('uj', 12),) * 3, 432, 16, 1, 14, (3, 9)),
    'mixed': _case(64, squares(9, 23, 40) + (('chain', 21), ('uj', 9)), 2312, 80, 1, 73, (2, 9)),
    '1d': _case(16, (('chain', 21),) * 13, 273, 8, 1, 5, (2, 3)),
    # node 11: an in-row of 35 (30 hub edges, the self-loop and the 4 edges the seed sends there besides); node 17: the self-loop alone
    'random-c8': _case(8, (('random', 777),), 777, 8, 1, 7, (1, 35), lone=17),
    'random-c64': _case(64, (('random', 777),), 777, 32, 1, 25, (1, 35), lone=17),
    'random-c128': _case(128, (('random', 777),), 777, 56, 1, 49, (1, 35), lone=17),
    # att_src, att_dst x 8: the weights of a row spread over up to thirteen decades (no `exp` reaches fp32's underflow at this factor)
    'spread': _case(128, filled(1537, 22, 22, 22), 1537, 104, 1, 97, (2, 7), scale=8.0),
}
IDS = list(CASES)
RUNS = [(cid, L) for cid in IDS] + [(cid, 1) for cid in IDS if CASES[cid].shared]          # (case, S): S = L per-layer vectors, 1 shared
RUN_IDS = [cid if s == L else cid + '-shared' for cid, s in RUNS]


def in_degrees(graph):
    """In-degree of every node of a MeshGraph, on the host."""
    return (graph.rowptr_t[1:] - graph.rowptr_t[:-1]).cpu()


def inputs(n, c, seed, scale=1.0):
    """Seeded x0 [n,c], up [n,c] and per S in (L, 1) the vectors (att_src, att_dst) [S,c], normal / sqrt(c) as glorot leaves them."""
    gen = torch.Generator().manual_seed(seed)
    x0, up = torch.randn(n, c, generator=gen), torch.randn(n, c, generator=gen)
    att = {s: tuple(scale * torch.randn(s, c, generator=gen) / math.sqrt(c) for _ in range(2)) for s in (L, 1)}
    return x0, up, att


@functools.lru_cache(maxsize=None)
def build(case_id):
    """The case, its edge list, the part boundaries, the self-looped MeshGraph on the host and the seeded inputs."""
    c = CASES[case_id]
    ei, n, ptr = graph_of(c.parts)
    looped = MeshGraph(ei, n, 'cpu').with_self_loops()
    x0, up, att = inputs(n, c.c, IDS.index(case_id), c.scale)
    return SimpleNamespace(case=c, id=case_id, ei=ei, n=n, ptr=ptr, looped=looped, x0=x0, up=up, att=att)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------

def block_restated(x0, edge_index, att_src, att_dst, L, dt, residual, res_lap, non_lin, dtype, up=None, order=None):  # noqa: N803
    """L iterations of `oracle.pyg_restatement.gat_plus` with the update of `src/GNN.py:284-296` (x + dt nl(res), or nl(res) without
    `residual`), in `dtype`, with autograd on (x_L * up).sum().  att_src / att_dst: [S,C], S = 1 (shared) or L.  Returns x_L, the last
    layer's alpha and the gradients with respect to x0, att_src, att_dst.  `gat_plus` appends the self-loops itself, in the order of
    `MeshGraph.with_self_loops()`; `order` (the looped graph's `eid_t`: target-CSR slot -> edge) brings alpha into target-CSR order."""
    x = x0.detach().to(dtype).requires_grad_(True)
    s_, d_ = (t.detach().to(dtype).requires_grad_(True) for t in (att_src, att_dst))
    S = s_.shape[0]  # noqa: N806
    assert S in (1, L) and d_.shape == s_.shape
    kind, nl = ('GAT_res_lap' if res_lap else 'GAT_lin'), _NONLIN[non_lin]
    y = x
    for layer in range(L):
        k = layer if S > 1 else 0
        res, (_, alpha) = gat_plus(y, edge_index, s_[k].view(1, 1, -1), d_[k].view(1, 1, -1), kind)
        y = y + dt * nl(res) if residual else nl(res)
    if up is None:
        up = torch.randn(x.shape, generator=torch.Generator().manual_seed(0))
    (y * up.to(dtype)).sum().backward()
    alpha = alpha.detach().reshape(-1)
    if order is not None:
        alpha = alpha[order.long().cpu()]
    return y.detach(), alpha, x.grad, s_.grad, d_.grad


@functools.lru_cache(maxsize=None)
def reference(case_id, S=L, dtype_name='float64', residual=True, res_lap=True, non_lin='tanh'):  # noqa: N803
    """{quantity: tensor} of `block_restated` on the case; alpha in the target-CSR order of the looped graph."""
    b = build(case_id)
    out = block_restated(b.x0, b.ei, *b.att[S], L, DT, residual, res_lap, non_lin, getattr(torch, dtype_name), up=b.up,
                         order=b.looped.eid_t[:b.looped.num_edges])
    return dict(zip(QUANTITIES, out))


def noise_of(case_id, S=L, **form):  # noqa: N803
    """{quantity: the fp32 restatement against the fp64 one, normwise}."""
    r32, r64 = reference(case_id, S, 'float32', **form), reference(case_id, S, 'float64', **form)
    return {q: rel_err(r32[q], r64[q])[0] for q in QUANTITIES}


# ---- the cases that go through GNN.forward ------------------------------------------------------------------------------------------
# d att_dst is a sum of per-node terms that vanish wherever the scores of an in-row share a sign (the softmax's shift invariance, up to
# leaky_relu's two slopes), so on a smooth mesh it is a small difference of rounding residues: on most seeds the fp32 oracle itself
# stands 1e-4 .. 4e-3 from fp64 there and moves as much with the edge order.  The seeds and the sharing below are the first, counted
# from seed 0, at which the fp32 oracle is quiet - below QUIET on every parameter, as run and over four edge orders
# (tests/test_gat_graphs_host.py) - chosen by the oracle's own noise alone.
MODEL_ROUTES = {
    '64x64-batch-9': SimpleNamespace(dims=(64, 64), batch=9, hidden=64, layers=2, seed=3, share=True, mixed=None, nodes=36864),
    'mixed-23-40-64': SimpleNamespace(dims=(23, 23), batch=6, hidden=64, layers=3, seed=3, share=True, mixed=(23, 40, 64), nodes=12450),
    '1d-21-batch-13': SimpleNamespace(dims=(21,), batch=13, hidden=16, layers=3, seed=1, share=False, mixed=None, nodes=273),
}


def model_case(route):
    """(opt, dataset, batch, fp32 oracle) of a model-route case, as `helpers.make_case` returns them - built anew at every call (the
    caller runs the oracle's backward).  The mixed batch is built as `narrow_graphs.build` builds its own; a 1-D target is [N,1], the
    shape of the model's output."""
    r = MODEL_ROUTES[route]
    extra = dict(non_lin='tanh', share_conv=r.share)
    if r.mixed is None:
        opt, ds, data, oracle = make_case(r.dims, r.batch, r.hidden, r.layers, 'GAT_plus', seed=r.seed, **extra)
    else:
        opt = hot_path_opt(mesh_dims=list(r.dims), hidden_dim=r.hidden, num_layers=r.layers, conv_type='GAT_plus', **extra)
        ds = MixedMeshDataset(list(r.mixed), r.batch, seed=r.seed)
        data = collate(ds.samples)
        torch.manual_seed(r.seed)
        oracle = OracleGNN(ds, dict(opt))
    if data.x_phys.dim() == 1:
        data.x_phys = data.x_phys.unsqueeze(-1)
    return opt, ds, data, oracle
