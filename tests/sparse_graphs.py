"""Seeded graphs and inputs for the tests of the message-passing primitives (csrc/gadapt_sparse.inc).

Every builder returns a `Case` that unpacks as `(edge_index, n)` and carries `claims`: what the case is there for, stated by the
builder (row-length histogram of the target CSR, out-degree of the last node, number of duplicate edges and of self-loops, and
where `n * LPN` lies relative to 512).  tests/test_sparse_restatement_host.py recounts every claim from the library's own CSR.

The launch geometry the cases aim at: a row is owned by a group of LPN = `lanes(C)` lanes, a workgroup has 256 threads, so the
last live group of a launch is thread `n * LPN - 1`.  Inputs are drawn in fp32, in the caller's edge order; the fp64 reference
upcasts the same numbers.
"""
import functools

import torch

WIDTHS = (1, 4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260, 516)
EDGE_VEC_WIDTHS = tuple(c for c in WIDTHS if c % 4 == 0)        # the per-edge-vector operations refuse the others
ATTENTION_WIDTHS = (12, 24, 200)
F32, F64 = torch.float32, torch.float64


def chunks(c: int) -> int:
    """float4 chunks of a row of `c` floats after the zero padding to a multiple of 4 (`c4` of the kernels)."""
    return (c + 3) // 4


def lanes(c: int) -> int:
    """Lanes per row at width `c`: `sparse::lanes_for(c4)`, the power of two >= c4, at most 64."""
    l = 1
    while l < chunks(c) and l < 64:
        l <<= 1
    return l


class Case:
    def __init__(self, name, edge_index, n, **claims):
        self.name, self.edge_index, self.n = name, edge_index.to(torch.int64).contiguous(), int(n)
        self.claims = claims

    def __iter__(self):
        return iter((self.edge_index, self.n))

    def __repr__(self):
        return self.name


def _histogram(lengths):
    vals, counts = torch.unique(torch.as_tensor(lengths, dtype=torch.int64), return_counts=True)
    return {int(v): int(c) for v, c in zip(vals, counts)}


def _counted(name, ei, n, **claims):
    """Fill in the claims a builder can only count (it counts from the edge list; the host test recounts from the CSR)."""
    e = ei.shape[1]
    claims.setdefault('row_lengths', _histogram(torch.bincount(ei[1], minlength=n)) if e else {0: n})
    claims.setdefault('last_out_degree', int((ei[0] == n - 1).sum()))
    claims.setdefault('duplicates', e - int(torch.unique(ei[0] * n + ei[1]).numel()))
    claims.setdefault('self_loops', int((ei[0] == ei[1]).sum()))
    return Case(name, ei, n, **claims)


@functools.lru_cache(maxsize=None)
def hub300(seed: int = 3):
    """`_graph(300, 2000, seed)` of tests/test_gpu_variants.py: random edges, a hub with 30 out-edges, one with 40 in-edges, node 5
    without in-edges."""
    n, e = 300, 2000
    g = torch.Generator().manual_seed(seed)
    ei = torch.stack([torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g)])
    ei = torch.cat([ei, torch.tensor([[7] * 30, list(range(30))]), torch.tensor([list(range(40, 80)), [9] * 40])], 1)
    ei = ei[:, ei[1] != 5]
    return _counted('hub300', ei, n, empty_rows=(5,))


@functools.lru_cache(maxsize=None)
def rows0to9(seed: int = 11):
    """n = 67, node i has i % 10 in-edges (every length 0 .. 9, odd and even tails of the two-in-flight loop), sources drawn with
    replacement from all nodes: self-loops and duplicate edges occur.  The edges of a row are NOT contiguous in the caller's order."""
    n = 67
    g = torch.Generator().manual_seed(seed)
    dst = torch.cat([torch.full((i % 10,), i, dtype=torch.int64) for i in range(n)])
    src = torch.randint(0, n, (dst.numel(),), generator=g)
    perm = torch.randperm(dst.numel(), generator=g)
    ei = torch.stack([src, dst])[:, perm]
    case = _counted('rows0to9', ei, n, row_lengths={k: (7 if k < 7 else 6) for k in range(10)})
    assert case.claims['duplicates'] > 0 and case.claims['self_loops'] > 0, case.claims
    return case


@functools.lru_cache(maxsize=None)
def long5(seed: int = 12):
    """n = 5: node 0 has 700 in-edges from nodes 0 .. 4 (duplicates throughout), node 4 one, nodes 1 .. 3 none.  Up to LPN = 8 the
    whole graph is less than one wave: dead lanes and empty rows sit in the wave that walks the 700-slot row."""
    n = 5
    g = torch.Generator().manual_seed(seed)
    src = torch.cat([torch.randint(0, n, (700,), generator=g), torch.tensor([2])])
    dst = torch.cat([torch.zeros(700, dtype=torch.int64), torch.tensor([4])])
    perm = torch.randperm(701, generator=g)
    ei = torch.stack([src, dst])[:, perm]
    case = _counted('long5', ei, n, row_lengths={0: 3, 1: 1, 700: 1}, empty_rows=(1, 2, 3))
    assert case.claims['duplicates'] >= 675 and case.claims['self_loops'] > 0, case.claims
    return case


@functools.lru_cache(maxsize=None)
def block_edge(c: int, d: int, seed: int = 13):
    """n = 512 / LPN(c) + d, d in {-1, 0, +1}: the last live lane group is the last of the second 256-thread workgroup, or the first
    of the third.  Mean in-degree 3; the last node has 17 in-edges and 17 out-edges, so the last row of both orientations is long."""
    l = lanes(c)
    n = 512 // l + d
    g = torch.Generator().manual_seed(seed + 7 * l + d)
    body = n - 1                                                   # nodes 0 .. n - 2 exchange 3 n - 34 random edges among themselves
    m = max(3 * n - 34, 0)
    ei = torch.stack([torch.randint(0, body, (m,), generator=g), torch.randint(0, body, (m,), generator=g)])
    last = torch.full((17,), n - 1, dtype=torch.int64)
    others_in, others_out = torch.randint(0, body, (17,), generator=g), torch.randint(0, body, (17,), generator=g)
    ei = torch.cat([ei, torch.stack([others_in, last]), torch.stack([last, others_out])], 1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    return _counted(f'block_edge({c},{d:+d})', ei, n, last_in_degree=17, last_out_degree=17, threads_past_512=d * l)


@functools.lru_cache(maxsize=None)
def empty130():
    return _counted('empty130', torch.zeros(2, 0, dtype=torch.int64), 130, row_lengths={0: 130}, duplicates=0, self_loops=0)


@functools.lru_cache(maxsize=None)
def one3():
    return _counted('one3', torch.zeros(2, 3, dtype=torch.int64), 1, row_lengths={3: 1}, duplicates=2, self_loops=3, last_out_degree=3)


GRAPHS = ('hub300', 'rows0to9', 'long5', 'block_edge-1', 'block_edge+0', 'block_edge+1', 'empty130', 'one3')


def case(name: str, c: int = 4) -> Case:
    """The case called `name` at width `c` (only `block_edge` depends on the width)."""
    if name.startswith('block_edge'):
        return block_edge(c, int(name[len('block_edge'):]))
    return {'hub300': hub300, 'rows0to9': rows0to9, 'long5': long5, 'empty130': empty130, 'one3': one3}[name]()


@functools.lru_cache(maxsize=None)
def inputs(name: str, c: int):
    """fp32 inputs of one (case, width), seeded by both, per-edge arrays in the CALLER's edge order:
    x, a, b [n, c]; w, scores, vals, g_edge [E]; bvec [E, c]; u, v [n]; g_node [n, c]."""
    ei, n = case(name, c)
    e = ei.shape[1]
    g = torch.Generator().manual_seed(1000 * GRAPHS.index(name) + c)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=F32)      # noqa: E731
    out = {'x': r(n, c), 'a': r(n, c), 'b': r(n, c), 'w': r(e), 'scores': 3 * r(e), 'vals': r(e), 'g_edge': r(e),
           'bvec': r(e, c), 'u': r(n), 'v': r(n), 'g_node': r(n, c)}
    return out
