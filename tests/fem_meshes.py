"""Meshes for the 2-D FEM tests in node and triangle orders other than square_mesh's row-major one: renumbered nodes (a wide
band on a small mesh), the same triangles in another row order, and the union-jack triangulation (valences 4 and 8).

The FEM tail takes any triangulation (gadapt_fem_topology_host computes the interior numbering and the half-bandwidth w
from the cells it is given); these helpers reach its wide-band and tight-ring code at sizes whose fp64 restatement runs in
seconds.  The seeds below are the first hits of a search from seed 0 (`first_seed`) with numpy's default_rng; the host
tests recompute each band."""
from __future__ import annotations

import numpy as np
import torch

from g_adaptivity_amd.fem import boundary_from_cells
from g_adaptivity_amd.mesh_graph import square_mesh

# permuted(square_mesh(11), ..., seed): 81 interior nodes, half-bandwidth 77 / 78 / 79 / 80 (80 = n_int - 1, a full matrix)
SEED_N11_W77 = 1
SEED_N11_W78 = 0
SEED_N11_W79 = 3
SEED_N11_W80 = 14
# permuted(square_mesh(12), ..., seed): 100 interior nodes, the first seed with w >= 90 and the band it gives
SEED_N12_WIDE = 0
W_N12_WIDE = 91
N11_SEEDS = {77: SEED_N11_W77, 78: SEED_N11_W78, 79: SEED_N11_W79, 80: SEED_N11_W80}


def band_of(cells, boundary) -> int:
    """Half-bandwidth of the interior block in the interior numbering (interior nodes in increasing node id)."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    bnd = np.asarray(boundary, dtype=bool).reshape(-1)
    idx = np.where(bnd, -1, np.cumsum(~bnd) - 1)
    ii = idx[cells]
    band = 0
    for i in range(3):
        for j in range(i + 1, 3):
            ok = (ii[:, i] >= 0) & (ii[:, j] >= 0)
            if ok.any():
                band = max(band, int(np.abs(ii[ok, i] - ii[ok, j]).max()))
    return band


def permuted(mesh_or_cells, x, boundary=None, seed=0, perm=None):
    """The mesh with its nodes renumbered by perm = default_rng(seed).permutation(N) (or the given perm): old node i
    becomes perm[i].  Returns (x', cells', boundary', perm) with x'[perm[i]] = x[i]; the triangles keep their row order and
    local order."""
    cells = getattr(mesh_or_cells, 'cells', mesh_or_cells)
    if boundary is None:
        boundary = mesh_or_cells.boundary_nodes
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    bnd = np.asarray(boundary, dtype=bool).reshape(-1)
    perm = np.random.default_rng(seed).permutation(bnd.shape[0]) if perm is None else np.asarray(perm, dtype=np.int64)
    x2 = torch.empty_like(x)
    x2[torch.from_numpy(perm)] = x
    b2 = np.empty_like(bnd)
    b2[perm] = bnd
    return x2, torch.from_numpy(perm[cells]), torch.from_numpy(b2), perm


def far_swap(n, w):
    """The renumbering of square_mesh(n) that swaps two interior nodes, the first one and the one w - (n - 2) places after it
    in the interior numbering: the second one's neighbour a grid row on (n - 2 places after it) is then w places from it, and
    nothing is farther.  The band is w with the n_int = (n - 2)^2 unknowns of the mesh, so at n = 12 and w = 77 ... 79 the
    windowed solve has more rows (100) than its ring (R = w + S = 84, 82, 81) and the ring wraps, which the 81 unknowns of
    the 11 x 11 cases never make it do."""
    k = n - 2
    i = w - k
    assert k + 1 < i and i + k < k * k
    a, b = n + 1, (i // k + 1) * n + i % k + 1
    perm = np.arange(n * n)
    perm[a], perm[b] = b, a
    return perm


def shuffled_triangles(cells, seed):
    """The same triangles (each with its local vertex order) in another row order."""
    cells = torch.as_tensor(cells)
    order = np.random.default_rng(seed).permutation(cells.shape[0])
    return cells[torch.from_numpy(order)]


def union_jack(n):
    """(x [n*n,2] fp32, cells [2(n-1)^2,3] int64, boundary [n*n] bool): square_mesh(n)'s nodes with alternating diagonals.
    Quad (ix, iy) with ix + iy even is cut from (ix, iy) to (ix+1, iy+1), the others as square_mesh cuts them, so interior
    nodes with ix + iy even have 8 triangles and the others 4.  Vertices are listed clockwise, as square_mesh's."""
    assert n >= 3
    tris = []
    for ix in range(n - 1):
        for iy in range(n - 1):
            v0, v1, v2, v3 = ix * n + iy, ix * n + iy + 1, (ix + 1) * n + iy + 1, (ix + 1) * n + iy
            tris += [(v0, v1, v2), (v0, v2, v3)] if (ix + iy) % 2 == 0 else [(v0, v1, v3), (v1, v2, v3)]
    cells = np.asarray(tris, dtype=np.int64)
    return square_mesh(n).x_comp.clone(), torch.from_numpy(cells), torch.from_numpy(boundary_from_cells(cells, n * n))


def first_seed(n, accept, limit=1000):
    """The first seed from 0 whose permuted(square_mesh(n)) has a band that `accept` takes: how the constants were found."""
    m = square_mesh(n)
    for seed in range(limit):
        _, cells, bnd, _ = permuted(m, m.x_comp, seed=seed)
        if accept(band_of(cells, bnd)):
            return seed
    raise LookupError(f"no seed below {limit}")
