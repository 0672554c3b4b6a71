"""Device-resident CSR of a batched mesh graph + the reference's edge surgery.

`prepare_edge_index` is the prologue of `GNN.forward` (`src/GNN.py:206-223`):
boundary masks, corner / end-point self-loops, optional `self_loops`.  It is a
pure function of the batch *topology*, which is identical for every batch of a
fixed-size dataset (all samples share one mesh, `src/data.py:290`), so
`GraphCache` runs it - and the CSR build behind it - once per topology instead
of once per forward.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _native
from ._native import GadaptGraph


def prepare_edge_index(data, dim: int, mesh_n: int, fix_boundary: bool, self_loops: bool,
                       num_nodes: int, corner_nodes=None) -> torch.Tensor:
    """CPU int64 [2,E] edge list the conv layers see (`src/GNN.py:206-223`).  `corner_nodes` overrides
    `data.corner_nodes` (a single un-collated sample carries one array instead of a list of arrays)."""
    edge_index = data.edge_index.detach().cpu()
    if fix_boundary:
        keep = ~(data.to_boundary_edge_mask.cpu() | data.to_corner_nodes_mask.cpu()
                 | data.diff_boundary_edges_mask.cpu())
        edge_index = edge_index[:, keep]
        num_in_batch = int(data.batch.max().item()) + 1
        if dim == 1:
            b = torch.arange(num_in_batch, dtype=torch.int64)
            ends = torch.stack([b * mesh_n, (b + 1) * mesh_n - 1], dim=1).reshape(-1)     # GNN.py:210
            loops = ends.repeat(2, 1)
        else:
            corners = data.corner_nodes if corner_nodes is None else corner_nodes
            corner = torch.stack([torch.as_tensor(np.asarray(a), dtype=torch.int64) for a in corners])
            counts = torch.bincount(data.batch.cpu(), minlength=num_in_batch)
            offsets = torch.cumsum(counts, 0) - counts                                     # GNN.py:214-216
            loops = (corner + offsets.unsqueeze(-1)).reshape(-1).repeat(2, 1)
        edge_index = torch.cat([edge_index, loops], dim=1)
    if self_loops:                                                                         # GNN.py:220-223
        edge_index = edge_index[:, edge_index[0] != edge_index[1]]
        ar = torch.arange(num_nodes, dtype=torch.int64)
        edge_index = torch.cat([edge_index, ar.repeat(2, 1)], dim=1)
    return edge_index.contiguous()


# ---------------------------------------------------------------------------------------------------------------
# Content fingerprint of index / mask tensors: what a graph cache may key on.  The reference rebuilds `edge_index` from
# `data` on every forward (`src/GNN.py:206-218`), so a cache must notice ANY change of the edge list or of the masks -
# equal sizes are not enough (two triangulations of one point set have equal node and edge counts).
# ---------------------------------------------------------------------------------------------------------------
_fp_memo: Dict[int, Tuple] = {}
_fp_weights: Dict[Tuple, torch.Tensor] = {}


def _fp_weight(n: int, device) -> torch.Tensor:
    key = (str(device), n)
    w = _fp_weights.get(key)
    if w is None:
        if len(_fp_weights) > 16:
            _fp_weights.clear()
        w = _fp_weights[key] = torch.arange(1, n + 1, device=device, dtype=torch.int64)
    return w


# splitmix64 constants as signed int64 (torch integer arithmetic wraps around)
_FP_GOLD, _FP_M1, _FP_M2 = -7046029254386353131, -4658895280553007687, -7723592293110705685


def _fp_mix(v: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Position-dependent NON-LINEAR mix of every element (splitmix64 finaliser of v_i + (i+1) * golden ratio).  A linear
    checksum pair (sum of v_i * (i+1), sum of v_i) collides on structured edits - e.g. flipping the diagonal of one grid quad,
    (a, a+n+1) -> (a+1, a+n) in place in both directions, keeps both sums - and would hand back a stale CSR."""
    z = w * _FP_GOLD                      # the one [n] temporary of the chain; every later step works in place on it and on `t`
    z.add_(v)
    t = z >> 30
    z.bitwise_xor_(t).mul_(_FP_M1)
    torch.bitwise_right_shift(z, 27, out=t)
    z.bitwise_xor_(t).mul_(_FP_M2)
    torch.bitwise_right_shift(z, 31, out=t)
    return z.bitwise_xor_(t)


FP_STATS = {'hashed': 0}            # tensors hashed so far (memo misses): a loop that re-hashes every step is paying a host synchronisation


def content_fingerprint(tensors) -> Tuple:
    """Order-sensitive checksums (int64 wrap-around arithmetic) of integer / bool tensors, on the device they live on: the sum
    of a per-element, position-dependent 64-bit hash (`_fp_mix`) and the plain sum.

    Memoised per tensor OBJECT (weak reference + version counter + data pointer): a batch object fed again - every step
    of a hipGraph-free training loop over `DeviceMeshLoader`, every call of a rollout - costs a dictionary lookup; a new
    tensor (even at a recycled address) is hashed again.  One host synchronisation per set of new tensors."""
    out, todo = [None] * len(tensors), []
    for k, t in enumerate(tensors):
        m = _fp_memo.get(id(t))
        if m is not None and m[0]() is t and m[1] == t._version and m[2] == t.data_ptr() and m[3] == tuple(t.shape):
            out[k] = m[4]
        else:
            todo.append(k)
    if todo:
        FP_STATS['hashed'] += len(todo)
        sums = []
        for k in todo:
            v = tensors[k].detach().reshape(-1).to(torch.int64)
            n = int(v.numel())
            if n == 0:
                sums.append(torch.zeros(2, dtype=torch.int64, device=v.device))
                continue
            sums.append(torch.stack([_fp_mix(v, _fp_weight(n, v.device)).sum(), v.sum()]))
        by_dev = {}
        for k, s_ in zip(todo, sums):
            by_dev.setdefault(str(s_.device), []).append((k, s_))
        for items in by_dev.values():                                   # one D2H copy per device
            vals = torch.stack([s_ for _, s_ in items]).tolist()
            for (k, _), v in zip(items, vals):
                t = tensors[k]
                fp = (tuple(t.shape), str(t.dtype), int(v[0]), int(v[1]))
                out[k] = fp
                if len(_fp_memo) > 256:
                    for dead in [i for i, m in _fp_memo.items() if m[0]() is None]:
                        _fp_memo.pop(dead, None)
                    if len(_fp_memo) > 256:
                        _fp_memo.clear()
                try:
                    _fp_memo[id(t)] = (weakref.ref(t), t._version, t.data_ptr(), tuple(t.shape), fp)
                except TypeError:
                    pass
    return tuple(out)


# The wide (hidden 64) kernels run on graphs that qualify (gadapt_ell_build_host); False keeps the tiled kernels
# everywhere (tests compare the two).  Read when a MeshGraph is built; part of the cache key.
WIDE_KERNELS = True
# ... and only from this many nodes on: a wide workgroup loads a 384-row window before it computes anything, which a
# batch too small to fill the 256 CUs does not earn back (forward of 64x64 meshes, hidden 64, 4 layers as one hipGraph:
# batch 1 / 4 / 8 / 16 = 78.6 / 80.7 / 85.7 / 93.2 us wide against 74.5 / 74.1 / 87.1 / 110.1 us tiled).
WIDE_MIN_NODES = 24576
# ... and up to this many on four-wave workgroups, steps of 128 nodes (csrc/gadapt_wide.inc, NWV = 4): the launcher takes them when the
# 256-node steps would fill at most half of the CUs
WIDE_HALF_MAX_NODES = 32768


class MeshGraph:
    """Both CSR orientations of one edge list, int32, resident on `device`."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int, device):
        ei = edge_index.detach().to('cpu', torch.int64).contiguous()
        n, e = int(num_nodes), int(ei.shape[1])
        self.num_nodes, self.num_edges = n, e
        self.device = torch.device(device)
        rowptr_t = torch.empty(n + 1, dtype=torch.int32)
        rowptr_s = torch.empty(n + 1, dtype=torch.int32)
        col_t, eid_t, col_s, perm_s, tpos_s = (torch.empty(max(e, 1), dtype=torch.int32) for _ in range(5))
        src, dst = ei[0].contiguous(), ei[1].contiguous()
        if e == 0:                                          # an empty tensor has no address; the build reads no entry of either
            src = dst = torch.zeros(1, dtype=torch.int64)
        rc = _native.lib().gadapt_csr_build_host(src.data_ptr(), dst.data_ptr(), e, n,
                                                 rowptr_t.data_ptr(), col_t.data_ptr(), eid_t.data_ptr(),
                                                 rowptr_s.data_ptr(), col_s.data_ptr(), perm_s.data_ptr(), tpos_s.data_ptr())
        if rc != 0:
            raise _native.NativeError(f"gadapt_csr_build_host failed (code {rc}): edge endpoint outside [0,{n})?")
        metas = {}
        for tag, rp, cl in (('t', rowptr_t, col_t), ('s', rowptr_s, col_s)):
            for tm in _native.TILE_HEIGHTS:
                m = torch.empty(4 * ((n + tm - 1) // tm), dtype=torch.int32)
                if _native.lib().gadapt_tile_meta_host(rp.data_ptr(), cl.data_ptr(), n, tm, m.data_ptr()) != 0:
                    raise _native.NativeError("gadapt_tile_meta_host failed")
                metas[(tag, tm)] = m
        metas = {k: v.to(self.device) for k, v in metas.items()}
        self._metas = metas
        # ELL-8 copies + eligibility for the wide (hidden 64) kernels
        n_pad = (n + 255) // 256 * 256
        ells, wide_deg = {}, {}
        for tag, rp, cl in (('t', rowptr_t, col_t), ('s', rowptr_s, col_s)):
            ell = torch.empty(n_pad * 8, dtype=torch.int32)
            md = C.c_int32(0)
            if _native.lib().gadapt_ell_build_host(rp.data_ptr(), cl.data_ptr(), n, ell.data_ptr(), C.addressof(md)) != 0:
                raise _native.NativeError("gadapt_ell_build_host failed")
            ells[tag], wide_deg[tag] = ell.to(self.device), (int(md.value) if (WIDE_KERNELS and n >= WIDE_MIN_NODES) else 0)
        self._ells, self.wide_deg = ells, wide_deg
        # 512-row window of the wide forward: row-major meshes with up to 128 nodes per mesh row that miss the 384-row one
        self.wide_big_deg = 0
        if WIDE_KERNELS and n >= WIDE_MIN_NODES and wide_deg['t'] == 0:
            md = C.c_int32(0)
            if _native.lib().gadapt_wide_window_host(rowptr_t.data_ptr(), col_t.data_ptr(), n, 256, 128, 7, C.addressof(md)) != 0:
                raise _native.NativeError("gadapt_wide_window_host failed")
            self.wide_big_deg = int(md.value)
        # steps of 128 nodes on four-wave workgroups (batches that would leave half of the CUs without a 256-node step)
        self.wide_half_deg = 0
        if wide_deg['t'] > 0 and n <= WIDE_HALF_MAX_NODES:
            md = C.c_int32(0)
            if _native.lib().gadapt_wide_window_host(rowptr_t.data_ptr(), col_t.data_ptr(), n, 128, 64, 8, C.addressof(md)) != 0:
                raise _native.NativeError("gadapt_wide_window_host failed")
            self.wide_half_deg = int(md.value)
        self._cpu_csr_t = (rowptr_t, col_t)                 # host copies for mesh_partition()
        self._partitions: Dict[Tuple, Optional[Tuple]] = {}
        self.edge_index = edge_index                        # as given (original order/device)
        self.rowptr_t, self.col_t, self.eid_t = (t.to(self.device) for t in (rowptr_t, col_t, eid_t))
        self.rowptr_s, self.col_s, self.perm_s, self.tpos_s = (t.to(self.device) for t in (rowptr_s, col_s, perm_s, tpos_s))
        self.max_in_degree = int((rowptr_t[1:] - rowptr_t[:-1]).max())
        self.c_struct = GadaptGraph(n, e, self.rowptr_t.data_ptr(), self.col_t.data_ptr(),
                                    self.rowptr_s.data_ptr(), self.col_s.data_ptr(), self.perm_s.data_ptr(),
                                    self.tpos_s.data_ptr(),
                                    (C.c_void_p * 3)(*[metas[('t', tm)].data_ptr() for tm in _native.TILE_HEIGHTS]),
                                    (C.c_void_p * 3)(*[metas[('s', tm)].data_ptr() for tm in _native.TILE_HEIGHTS]),
                                    ells['t'].data_ptr(), ells['s'].data_ptr(), wide_deg['t'], wide_deg['s'], self.wide_big_deg, self.wide_half_deg)
        self.c_ref = C.byref(self.c_struct)
        # one launch for up to four forward layers of the narrow route (csrc/gadapt_block_plan.h): the halo is found on the host copy of
        # the CSR and registered with the library, which sees device arrays only
        self.narrow_block_halo = 0
        if wide_deg['t'] > 0 or self.wide_big_deg > 0:
            hl = C.c_int32(0)
            if _native.lib().gadapt_narrow_block_halo_host(rowptr_t.data_ptr(), col_t.data_ptr(), n, C.addressof(hl)) != 0:
                raise _native.NativeError("gadapt_narrow_block_halo_host failed")
            self.narrow_block_halo = int(hl.value)
        _native.check(_native.lib().gadapt_narrow_block_register(self.c_ref, self.narrow_block_halo), "gadapt_narrow_block_register")
        # ... and one launch for the backward layers below the top (csrc/gadapt_narrow_bwd_block.inc): the same test on the out-edges
        self.narrow_block_halo_source = 0
        if self.narrow_block_halo and e > 0:
            hl = C.c_int32(0)
            if _native.lib().gadapt_narrow_block_halo_host(rowptr_s.data_ptr(), col_s.data_ptr(), n, C.addressof(hl)) != 0:
                raise _native.NativeError("gadapt_narrow_block_halo_host failed")
            self.narrow_block_halo_source = int(hl.value)
        _native.check(_native.lib().gadapt_narrow_block_register_source(self.c_ref, self.narrow_block_halo_source),
                      "gadapt_narrow_block_register_source")

    def __del__(self):
        try:                                                # the device arrays go back to the allocator: forget their registration
            if getattr(self, 'narrow_block_halo', 0):
                _native.lib().gadapt_narrow_block_register(self.c_ref, 0)
            if getattr(self, 'narrow_block_halo_source', 0):
                _native.lib().gadapt_narrow_block_register_source(self.c_ref, 0)
        except Exception:
            pass

    def narrow_route(self, c: int) -> bool:
        """Whether the block runs on the four live columns at hidden size `c` on this graph (`gadapt_narrow_route`: hidden 64 where the
        wide forward takes the graph)."""
        return bool(_native.lib().gadapt_narrow_route(self.c_ref, int(c)))

    def mesh_partition(self, batch: Optional[torch.Tensor]):
        """(mesh_ptr int32 [2, B+1] on the device - row 0 the first node, row 1 the first in-edge of each mesh -, n_meshes, max nodes
        per mesh, max in-edges per mesh) when the meshes of the batch are
        contiguous node ranges that no edge leaves - what PyG collation produces (`batch` non-decreasing, edge_index offset per
        graph) - else None.  `batch=None`: the whole graph is one mesh.  Checked once per `batch` content (one host
        synchronisation), then a dictionary lookup: the one-launch small-mesh forward (csrc/gadapt_smallmesh.inc) needs it."""
        key = () if batch is None else content_fingerprint([batch])
        if key in self._partitions:
            return self._partitions[key]
        n = self.num_nodes
        rowptr, col = self._cpu_csr_t
        part = None
        if batch is None:
            ptr_ = torch.tensor([0, n], dtype=torch.int64)
            ok = True
        else:
            b = batch.detach().to('cpu', torch.int64).reshape(-1)
            ok = b.numel() == n and n > 0 and bool((b[1:] >= b[:-1]).all()) and int(b[0]) == 0
            if ok:
                counts = torch.bincount(b)
                ok = bool((counts > 0).all())
                ptr_ = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])
                if ok and self.num_edges:
                    deg = (rowptr[1:] - rowptr[:-1]).to(torch.int64)
                    dst = torch.repeat_interleave(torch.arange(n, dtype=torch.int64), deg)
                    ok = bool((b[col[:self.num_edges].to(torch.int64)] == b[dst]).all())
        if ok:
            rp = rowptr.to(torch.int64)
            e_per = rp[ptr_[1:]] - rp[ptr_[:-1]]
            part = (torch.stack([ptr_, rp[ptr_]]).to(torch.int32).contiguous().to(self.device), int(ptr_.numel() - 1), int((ptr_[1:] - ptr_[:-1]).max()), int(e_per.max()))
        if len(self._partitions) > 8:
            self._partitions.clear()
        self._partitions[key] = part
        return part

    @property
    def has_in(self) -> torch.Tensor:
        """[N,1] float mask: 1 where a node has at least one in-edge (kept on the graph it belongs to)."""
        m = getattr(self, '_has_in', None)
        if m is None:
            m = self._has_in = (self.rowptr_t[1:] > self.rowptr_t[:-1]).to(torch.float32).unsqueeze(-1)
        return m

    def with_self_loops(self) -> 'MeshGraph':
        """The graph PyG's `remove_self_loops` + `add_self_loops` (GATConv's default) / `add_remaining_self_loops` (gcn_norm,
        unweighted) make of this one: the non-loop edges in their order, then one loop per node 0..N-1.  Built once."""
        g = getattr(self, '_looped', None)
        if g is None:
            ei = self.edge_index.detach().to('cpu', torch.int64)
            ei = ei[:, ei[0] != ei[1]]
            ar = torch.arange(self.num_nodes, dtype=torch.int64)
            ei = torch.cat([ei, ar.unsqueeze(0).repeat(2, 1)], dim=1).contiguous()
            g = self._looped = MeshGraph(ei.to(self.edge_index.device), self.num_nodes, self.device)
        return g

    def alpha_to_edge_order(self, alpha_t: torch.Tensor) -> torch.Tensor:
        """[.., E] attention in target-CSR order -> the caller's edge order."""
        out = torch.empty_like(alpha_t)
        out[..., self.eid_t.long()] = alpha_t
        return out


class GraphCache:
    """edge list -> MeshGraph, keyed by content (shape + hash of the int64 bytes)."""

    def __init__(self, capacity: int = 16):
        self.capacity = capacity
        self._store: Dict[Tuple, MeshGraph] = {}

    @staticmethod
    def _key(edge_index: torch.Tensor, num_nodes: int, device) -> Tuple:
        return (int(num_nodes), str(device), content_fingerprint([edge_index]), WIDE_KERNELS, WIDE_MIN_NODES, WIDE_HALF_MAX_NODES)

    def get(self, edge_index: torch.Tensor, num_nodes: int, device) -> MeshGraph:
        key = self._key(edge_index, num_nodes, device)
        g = self._store.get(key)
        if g is None:
            if len(self._store) >= self.capacity:
                self._store.pop(next(iter(self._store)))
            g = MeshGraph(edge_index, num_nodes, device)
            self._store[key] = g
        return g


_default_cache = GraphCache()


def graph_for(edge_index: torch.Tensor, num_nodes: int, device) -> MeshGraph:
    return _default_cache.get(edge_index, num_nodes, device)
