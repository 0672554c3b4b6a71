"""The message-passing primitives of csrc/gadapt_sparse.inc restated as plain gather / scatter in torch, for any dtype (fp64 is the
reference), with the quantity each elementwise error bound scales with next to every operation.

Everything works in the CALLER's edge order: edge e runs from `ei[0, e]` (source j) to `ei[1, e]` (target i).  The library keeps
per-edge arrays in target-CSR order; `csr_orders` restates that order (a stable sort by target, and for the source CSR a stable
sort of the target slots by source), `graph_orders` takes it from `MeshGraph(ei, n, 'cpu')` - the CSR build is host code.

BARS (u = 2^-24, gamma_k = k u / (1 - k u); derived, none fitted to a kernel; tests/test_sparse_restatement_host.py shows on the
CPU that an fp32 evaluation slot by slot in CSR order meets each of them on every case and that each planted fault leaves them):
  spmm, either orientation     gamma_(L+2) (sum_row |w_e| |x_j| + |self_scale| |x_i|): a product and at most L additions per term
  edge_weighted_rowsum         gamma_(L+1) sum_row |w_e| |B_e|
  edge_rowsum                  gamma_L sum_row |v_e|: exact for L <= 1
  sddmm, edge_node_dot         gamma_(C4+2) |scale| sum_c |a| |b|, C4 the padded width: any summation order, with or without FMA
  edge_add, edge_mul, mode 2   bit-equal to the fp32 torch expression (one correctly rounded operation each)
  empty row                    exactly 0, or exactly fl(self_scale x_i)
  edge_softmax backward        gamma_(L+3) |alpha_e| (|dalpha_e| + sum_row |alpha dalpha|), from the fp32 alpha the forward returned
  edge_softmax forward         expf cannot be derived: per row, noise = max over the row of max(|a32 - a64|, |a32' - a32|), a32 the fp32
                               restatement and a32' the same with every exponential multiplied by a seeded 1 +- 2^-23; the bar is
                               max_row |got - a64| <= max(4 noise, (L + 4) u)  (the rule and the 4 of tests/ma_restatement.py,
                               tests/test_gpu_ma.py; the floor is for rows whose noise is exactly zero)
L is the row length in the orientation walked (in-degree, or out-degree for the transposed products).
"""
import torch

from oracle.pyg_restatement import pyg_softmax

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24


def gamma(k):
    """gamma_k = k u / (1 - k u) for a number or a tensor of counts (fp64)."""
    k = torch.as_tensor(k, dtype=F64)
    return k * U / (1.0 - k * U)


# --------------------------------------------------------------------------------------------------------------- orders
def csr_orders(ei, n):
    """(eid_t, perm_s, rowptr_t, rowptr_s) restated: `eid_t[slot]` = caller's edge id of target-CSR slot `slot` (stable sort by
    target); `perm_s[slot_s]` = target-CSR slot of source-CSR slot `slot_s` (stable sort of the target slots by source)."""
    src, dst = ei[0], ei[1]
    eid_t = torch.sort(dst, stable=True).indices
    perm_s = torch.sort(src[eid_t], stable=True).indices
    rowptr = lambda idx: torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(idx, minlength=n), 0)])   # noqa: E731
    return eid_t, perm_s, rowptr(dst), rowptr(src)


def graph_orders(ei, n):
    """The same four arrays from the library (`MeshGraph(ei, n, 'cpu')`), int64, cut to E entries."""
    from g_adaptivity_amd import MeshGraph
    g = MeshGraph(ei, n, 'cpu')
    e = ei.shape[1]
    return g.eid_t[:e].long(), g.perm_s[:e].long(), g.rowptr_t.long(), g.rowptr_s.long()


def _scatter(index, vals, n):
    return torch.zeros((n,) + tuple(vals.shape[1:]), dtype=vals.dtype).index_add_(0, index, vals)


# ----------------------------------------------------------------------------------------------------------------- spmm
def spmm(ei, n, w, x, transpose=False, self_scale=0.0, dtype=F64):
    """out_i = sum_{e: j -> i} w_e x_j + self_scale x_i; transposed: out_j = sum_{e: j -> i} w_e x_i + self_scale x_j.  w None: 1."""
    gather, scatter = (ei[1], ei[0]) if transpose else (ei[0], ei[1])
    x = x.to(dtype)
    msg = x.index_select(0, gather)
    if w is not None:
        msg = w.to(dtype).unsqueeze(-1) * msg
    out = _scatter(scatter, msg, n)
    return out + self_scale * x if self_scale != 0.0 else out


def spmm_bound(ei, n, w, x, transpose=False, self_scale=0.0):
    """(S [n, C], L [n]): |got - ref| <= gamma_(L+2) S."""
    gather, scatter = (ei[1], ei[0]) if transpose else (ei[0], ei[1])
    ax = x.to(F64).abs()
    msg = ax.index_select(0, gather)
    if w is not None:
        msg = w.to(F64).abs().unsqueeze(-1) * msg
    return _scatter(scatter, msg, n) + abs(self_scale) * ax, torch.bincount(scatter, minlength=n)


# ---------------------------------------------------------------------------------------------------------------- sddmm
def sddmm(ei, a, b, scale=1.0, dtype=F64):
    """s_e = scale <a_i, b_j> for e: j -> i."""
    return scale * (a.to(dtype).index_select(0, ei[1]) * b.to(dtype).index_select(0, ei[0])).sum(-1)


def sddmm_bound(ei, a, b, scale=1.0):
    """(S [E], C4): |got - ref| <= gamma_(C4+2) S."""
    c = a.shape[1]
    return abs(scale) * (a.to(F64).abs().index_select(0, ei[1]) * b.to(F64).abs().index_select(0, ei[0])).sum(-1), (c + 3) // 4 * 4


# --------------------------------------------------------------------------------------------------------- edge softmax
def edge_softmax(ei, n, scores, dtype=F64):
    """PyG `utils.softmax` grouped by target, the 1e-16 kept (oracle.pyg_restatement.pyg_softmax)."""
    return pyg_softmax(scores.to(dtype).unsqueeze(-1), ei[1], n).squeeze(-1)


def edge_softmax_perturbed(ei, n, scores, seed=None, dtype=F32):
    """`pyg_softmax` spelled out (same operations: bit-equal to it without a seed), every exponential multiplied by 1 + 2^-23 or
    1 - 2^-23 drawn from `seed`: the price of an expf that rounds differently from the host's."""
    s, dst = scores.to(dtype), ei[1]
    mx = torch.full((n,), float('-inf'), dtype=dtype).scatter_reduce(0, dst, s, reduce='amax', include_self=True)
    ex = (s - mx.index_select(0, dst)).exp()
    if seed is not None:
        sign = torch.randint(0, 2, ex.shape, generator=torch.Generator().manual_seed(seed)).to(dtype) * 2 - 1
        ex = ex * (1 + sign * 2.0 ** -23)
    den = _scatter(dst, ex, n) + 1e-16
    return ex / den.index_select(0, dst)


def edge_softmax_noise(ei, n, scores, seed=1):
    """[n] noise_row = max over the row of max(|a32 - a64|, |a32' - a32|); 0 for an empty row."""
    a64 = edge_softmax(ei, n, scores, F64)
    a32 = edge_softmax(ei, n, scores, F32).double()
    a32p = edge_softmax_perturbed(ei, n, scores, seed, F32).double()
    return row_max(ei, n, torch.maximum((a32 - a64).abs(), (a32p - a32).abs()))


def edge_softmax_bar(ei, n, scores, seed=1):
    """(a64 [E], bar [E]): per edge, the bar of its row: max(4 noise_row, (L + 4) u)."""
    length = torch.bincount(ei[1], minlength=n).double()
    bar = torch.maximum(4 * edge_softmax_noise(ei, n, scores, seed), (length + 4) * U)
    return edge_softmax(ei, n, scores, F64), bar.index_select(0, ei[1])


def row_max(ei, n, per_edge):
    """[n] max over each target's in-edges of a non-negative per-edge quantity (0 for an empty row)."""
    return torch.zeros(n, dtype=per_edge.dtype).scatter_reduce(0, ei[1], per_edge, reduce='amax', include_self=True)


def edge_softmax_backward(ei, n, alpha, dalpha, dtype=F64):
    """ds_e = alpha_e (dalpha_e - sum_row alpha dalpha), on the alpha given."""
    al, da = alpha.to(dtype), dalpha.to(dtype)
    d = _scatter(ei[1], al * da, n)
    return al * (da - d.index_select(0, ei[1]))


def edge_softmax_backward_bound(ei, n, alpha, dalpha):
    """(S [E], L [E]): |got - ref| <= gamma_(L+3) S."""
    al, da = alpha.to(F64).abs(), dalpha.to(F64).abs()
    d = _scatter(ei[1], al * da, n)
    return al * (da + d.index_select(0, ei[1])), torch.bincount(ei[1], minlength=n).index_select(0, ei[1])


# --------------------------------------------------------------------------------------------------------- edge combine
def edge_add(ei, u, v, dtype=F64):
    """o_e = u_j + v_i."""
    return u.to(dtype).index_select(0, ei[0]) + v.to(dtype).index_select(0, ei[1])


def edge_mul(ei, u, v, dtype=F64):
    """o_e = u_j v_i."""
    return u.to(dtype).index_select(0, ei[0]) * v.to(dtype).index_select(0, ei[1])


def edge_rowsum(ei, n, vals, by_source=False, dtype=F64):
    """r_i = sum of vals over the in-edges of i (by target) or over its out-edges (by source)."""
    return _scatter(ei[0] if by_source else ei[1], vals.to(dtype), n)


def edge_rowsum_bound(ei, n, vals, by_source=False):
    """(S [n], L [n]): |got - ref| <= gamma_L S; exact for L <= 1."""
    idx = ei[0] if by_source else ei[1]
    return _scatter(idx, vals.to(F64).abs(), n), torch.bincount(idx, minlength=n)


# -------------------------------------------------------------------------------------------------- per-edge vectors
def edge_node_dot(ei, a, bvec, dtype=F64):
    """mode 0: s_e = <a_i, B_e>, i the target of e."""
    return (a.to(dtype).index_select(0, ei[1]) * bvec.to(dtype)).sum(-1)


def edge_node_dot_bound(ei, a, bvec):
    """(S [E], C4): |got - ref| <= gamma_(C4+2) S."""
    c = a.shape[1]
    return (a.to(F64).abs().index_select(0, ei[1]) * bvec.to(F64).abs()).sum(-1), (c + 3) // 4 * 4


def edge_weighted_rowsum(ei, n, w, bvec, dtype=F64):
    """mode 1: out_i = sum over the in-edges of i of w_e B_e."""
    return _scatter(ei[1], w.to(dtype).unsqueeze(-1) * bvec.to(dtype), n)


def edge_weighted_rowsum_bound(ei, n, w, bvec):
    """(S [n, C], L [n]): |got - ref| <= gamma_(L+1) S."""
    return _scatter(ei[1], w.to(F64).abs().unsqueeze(-1) * bvec.to(F64).abs(), n), torch.bincount(ei[1], minlength=n)


def edge_scale_gather(ei, w, a, dtype=F64):
    """mode 2: out_e = w_e a_i, i the target of e."""
    return w.to(dtype).unsqueeze(-1) * a.to(dtype).index_select(0, ei[1])


# ------------------------------------------------------------------------------------------------------------- measures
def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements; where the bound is 0 the result must be equal (inf otherwise).  0 for no elements."""
    err = (got.detach().to('cpu', F64) - ref.detach().to(F64)).abs()
    bound = torch.as_tensor(bound, dtype=F64).expand_as(err)
    if err.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(err).all()):
        return float('inf')
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return float(ratio.max())


def spmm_ratio(got, ei, n, w, x, transpose=False, self_scale=0.0):
    s, length = spmm_bound(ei, n, w, x, transpose, self_scale)
    return worst_ratio(got, spmm(ei, n, w, x, transpose, self_scale), gamma(length + 2).unsqueeze(-1) * s)


def empty_rows_exact(got, ei, n, x=None, transpose=False, self_scale=0.0):
    """Rows without a slot in the orientation walked hold exactly 0, or exactly fl(self_scale x_i) (fp32 `got` only)."""
    empty = torch.bincount(ei[0] if transpose else ei[1], minlength=n) == 0
    got = got.detach().cpu()
    want = torch.zeros_like(got[empty]) if self_scale == 0.0 else (torch.tensor(self_scale, dtype=F32) * x.to(F32))[empty]
    return torch.equal(got[empty], want)


def sddmm_ratio(got, ei, a, b, scale=1.0):
    s, c4 = sddmm_bound(ei, a, b, scale)
    return worst_ratio(got, sddmm(ei, a, b, scale), gamma(c4 + 2) * s)


def edge_softmax_ratio(got, ei, n, scores):
    """Worst over the rows of max_row |got - a64| / bar_row."""
    a64, bar = edge_softmax_bar(ei, n, scores)
    return worst_ratio(got, a64, bar)


def edge_softmax_backward_ratio(got, ei, n, alpha, dalpha):
    s, length = edge_softmax_backward_bound(ei, n, alpha, dalpha)
    return worst_ratio(got, edge_softmax_backward(ei, n, alpha, dalpha), gamma(length + 3) * s)


def edge_rowsum_ratio(got, ei, n, vals, by_source=False):
    s, length = edge_rowsum_bound(ei, n, vals, by_source)
    bound = torch.where(length <= 1, torch.zeros_like(s), gamma(length) * s)          # exact for L <= 1
    return worst_ratio(got, edge_rowsum(ei, n, vals, by_source), bound)


def edge_node_dot_ratio(got, ei, a, bvec):
    s, c4 = edge_node_dot_bound(ei, a, bvec)
    return worst_ratio(got, edge_node_dot(ei, a, bvec), gamma(c4 + 2) * s)


def edge_weighted_rowsum_ratio(got, ei, n, w, bvec):
    s, length = edge_weighted_rowsum_bound(ei, n, w, bvec)
    return worst_ratio(got, edge_weighted_rowsum(ei, n, w, bvec), gamma(length + 1).unsqueeze(-1) * s)


# ------------------------------------------------------------------------------------------- fp32, slot by slot, in CSR order
def _walk(rowptr, n):
    """Yields (rows, slots) for k = 0, 1, ...: the rows that have a k-th slot and that slot."""
    length = rowptr[1:] - rowptr[:-1]
    for k in range(int(length.max()) if n else 0):
        rows = torch.nonzero(length > k).squeeze(-1)
        yield rows, rowptr[rows] + k


def slotwise(ei, n, orders, transpose=False):
    """(rowptr, col, emap) of the orientation, emap: slot -> caller's edge id."""
    eid_t, perm_s, rowptr_t, rowptr_s = orders
    if transpose:
        emap = eid_t[perm_s]
        return rowptr_s, ei[1][emap], emap
    return rowptr_t, ei[0][eid_t], eid_t


def spmm_f32(ei, n, orders, w, x, transpose=False, self_scale=0.0):
    """fp32: acc += w x per slot in CSR order, the self term last - the kernel's order without its FMA."""
    rowptr, col, emap = slotwise(ei, n, orders, transpose)
    acc = torch.zeros(n, x.shape[1], dtype=F32)
    for rows, slots in _walk(rowptr, n):
        term = x[col[slots]] if w is None else w[emap[slots]].unsqueeze(-1) * x[col[slots]]
        acc[rows] = acc[rows] + term
    return acc + torch.tensor(self_scale, dtype=F32) * x if self_scale != 0.0 else acc


def edge_rowsum_f32(ei, n, orders, vals, by_source=False):
    rowptr, _, emap = slotwise(ei, n, orders, by_source)
    acc = torch.zeros(n, dtype=F32)
    for rows, slots in _walk(rowptr, n):
        acc[rows] = acc[rows] + vals[emap[slots]]
    return acc


def edge_weighted_rowsum_f32(ei, n, orders, w, bvec):
    rowptr, _, emap = slotwise(ei, n, orders)
    acc = torch.zeros(n, bvec.shape[1], dtype=F32)
    for rows, slots in _walk(rowptr, n):
        acc[rows] = acc[rows] + w[emap[slots]].unsqueeze(-1) * bvec[emap[slots]]
    return acc


def edge_softmax_f32(ei, n, orders, scores):
    """fp32 as the kernel spells it: running max, running sum of exponentials, one reciprocal per row, a product per slot."""
    rowptr, _, emap = slotwise(ei, n, orders)
    mx = torch.full((n,), float('-inf'), dtype=F32)
    for rows, slots in _walk(rowptr, n):
        mx[rows] = torch.maximum(mx[rows], scores[emap[slots]])
    den = torch.zeros(n, dtype=F32)
    for rows, slots in _walk(rowptr, n):
        den[rows] = den[rows] + (scores[emap[slots]] - mx[rows]).exp()
    inv = 1.0 / (den + torch.tensor(1e-16, dtype=F32))
    return (scores - mx[ei[1]]).exp() * inv[ei[1]]


def edge_softmax_backward_f32(ei, n, orders, alpha, dalpha):
    rowptr, _, emap = slotwise(ei, n, orders)
    d = torch.zeros(n, dtype=F32)
    for rows, slots in _walk(rowptr, n):
        d[rows] = d[rows] + alpha[emap[slots]] * dalpha[emap[slots]]
    return alpha * (dalpha - d[ei[1]])
