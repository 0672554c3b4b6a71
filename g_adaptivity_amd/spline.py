"""Batched not-a-knot interpolating cubic splines on the MI355X: scipy's `UnivariateSpline(x, y, s=0)` of the reference's
Burgers rollout (`src/utils_eval_Burgers.py:215-239, :313-315`), its value and its first two derivatives.

    cubic_spline_1d(x, y, counts, q, q_counts=None, deriv=0) -> (values, status)

One launch of `libgadapt_fem.so` (`gadapt_fem1d_spline`, fem_csrc/spline_kernels.hip) for any number of data sets of mixed
sizes: one workgroup per set, the set in LDS, elimination and evaluation in fp64 on the fp32 data.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native_fem as _nf
from ._native import NativeError, current_stream

__all__ = ['cubic_spline_1d', 'SPLINE_OK', 'SPLINE_NOT_INCREASING', 'SPLINE_NOT_FINITE', 'MIN_POINTS', 'MAX_POINTS']

SPLINE_OK, SPLINE_NOT_INCREASING, SPLINE_NOT_FINITE = _nf.SPLINE_OK, _nf.SPLINE_NOT_INCREASING, _nf.SPLINE_NOT_FINITE
MIN_POINTS, MAX_POINTS = 4, 1024          # GADAPT_FEM1D_MAX_NODES

call_stats = {'calls': 0, 'sets': 0}


def _offsets(counts: Sequence[int], device) -> torch.Tensor:
    return torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=device)


def cubic_spline_1d(x: torch.Tensor, y: torch.Tensor, counts: Sequence[int], q: torch.Tensor,
                    q_counts: Optional[Sequence[int]] = None, deriv: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The not-a-knot cubic spline through each data set, evaluated at the queries: (values, status).

    x, y [sum(counts)]: the sets concatenated, set b of counts[b] points (4..1024), abscissae strictly increasing.
    q, q_counts=None: one array [Q] of query points shared by all sets; values is [B, Q].
    q, q_counts given: the sets' own queries concatenated, q_counts[b] of them for set b; values is laid out like q.
    deriv 0, 1 or 2: the value or that derivative.  Queries outside [x[0], x[-1]] use the end pieces, as FITPACK's ext=0.

    status [B] int32, on the device: SPLINE_OK, SPLINE_NOT_INCREASING (some x[i+1] <= x[i]) or SPLINE_NOT_FINITE (a NaN or
    infinity in x or y).  A flagged set's values are NaN; the other sets of the call are not affected, and a set's values
    do not depend on what else is in the call.  GPU tensors in and out; nothing waits for the device; no gradient."""
    for name, t in (('x', x), ('y', y), ('q', q)):
        if not torch.is_tensor(t):
            raise TypeError(f"cubic_spline_1d: {name} must be a tensor (got {type(t).__name__})")
        if not t.is_cuda:
            raise NativeError(f"cubic_spline_1d: the spline runs on the MI355X only ({name} is a {t.device} tensor); "
                              "there is no CPU fallback")
    if deriv not in (0, 1, 2):
        raise ValueError(f"cubic_spline_1d: deriv={deriv!r}; 0, 1 or 2")
    counts = [int(c) for c in counts]
    if not counts:
        raise ValueError("cubic_spline_1d: no data sets")
    if min(counts) < MIN_POINTS or max(counts) > MAX_POINTS:
        raise ValueError(f"cubic_spline_1d: sets of {min(counts)}..{max(counts)} points; {MIN_POINTS}..{MAX_POINTS} per set "
                         "(a cubic needs four, and a set lives in one workgroup's LDS)")
    if x.dim() != 1 or y.shape != x.shape or x.shape[0] != sum(counts):
        raise ValueError(f"cubic_spline_1d: x {tuple(x.shape)} and y {tuple(y.shape)} for counts summing to {sum(counts)}")
    if q.dim() != 1:
        raise ValueError(f"cubic_spline_1d: q must be one-dimensional (got {tuple(q.shape)})")
    dev, B = x.device, len(counts)
    x, y, q = (t.detach().to(device=dev, dtype=torch.float32).contiguous() for t in (x, y, q))
    if q_counts is None:
        Q = int(q.shape[0])
        if Q < 1:
            raise ValueError("cubic_spline_1d: no query points")
        q_off, out = None, torch.empty(B, Q, device=dev)
    else:
        q_counts = [int(c) for c in q_counts]
        if len(q_counts) != B or min(q_counts) < 0 or sum(q_counts) != q.shape[0]:
            raise ValueError(f"cubic_spline_1d: q_counts {q_counts[:8]}... for {B} sets and {q.shape[0]} queries")
        if q.shape[0] < 1:
            raise ValueError("cubic_spline_1d: no query points")
        Q, q_off, out = 0, _offsets(q_counts, dev), torch.empty(q.shape[0], device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    off = _offsets(counts, dev)
    with torch.cuda.device(dev):
        # sets and queries, not a mesh batch with Gaussians: the head is spelt here and not by fem1d._Batch
        _nf.call('gadapt_fem1d_spline', B, max(counts), off.data_ptr(), x.data_ptr(), y.data_ptr(), Q, q.data_ptr(),
                 None if q_off is None else q_off.data_ptr(), int(deriv), out.data_ptr(), status.data_ptr(), current_stream(dev))
    call_stats['calls'] += 1
    call_stats['sets'] += B
    return out, status
