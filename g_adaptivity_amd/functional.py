"""Autograd-facing wrappers over the C-ABI (include/gadapt_hip.h).

`grand_euler_block` is the loop of `src/GNN.py:273-291` over GRAND / GRAND_plus layers
(`src/GRAND_plus.py:204-343`) as one differentiable op: L fused forward launches, and in
backward 2 launches per layer plus the small weight-gradient chain.  Tensors are only
handed over as raw device pointers on the current HIP stream; nothing here computes on
the CPU and nothing falls back to torch ops.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import os

import torch

from . import _native
from ._native import check, current_stream, lib, ptr
from .graph import MeshGraph


def _require_gpu(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise _native.NativeError(f"{what}: the message-passing path runs on the MI355X only (got a {t.device} tensor); "
                                  "there is no CPU fallback")
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: fp32 expected, got {t.dtype}")


def bucket_cuts(c: int, S: int = 1):
    """Offsets of [Wq | bq | Wk | bk | end] (S stacked convs each) in a flat parameter or gradient bucket: the layout FlatAdam gives
    the conv parameters and the weight-gradient ops return."""
    return [0, S * c * c, S * (c * c + c), S * (2 * c * c + c), S * (2 * c * c + 2 * c)]


def composite_coeffs(wq, bq, wk):
    """(A, p0) = (Wk^T Wq, Wk^T bq) on device via the native kernel (no autograd)."""
    c = wq.shape[0]
    a = torch.empty(c, c, device=wq.device, dtype=torch.float32)
    p0 = torch.empty(c, device=wq.device, dtype=torch.float32)
    check(lib().gadapt_coeffs_forward(ptr(wq), ptr(bq), ptr(wk), ptr(a), ptr(p0), c, current_stream(wq.device)),
          'gadapt_coeffs_forward')
    return a, p0


class _GrandEulerBlock(torch.autograd.Function):
    """x_L = Euler^L(x_0).  Parameters stacked per distinct layer: wq/wk [S,C,C], bq/bk [S,C],
    S = 1 (share_conv) or L; layer_params [L,2] = (dt, score_scale).

    `steps` (trailing inputs, optional): the L one-element step parameters of `learn_step` (`GNN.steps`, GNN.py:179-180) handed
    over as they are; `layer_params` is then the [L] vector of score scales.  The op packs (dt_l, scale_l) itself (one launch)
    and returns d dt_l as one-element slices of the SAME flat tensor that carries the weight gradients, laid out
    [dWq | dbq | dWk | dbk | d dt (L) | d scale (L)]: autograd installs them as `.grad` without copies and `FlatAdam` adopts the
    whole range as its bucket - the `learn_step` path costs two small launches more than the fixed-step path, not ten."""

    @staticmethod
    def forward(ctx, x0, wq, bq, wk, bk, layer_params, graph: MeshGraph, num_layers: int, want_alpha: bool, x_all=None,
                out_cols=None, x0_cols=0, coeffs=None, narrow=False, *steps):
        for t, n in ((x0, 'x'), (wq, 'lin_query.weight'), (bq, 'lin_query.bias'), (wk, 'lin_key.weight'),
                     (layer_params, 'layer_params')):
            _require_gpu(t, n)
        n, c = x0.shape
        if x0_cols:                            # x0 = the compact [N,4] identity-encoder output at the start of x_all's slot 0
            assert x0_cols == 4 and c == 4 and x_all is not None and not ctx.needs_input_grad[0]
            c = x_all[0].shape[2]
        if n != graph.num_nodes:
            raise ValueError(f"x has {n} rows but the graph has {graph.num_nodes} nodes")
        if c not in _native.SUPPORTED_HIDDEN:
            raise NotImplementedError(f"hidden_dim={c}: fused kernels are built for {_native.SUPPORTED_HIDDEN}")
        L, S = int(num_layers), wq.shape[0]
        ctx.n_steps, ctx.step_shapes = len(steps), [tuple(s_.shape) for s_ in steps]
        if steps:
            assert len(steps) == L and layer_params.shape == (L,) and all(s_.numel() == 1 for s_ in steps)
            parts = []
            for l in range(L):
                _require_gpu(steps[l], f'steps.{l}')
                parts += [steps[l].reshape(1), layer_params[l:l + 1]]
            layer_params = torch.cat(parts).view(L, 2)                     # (dt_l, scale_l) pairs: one launch
        assert S in (1, L) and layer_params.shape == (L, 2)
        dev, st = x0.device, current_stream(x0.device)
        wq, bq, wk = wq.contiguous(), bq.contiguous(), wk.contiguous()
        layer_params = layer_params.contiguous()
        if coeffs is not None:                 # (A, p0) of these very weights, already computed (merged encoder launch)
            a, p0 = coeffs[0]
            assert a.shape == (S, c, c) and p0.shape == (S, c) and a.is_contiguous() and p0.is_contiguous()
        else:
            a = torch.empty(S, c, c, device=dev, dtype=torch.float32)
            p0 = torch.empty(S, c, device=dev, dtype=torch.float32)
            for s in range(S):
                check(lib().gadapt_coeffs_forward(ptr(wq[s]), ptr(bq[s]), ptr(wk[s]), ptr(a[s]), ptr(p0[s]), c, st),
                      'gadapt_coeffs_forward')
        need_grad = any(ctx.needs_input_grad[:6]) or any(ctx.needs_input_grad[14:])
        # narrow: every slot holds [N,4] rows at its start (x_top4 the last layer's); only with the compact x0 and the [N,4] head
        narrow = bool(narrow) and bool(x0_cols) and out_cols is not None and out_cols <= 4 and not steps
        if x_all is None:                      # else: caller's [(L+1),N,C] buffer whose slot 0 already holds x0
            x_all = torch.empty(L + 1, n, c, device=dev, dtype=torch.float32)
            x_all[0].copy_(x0)
        else:
            x_all = x_all[0]                   # boxed in a list so autograd does not track it as an input
            assert x_all.shape == (L + 1, n, c) and x_all.is_contiguous() and x_all.data_ptr() == x0.data_ptr()
        keep_alpha = need_grad or want_alpha
        alpha = torch.empty(L, max(graph.num_edges, 1), device=dev, dtype=torch.float32) if keep_alpha else None
        # out_cols <= 4: the last layer writes only the [N,4] head of its rows (x_phys = x[:, :dim], GNN.py:299)
        x_top4 = torch.empty(n, 4, device=dev, dtype=torch.float32) if (out_cols is not None and out_cols <= 4) else None
        fwd = lib().gadapt_block_forward_narrow if narrow else lib().gadapt_block_forward
        check(fwd(graph.c_ref, ptr(x_all), int(x0_cols), L, ptr(a), c * c if S > 1 else 0,
                  ptr(p0), c if S > 1 else 0, ptr(layer_params), ptr(alpha), ptr(x_top4), c, st),
              'gadapt_block_forward_narrow' if narrow else 'gadapt_block_forward')
        ctx.graph, ctx.L, ctx.S, ctx.c, ctx.narrow = graph, L, S, c, narrow
        ctx.out_cols, ctx.x0_cols = out_cols, int(x0_cols)
        ctx.save_for_backward(x_all, alpha if need_grad else None, a, p0, wq, bq, wk, layer_params)
        if x_top4 is not None:
            out = x_top4[:, :out_cols]
        else:
            out = x_all[L] if out_cols is None else x_all[L][:, :out_cols]    # x[:, :dim] (GNN.py:299)
        if want_alpha:
            ctx.mark_non_differentiable(alpha)
            return out, alpha
        return out, None

    @staticmethod
    def backward(ctx, g_top, _g_alpha):
        x_all, alpha, a, p0, wq, bq, wk, layer_params = ctx.saved_tensors
        graph, L, S, c = ctx.graph, ctx.L, ctx.S, ctx.c
        n = graph.num_nodes
        dev, st = g_top.device, current_stream(g_top.device)
        g_top = g_top.contiguous()
        g_cols = 0
        if ctx.out_cols is not None:
            if ctx.out_cols <= 4:
                g_cols = int(ctx.out_cols)      # the top layer's kernels read the compact [N,dim] gradient directly
            else:                               # one zero-padding pass instead of autograd's zeros + slice copy
                g_phys, g_top = g_top, torch.empty(n, c, device=dev, dtype=torch.float32)
                check(lib().gadapt_pad_columns(ptr(g_phys), ptr(g_top), n, ctx.out_cols, c, st), 'gadapt_pad_columns')
        need_x0 = ctx.needs_input_grad[0]
        slab_floats = lib().gadapt_backward_slab_floats(n, c)
        slab_rows = lib().gadapt_backward_slab_rows(n, c)
        g_ws = torch.empty(2, n, c, device=dev, dtype=torch.float32)
        dxd_ws = torch.empty(n, c, device=dev, dtype=torch.float32)
        edge_ws = torch.empty(max(graph.num_edges, 1), 2, device=dev, dtype=torch.float32)
        slab = torch.empty(S, slab_floats, device=dev, dtype=torch.float32)
        want_lp = ctx.needs_input_grad[5] or any(ctx.needs_input_grad[14:])
        # one flat tensor [dWq | dbq | dWk | dbk | d dt (L) | d scale (L)]: installed as the parameters' .grad without a copy, it
        # is the gradient bucket of optim.FlatAdam (one Adam launch, one all-reduce); the 2L tail only when a step / scale
        # gradient is wanted (summed from per-workgroup partials by gadapt_layer_params_reduce)
        n_w = S * (2 * c * c + 2 * c)
        flat = torch.empty(n_w + (2 * L if want_lp else 0), device=dev, dtype=torch.float32)
        d_lp = d_ws = None
        if want_lp:
            d_lp = flat[n_w:]                   # [2,L], written whole by gadapt_layer_params_reduce below
            d_ws = torch.empty(2 * L * slab_rows, device=dev, dtype=torch.float32)   # one slot per (kind, layer, workgroup)
        d_x0 = torch.empty(n, c, device=dev, dtype=torch.float32) if need_x0 else None
        bwd = lib().gadapt_block_backward_narrow if ctx.narrow else lib().gadapt_block_backward
        check(bwd(graph.c_ref, ptr(x_all), ctx.x0_cols, ptr(alpha), ptr(g_top), g_cols, L,
                  ptr(a), c * c if S > 1 else 0, ptr(p0), c if S > 1 else 0, ptr(layer_params),
                  ptr(g_ws), ptr(dxd_ws), ptr(edge_ws), ptr(slab), ptr(d_ws), int(bool(ctx.needs_input_grad[5])),
                  ptr(d_x0), c, st),
              'gadapt_block_backward_narrow' if ctx.narrow else 'gadapt_block_backward')
        scratch = torch.empty(32 * (c * c + c), device=dev, dtype=torch.float32)
        cuts = bucket_cuts(c, S)
        d_wq, d_wk = flat[cuts[0]:cuts[1]].view(S, c, c), flat[cuts[2]:cuts[3]].view(S, c, c)
        d_bq, d_bk = flat[cuts[1]:cuts[2]].view(S, c), flat[cuts[3]:cuts[4]].view(S, c)
        for s in range(S):                      # slab -> second-level sums + chain rule to the Linear parameters: 2 launches
            lp_here = want_lp and s == 0       # the d dt / d scale partials are summed by extra workgroups of the first launch
            check(lib().gadapt_slab_reduce_coeffs_backward(ptr(slab[s]), slab_rows, ptr(scratch), ptr(wq[s]), ptr(bq[s]), ptr(wk[s]),
                                                           ptr(d_wq[s]), ptr(d_bq[s]), ptr(d_wk[s]), ptr(d_bk[s]), c, st,
                                                           ptr(d_ws) if lp_here else None, L, int(bool(ctx.needs_input_grad[5])),
                                                           ptr(d_lp) if lp_here else None),
                  'gadapt_slab_reduce_coeffs_backward')
        if ctx.n_steps:                         # layer_params was the [L] scale vector; the steps get their slices of the d dt row
            d_scales = d_lp[L:] if ctx.needs_input_grad[5] else None
            d_steps = tuple(d_lp[l:l + 1].view(ctx.step_shapes[l]) if ctx.needs_input_grad[14 + l] else None for l in range(L))
            return (d_x0, d_wq, d_bq, d_wk, d_bk, d_scales, None, None, None, None, None, None, None, None) + d_steps
        d_lp2 = d_lp.view(2, L).t() if ctx.needs_input_grad[5] else None     # [L,2] view of the [2,L] rows
        return d_x0, d_wq, d_bq, d_wk, d_bk, d_lp2, None, None, None, None, None, None, None, None


class _GrandResidual(torch.autograd.Function):
    """res = A(x)x - x for one layer: the return value of `GRAND_plusConv.forward`
    (`src/GRAND_plus.py:267`) / `GRAND_conv.forward` (`:380-382`)."""

    @staticmethod
    def forward(ctx, x, wq, bq, wk, bk, scale, graph: MeshGraph, want_alpha: bool):
        for t, n in ((x, 'x'), (wq, 'lin_query.weight'), (bq, 'lin_query.bias'), (wk, 'lin_key.weight'), (scale, 'scale')):
            _require_gpu(t, n)
        n, c = x.shape
        if n != graph.num_nodes:
            raise ValueError(f"x has {n} rows but the graph has {graph.num_nodes} nodes")
        if c not in _native.SUPPORTED_HIDDEN:
            raise NotImplementedError(f"hidden_dim={c}: fused kernels are built for {_native.SUPPORTED_HIDDEN}")
        dev, st = x.device, current_stream(x.device)
        x, wq, bq, wk = x.contiguous(), wq.contiguous(), bq.contiguous(), wk.contiguous()
        a, p0 = composite_coeffs(wq, bq, wk)
        lp = torch.stack([torch.ones((), device=dev), scale.reshape(())]).contiguous()
        need_grad = any(ctx.needs_input_grad[:6])
        res = torch.empty_like(x)
        alpha = torch.empty(max(graph.num_edges, 1), device=dev, dtype=torch.float32) if (need_grad or want_alpha) else None
        check(lib().gadapt_layer_forward(graph.c_ref, ptr(x), ptr(res), ptr(a), ptr(p0), ptr(lp), ptr(alpha), 1, c, st),
              'gadapt_layer_forward')
        ctx.graph, ctx.c = graph, c
        ctx.save_for_backward(x, alpha if need_grad else None, a, p0, wq, bq, wk, lp)
        if want_alpha:
            ctx.mark_non_differentiable(alpha)
            return res, alpha
        return res, None

    @staticmethod
    def backward(ctx, g, _g_alpha):
        x, alpha, a, p0, wq, bq, wk, lp = ctx.saved_tensors
        graph, c = ctx.graph, ctx.c
        n = graph.num_nodes
        dev, st = g.device, current_stream(g.device)
        g = g.contiguous()
        slab = torch.empty(lib().gadapt_backward_slab_floats(n, c), device=dev, dtype=torch.float32)
        dxd_ws, d_x = torch.empty_like(x), torch.empty_like(x)
        edge_ws = torch.empty(max(graph.num_edges, 1), 2, device=dev, dtype=torch.float32)
        sums = torch.zeros(2, device=dev, dtype=torch.float32)
        check(lib().gadapt_layer_backward(graph.c_ref, ptr(x), ptr(g), ptr(alpha), ptr(a), ptr(p0), ptr(lp), ptr(edge_ws),
                                          ptr(dxd_ws), ptr(slab), 0, ptr(sums), ptr(d_x), 1, c, st), 'gadapt_layer_backward')
        scratch = torch.empty(32 * (c * c + c), device=dev, dtype=torch.float32)
        d_a, d_p0 = torch.empty(c, c, device=dev), torch.empty(c, device=dev)
        d_wq, d_bq, d_wk, d_bk = (torch.empty_like(t) for t in (wq, bq, wk, bq))
        check(lib().gadapt_slab_reduce(ptr(slab), lib().gadapt_backward_slab_rows(n, c), ptr(scratch), ptr(d_a), ptr(d_p0), c, st),
              'gadapt_slab_reduce')
        check(lib().gadapt_coeffs_backward(ptr(wq), ptr(bq), ptr(wk), ptr(d_a), ptr(d_p0), ptr(d_wq), ptr(d_bq), ptr(d_wk),
                                           ptr(d_bk), c, st), 'gadapt_coeffs_backward')
        return d_x, d_wq, d_bq, d_wk, d_bk, sums[1].reshape(()), None, None


def grand_residual(x, wq, bq, wk, bk, scale: torch.Tensor, graph: MeshGraph, want_alpha: bool = False):
    """(A(x)x - x [N,C], alpha [E] in target-CSR order or None); `scale` is a 0-d device tensor."""
    return _GrandResidual.apply(x, wq, bq, wk, bk, scale, graph, want_alpha)


def grand_euler_block(x0: torch.Tensor, wq, bq, wk, bk, layer_params: torch.Tensor, graph: MeshGraph,
                      num_layers: int, want_alpha: bool = False, x_all: Optional[torch.Tensor] = None,
                      out_cols: Optional[int] = None, x0_cols: int = 0, coeffs=None, steps=None, narrow: bool = False):
    """Returns (x_L [N,C], alpha [L,E] in target-CSR order or None).

    `x_all` (optional): a contiguous [(L+1),N,C] buffer whose slot 0 IS `x0` (same memory); the
    layers then write straight into it and no copy of x0 is made.  `out_cols`: return only the first
    columns of x_L (the `x[:, :dim]` slice of `src/GNN.py:299`) with a single-pass backward.
    `x0_cols=4`: `x0` is the compact [N,4] output of the identity encoder (zero-pad, `src/GNN.py:75-82`) stored at the
    start of `x_all`'s slot 0; layer 0 reads it directly and the padded [N,C] matrix is never written.
    `coeffs=(a [S,C,C], p0 [S,C])`: the composite coefficients of exactly these weights when the caller has them already
    (`encode_features(..., conv=...)` computes them in the encoder's launch).
    `steps`: the L one-element step parameters (`learn_step`); `layer_params` is then the [L] vector of score scales (see
    `_GrandEulerBlock`).  `narrow`: the block runs on the four live columns (`GNN._route`'s `narrow`) - only
    with `x0_cols=4`, `out_cols <= 4`, fixed steps, on a graph where `MeshGraph.narrow_route` holds."""
    return _GrandEulerBlock.apply(x0.contiguous(), wq, bq, wk, bk, layer_params, graph, num_layers, want_alpha,
                                  None if x_all is None else [x_all], out_cols, x0_cols, None if coeffs is None else [coeffs],
                                  bool(narrow), *(steps or ()))


NONLIN_CODES = {'identity': 0, 'relu': 1, 'tanh': 2, 'sigmoid': 3, 'leaky_relu': 4, 'elu': 5, 'selu': 6}   # get_nonlin, src/GNN.py:48-64


class _GatPlusBlock(torch.autograd.Function):
    """x_L = the L iterations of `src/GNN.py:273-296` around `GAT_plus.forward` (`src/GRAND_plus.py:400-416`) on the self-looped
    graph: per layer one fused forward launch, in backward a target-side and a source-side launch plus the ordered sum of the
    att_src / att_dst gradient partials (include/gadapt_hip.h, gadapt_gat_plus_block_*).  att_src / att_dst: [S,C], S = 1
    (share_conv) or L."""

    @staticmethod
    def forward(ctx, x0, att_src, att_dst, looped: MeshGraph, num_layers: int, dt: float, residual: bool, res_lap: bool, non_lin: int,
                out_cols=None, x_all=None):
        for t, n in ((x0, 'x'), (att_src, 'att_src'), (att_dst, 'att_dst')):
            _require_gpu(t, n)
        n, c = x0.shape
        if n != looped.num_nodes:
            raise ValueError(f"x has {n} rows but the graph has {looped.num_nodes} nodes")
        if c not in _native.SUPPORTED_HIDDEN:
            raise NotImplementedError(f"hidden_dim={c}: fused kernels are built for {_native.SUPPORTED_HIDDEN}")
        L, S = int(num_layers), att_src.shape[0]
        assert S in (1, L) and att_src.shape == (S, c) and att_dst.shape == (S, c)
        dev, st = x0.device, current_stream(x0.device)
        att_src, att_dst = att_src.contiguous(), att_dst.contiguous()
        if x_all is None:                      # else: the caller's [(L+1),N,C] buffer whose slot 0 already IS x0 (no copy)
            x_all = torch.empty(L + 1, n, c, device=dev, dtype=torch.float32)
            x_all[0].copy_(x0)
        else:
            x_all = x_all[0]                   # boxed in a list so autograd does not track it as an input
            assert x_all.shape == (L + 1, n, c) and x_all.is_contiguous() and x_all.data_ptr() == x0.data_ptr()
        ab = torch.empty(L, 2, n, device=dev, dtype=torch.float32)
        alpha = torch.empty(L, max(looped.num_edges, 1), device=dev, dtype=torch.float32)
        check(lib().gadapt_gat_plus_block_forward(looped.c_ref, ptr(x_all), L, ptr(att_src), ptr(att_dst), c if S > 1 else 0, float(dt),
                                                  int(bool(residual)), int(bool(res_lap)), int(non_lin), ptr(ab), ptr(alpha), c, st),
              'gadapt_gat_plus_block_forward')
        ctx.graph, ctx.L, ctx.S, ctx.c = looped, L, S, c
        ctx.cfg = (float(dt), int(bool(residual)), int(bool(res_lap)), int(non_lin))
        ctx.out_cols = out_cols
        ctx.save_for_backward(x_all, alpha, ab, att_src, att_dst)
        ctx.mark_non_differentiable(alpha)
        out = x_all[L] if out_cols is None else x_all[L][:, :out_cols]          # x[:, :dim] (GNN.py:299)
        return out, alpha

    @staticmethod
    def backward(ctx, g_top, _g_alpha):
        x_all, alpha, ab, att_src, att_dst = ctx.saved_tensors
        graph, L, S, c = ctx.graph, ctx.L, ctx.S, ctx.c
        dt, residual, res_lap, non_lin = ctx.cfg
        n = graph.num_nodes
        dev, st = g_top.device, current_stream(g_top.device)
        g_top = g_top.contiguous()
        if ctx.out_cols is not None:            # one zero-padding pass instead of autograd's zeros + slice copy
            g_phys, g_top = g_top, torch.empty(n, c, device=dev, dtype=torch.float32)
            check(lib().gadapt_pad_columns(ptr(g_phys), ptr(g_top), n, ctx.out_cols, c, st), 'gadapt_pad_columns')
        g_ws = torch.empty(2, n, c, device=dev, dtype=torch.float32)
        gr_ws = torch.empty(n, c, device=dev, dtype=torch.float32)
        dz_ws = torch.empty(max(graph.num_edges, 1), device=dev, dtype=torch.float32)
        db_ws = torch.empty(n, device=dev, dtype=torch.float32)
        part = torch.empty(lib().gadapt_gat_plus_partial_rows(n, c), 2 * c, device=dev, dtype=torch.float32)
        d_att = torch.empty(S, 2, c, device=dev, dtype=torch.float32)          # (d att_src | d att_dst): one flat tensor, FlatAdam's bucket
        d_x0 = torch.empty(n, c, device=dev, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        check(lib().gadapt_gat_plus_block_backward(graph.c_ref, ptr(x_all), ptr(alpha), ptr(ab), ptr(g_top), L, ptr(att_src), ptr(att_dst),
                                                   c if S > 1 else 0, dt, residual, res_lap, non_lin, ptr(g_ws), ptr(gr_ws), ptr(dz_ws),
                                                   ptr(db_ws), ptr(part), ptr(d_att), ptr(d_x0), c, st), 'gadapt_gat_plus_block_backward')
        return d_x0, d_att[:, 0], d_att[:, 1], None, None, None, None, None, None, None, None


def gat_plus_block(x0: torch.Tensor, att_src: torch.Tensor, att_dst: torch.Tensor, looped: MeshGraph, num_layers: int, dt: float,
                   residual: bool = True, res_lap: bool = True, non_lin: str = 'identity', out_cols: Optional[int] = None,
                   x_all: Optional[torch.Tensor] = None):
    """(x_L [N,C] or its first `out_cols` columns, alpha [L,E] in the target-CSR order of `looped`): L fused GAT_plus layers with
    the update of `src/GNN.py:284-296`.  `looped` = `graph.with_self_loops()` (GATConv's edge surgery)."""
    return _GatPlusBlock.apply(x0.contiguous(), att_src, att_dst, looped, num_layers, dt, residual, res_lap, NONLIN_CODES[non_lin], out_cols,
                               None if x_all is None else [x_all])


def score_scale(hidden_dim: int, temperature=None):
    """1/(sqrt(C) T): `src/GRAND_plus.py:279` and `:35-37`."""
    s = 1.0 / math.sqrt(hidden_dim)
    return s if temperature is None else s / temperature


def encode_linear(feats: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x0 = feats @ W^T (+b) through the native kernel (frozen encoder: no autograd)."""
    _require_gpu(feats, 'features')
    n, f = feats.shape
    c = weight.shape[0]
    x0 = torch.empty(n, c, device=feats.device, dtype=torch.float32) if out is None else out
    assert x0.shape == (n, c) and x0.is_contiguous()
    check(lib().gadapt_encode_linear(ptr(feats.contiguous()), ptr(weight.contiguous()),
                                     ptr(bias.contiguous()) if bias is not None else None,
                                     ptr(x0), n, f, c, current_stream(feats.device)), 'gadapt_encode_linear')
    return x0


def encode_features(x_comp: torch.Tensor, f_tensor: Optional[torch.Tensor], uu_tensor: Optional[torch.Tensor],
                    weight: torch.Tensor, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, conv=None):
    """x0 = enc([x_comp | f | uu]) (`src/GNN.py:225-239,270`) without materialising the concatenated feature matrix.
    `conv=(wq, bq, wk)` (weights of ONE conv, [C,C] / [C]): the same launch also computes that conv's composite
    coefficients; returns (x0, (a [1,C,C], p0 [1,C])) instead of x0."""
    _require_gpu(x_comp, 'x_comp')
    n, dim = x_comp.shape
    c = weight.shape[0]
    for t, name in ((f_tensor, 'f_tensor'), (uu_tensor, 'uu_tensor')):
        if t is not None:
            _require_gpu(t, name)
            if t.shape != (n,) or not t.is_contiguous():
                raise ValueError(f"{name}: expected a dense [{n}] tensor, got {tuple(t.shape)}")
    if weight.shape[1] != dim + (f_tensor is not None) + (uu_tensor is not None):
        raise ValueError(f"encoder weight has {weight.shape[1]} input columns for {dim} coordinates + extras")
    x0 = torch.empty(n, c, device=x_comp.device, dtype=torch.float32) if out is None else out
    assert x0.shape == (n, c) and x0.is_contiguous()
    if conv is not None:
        wq, bq, wk = (t.detach().contiguous() for t in conv)
        cc = wq.shape[0]
        a = torch.empty(1, cc, cc, device=x_comp.device, dtype=torch.float32)
        p0 = torch.empty(1, cc, device=x_comp.device, dtype=torch.float32)
        check(lib().gadapt_encode_features_coeffs(ptr(x_comp.contiguous()), dim, ptr(f_tensor), ptr(uu_tensor), ptr(weight.contiguous()),
                                                  ptr(bias.contiguous()) if bias is not None else None, ptr(x0), n, c,
                                                  ptr(wq), ptr(bq), ptr(wk), ptr(a), ptr(p0), cc, current_stream(x_comp.device)),
              'gadapt_encode_features_coeffs')
        return x0, (a, p0)
    check(lib().gadapt_encode_features(ptr(x_comp.contiguous()), dim, ptr(f_tensor), ptr(uu_tensor), ptr(weight.contiguous()),
                                       ptr(bias.contiguous()) if bias is not None else None, ptr(x0), n, c,
                                       current_stream(x_comp.device)), 'gadapt_encode_features')
    return x0


# One-launch evaluation forward of a batch of small meshes (csrc/gadapt_smallmesh.inc); False keeps the per-layer launches
# everywhere (tests compare the two).
SMALL_MESH_FORWARD = os.environ.get('GADAPT_SMALL_MESH', '1') != '0'
SMALL_MESH_FORCE = os.environ.get('GADAPT_SMALL_MESH', '1') == '2'      # experiments: every size the kernels take, whatever the policies say


def small_forward_policy(c: int, max_nodes: int) -> bool:
    """Sizes at which the one-launch forward is the faster one (tools/gpu_small_c16.sh / tools/sweep_small_mesh.py, time between HIP
    events around the replayed forward, one-launch against per-layer: hidden 8: 14.6 / 28.8 us at 11 x 11 ... 29.1 / 29.5 at 31 x 31;
    hidden 16: 22.4 / 33.6 at 11 x 11, 29.8 / 34.2 at 19 x 19, 51.3 / 34.3 at 23 x 23; hidden 32: 35.4 / 37.9 at 11 x 11, 52.5 / 38.8 at
    15 x 15).  A workgroup has at most 1024 threads: from 257 nodes on a node has fewer than four lanes, from 513 on one, and the wide
    rows then run long serial chains."""
    return SMALL_MESH_FORCE or c <= 8 or (c == 16 and max_nodes <= 384) or (c == 32 and max_nodes <= 128)


def small_forward_fits(graph: MeshGraph, part, c: int) -> bool:
    """True when gadapt_small_forward takes this partition at hidden size c (rows + CSR slice of the largest mesh within the LDS)
    and the size is one where it pays."""
    return part is not None and c in (4, 8, 16, 32) and small_forward_policy(c, part[2]) \
        and lib().gadapt_small_forward_lds_bytes(part[2], part[3], c) > 0


def small_training_policy(c: int, max_nodes: int) -> bool:
    """Training sizes at which the one-launch forward + one-launch backward pair is the faster step (tools/gpu_small_train.sh,
    tools/gpu_small_c16.sh: captured step, meshes/s against the per-layer kernels.  Hidden 8: 11 x 11, batch 8: 156k / 94k; batch 64:
    1 196k / 720k; 23 x 23, batch 16: 197k / 178k.  Hidden 16: 11 x 11, batch 8: 115k / 91k; 15 x 15, batch 64: 707k / 624k; 20 x 20,
    batch 16: 135k / 172k.  Hidden 32: 44k / 73k at 11 x 11 - its backward holds a 32 x 32 contraction per mesh in one workgroup)."""
    return SMALL_MESH_FORCE or c <= 8 or (c == 16 and max_nodes <= 256)


def small_backward_fits(graph: MeshGraph, part, c: int) -> bool:
    return part is not None and c in (4, 8, 16, 32) and small_training_policy(c, part[2]) \
        and lib().gadapt_small_forward_lds_bytes(part[2], part[3], c) > 0 and lib().gadapt_small_backward_lds_bytes(part[2], part[3], c) > 0


def _small_args(graph, part, x_comp, dim, f_tensor, uu_tensor, enc_weight, wq, bq, wk, S, layer_params, num_layers, out, out_cols, alpha, x_all):
    """gadapt_small_forward's argument list up to x_all (gadapt_small_forward_loss continues it with the loss arguments); fields by
    address (int or None), everything else as tensors."""
    mesh_ptr, n_meshes, max_nodes, max_edges = part
    c = wq.shape[-1]
    return [graph.c_ref, ptr(mesh_ptr[0]), ptr(mesh_ptr[1]), n_meshes, max_nodes, max_edges, x_comp, dim, f_tensor, uu_tensor, ptr(enc_weight),
            enc_weight.shape[1], ptr(wq), ptr(bq), ptr(wk), c * c if S > 1 else 0, c if S > 1 else 0, ptr(layer_params), num_layers, ptr(out),
            out_cols, ptr(alpha), ptr(x_all)]


def _small_launch(graph, part, x_comp, f_tensor, uu_tensor, enc_weight, wq, bq, wk, layer_params, num_layers, out_cols, want_alpha, keep):
    n, dim = x_comp.shape
    c, S = wq.shape[1], wq.shape[0]
    dev = x_comp.device
    out = torch.empty(n, out_cols, device=dev, dtype=torch.float32)
    alpha = torch.empty(num_layers, max(graph.num_edges, 1), device=dev, dtype=torch.float32) if (want_alpha or keep) else None
    x_all = torch.empty(num_layers, n, c, device=dev, dtype=torch.float32) if keep else None
    check(lib().gadapt_small_forward(*_small_args(graph, part, ptr(x_comp), dim, ptr(f_tensor), ptr(uu_tensor), enc_weight, wq, bq, wk, S,
                                                  layer_params, num_layers, out, out_cols, alpha, x_all), c, current_stream(dev)),
          'gadapt_small_forward')
    return out, alpha, x_all


@torch.no_grad()
def small_forward(graph: MeshGraph, part, x_comp, f_tensor, uu_tensor, enc_weight, wq, bq, wk, layer_params, num_layers: int,
                  out_cols: int, want_alpha: bool = False):
    """x_phys [N,out_cols] (and alpha [L,E] in target-CSR order, or None) of encoder + L Euler steps + head in ONE launch, one
    workgroup per mesh (`src/GNN.py:225-299` for batches of small meshes: the reference's own sizes).  Inference: nothing is
    kept for a backward (`small_block` is the differentiable form).  wq / bq / wk: [S,C,C] / [S,C], S = 1 (shared conv) or L;
    layer_params [L,2] = (dt, score scale)."""
    _require_gpu(x_comp, 'x_comp')
    out, alpha, _ = _small_launch(graph, part, x_comp.contiguous(), f_tensor, uu_tensor, enc_weight.contiguous(), wq.contiguous(), bq.contiguous(),
                                  wk.contiguous(), layer_params.contiguous(), num_layers, out_cols, want_alpha, False)
    return out, alpha


class _SmallMeshBlock(torch.autograd.Function):
    """Encoder + L Euler steps + head of a small-mesh batch as ONE launch forward and ONE launch backward (csrc/gadapt_smallmesh.inc),
    differentiable wrt the conv parameters (the encoder is frozen, `src/GNN.py:82,89`; the node fields carry no gradient).  The
    parameter gradients come back as slices of one flat tensor laid out like `_GrandEulerBlock`'s ([dWq | dbq | dWk | dbk]), so
    `FlatAdam` adopts it as its bucket."""

    @staticmethod
    def forward(ctx, wq, bq, wk, bk, x_comp, f_tensor, uu_tensor, enc_weight, layer_params, graph, part, num_layers, out_cols):
        for t, n_ in ((x_comp, 'x_comp'), (wq, 'lin_query.weight'), (bq, 'lin_query.bias'), (wk, 'lin_key.weight')):
            _require_gpu(t, n_)
        wq, bq, wk, lp = wq.contiguous(), bq.contiguous(), wk.contiguous(), layer_params.contiguous()
        out, alpha, x_all = _small_launch(graph, part, x_comp.contiguous(), f_tensor, uu_tensor, enc_weight.contiguous(), wq, bq, wk, lp,
                                          num_layers, out_cols, True, True)
        ctx.graph, ctx.part, ctx.L, ctx.out_cols = graph, part, int(num_layers), int(out_cols)
        ctx.save_for_backward(x_all, alpha, wq, bq, wk, lp)
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    def backward(ctx, g_out, _g_alpha):
        x_all, alpha, wq, bq, wk, lp = ctx.saved_tensors
        graph, (mesh_ptr, n_meshes, max_nodes, max_edges), L = ctx.graph, ctx.part, ctx.L
        S, c = wq.shape[0], wq.shape[1]
        dev, st = g_out.device, current_stream(g_out.device)
        g_top = g_out.contiguous()
        row = c * c + c
        slab = torch.empty(S, n_meshes, row, device=dev, dtype=torch.float32)
        check(lib().gadapt_small_backward(graph.c_ref, ptr(mesh_ptr[0]), ptr(mesh_ptr[1]), n_meshes, max_nodes, max_edges, ptr(x_all), ptr(alpha), ptr(g_top),
                                          ctx.out_cols, ptr(wq), ptr(bq), ptr(wk), c * c if S > 1 else 0, c if S > 1 else 0, ptr(lp), L,
                                          ptr(slab), c, st), 'gadapt_small_backward')
        flat = torch.empty(S * (2 * c * c + 2 * c), device=dev, dtype=torch.float32)
        cuts = bucket_cuts(c, S)
        d_wq, d_wk = flat[cuts[0]:cuts[1]].view(S, c, c), flat[cuts[2]:cuts[3]].view(S, c, c)
        d_bq, d_bk = flat[cuts[1]:cuts[2]].view(S, c), flat[cuts[3]:cuts[4]].view(S, c)
        scratch = torch.empty(32 * row, device=dev, dtype=torch.float32)
        for s_ in range(S):
            check(lib().gadapt_slab_reduce_coeffs_backward(ptr(slab[s_]), n_meshes, ptr(scratch), ptr(wq[s_]), ptr(bq[s_]), ptr(wk[s_]),
                                                           ptr(d_wq[s_]), ptr(d_bq[s_]), ptr(d_wk[s_]), ptr(d_bk[s_]), c, st, None, L, 0, None),
                  'gadapt_slab_reduce_coeffs_backward')
        return d_wq, d_bq, d_wk, d_bk, None, None, None, None, None, None, None, None, None


def small_block(graph: MeshGraph, part, x_comp, f_tensor, uu_tensor, enc_weight, wq, bq, wk, bk, layer_params, num_layers: int, out_cols: int):
    """Differentiable one-launch block for small-mesh batches: returns (x_phys [N,out_cols], alpha [L,E])."""
    return _SmallMeshBlock.apply(wq, bq, wk, bk, x_comp, f_tensor, uu_tensor, enc_weight.detach(), layer_params.detach(), graph, part,
                                 num_layers, out_cols)


_loss_scratch = {}


class _MeshLoss(torch.autograd.Function):
    """mean((pred-target)^2) / mean(|pred-target|) with the derivative produced by the same launch."""

    @staticmethod
    def forward(ctx, pred, target, l1: bool):
        _require_gpu(pred, 'loss input')
        _require_gpu(target, 'loss target')
        if pred.shape != target.shape or pred.dim() != 2:
            raise ValueError(f"loss: shapes {tuple(pred.shape)} vs {tuple(target.shape)} (expected equal [N,d])")
        if pred.stride(1) != 1:
            pred = pred.contiguous()
        n, d = pred.shape
        dev = pred.device
        key = (dev, torch.cuda.current_stream(dev).cuda_stream)
        scratch = _loss_scratch.get(key)
        if scratch is None:
            scratch = _loss_scratch[key] = torch.zeros(lib().gadapt_loss_scratch_floats(), device=dev, dtype=torch.float32)
        seed = torch.empty(n, d, device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        check(lib().gadapt_loss_forward(pred.data_ptr(), pred.stride(0), ptr(target.contiguous()), n, d, int(bool(l1)), ptr(seed),
                                        ptr(loss), ptr(scratch), current_stream(dev)), 'gadapt_loss_forward')
        ctx.save_for_backward(seed)
        return loss

    @staticmethod
    def backward(ctx, g):
        (seed,) = ctx.saved_tensors
        unit = _unit_grads.get(g.device)
        if unit is not None and g.data_ptr() == unit.data_ptr():
            return seed, None, None          # the caller passed unit_gradient(): d loss / d loss = 1, nothing to multiply
        return seed * g, None, None


_unit_grads = {}


def unit_gradient(device) -> torch.Tensor:
    """The root gradient of a scalar loss, kept per device: `loss.backward(gradient=unit_gradient(dev))` is
    `loss.backward()` (`src/run_GNN.py:84`) without the two launches autograd otherwise adds per step - filling a fresh
    one-element tensor with 1 and multiplying the loss derivative by it (`mse_loss` / `l1_loss` recognise this tensor by
    its address and hand their derivative on as it is).  Read-only by contract."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    t = _unit_grads.get(device)
    if t is None:
        t = _unit_grads[device] = torch.ones((), device=device, dtype=torch.float32)
    return t


def mse_loss(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """`F.mse_loss(out, data.x_phys)` of the training loop (`src/run_GNN.py:80-84,106`) as one launch (value + derivative)."""
    return _MeshLoss.apply(pred, target, False)


def l1_loss(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """`F.l1_loss(out, data.x_phys)` (`src/run_GNN.py:82`) as one launch."""
    return _MeshLoss.apply(pred, target, True)


def flat_bucket(wq, bq, wk):
    """Address of [Wq | bq | Wk] when the three tensors lie back to back in that order (FlatAdam's bucket), else None."""
    c = wq.shape[0]
    ok = wq.is_contiguous() and bq.is_contiguous() and wk.is_contiguous() and bq.data_ptr() == wq.data_ptr() + 4 * c * c \
        and wk.data_ptr() == bq.data_ptr() + 4 * c
    return wq.data_ptr() if ok else None


class _OneCall:
    """A one-call forward of a weight-shared model: buffers and C-ABI argument list built once; per call only the node-field addresses
    and the stream are filled in.  The list points into the parameters' storage: `moved()` notices storage that moved (FlatAdam lays
    its bucket out, `load_state_dict(assign=True)`, `p.data = ...`) and `bind()` rebuilds the list over the same buffers."""

    def moved(self) -> bool:
        return any(t.data_ptr() != p for t, p in self._live)

    def __call__(self, x_comp, f_tensor, uu_tensor, stream) -> int:
        """Node fields by address (None: not an input).  Returns the number of loss partials written (0 without a target)."""
        a, i = self.args, self._at
        a[i], a[i + 2], a[i + 3], a[-1] = x_comp, f_tensor, uu_tensor, stream
        rc = self._fn(*a)
        if rc < 0:
            check(rc, self._name)
        return rc

    def _buffers(self, model, graph, target, l1, keep_alpha):
        o = model.opt
        self.model, self.graph, self.target, self.l1 = model, graph, target, int(bool(l1))
        self.n, self.c, self.L, self.d = graph.num_nodes, int(o['hidden_dim']), int(o['num_layers']), int(model.dim)
        self.f32 = dict(device=torch.device(o['device']), dtype=torch.float32)
        self.alpha = torch.empty(self.L, max(graph.num_edges, 1), **self.f32) if keep_alpha else None
        self.seed = torch.empty(self.n, self.d, **self.f32) if target is not None else None
        self.partials = torch.zeros(lib().gadapt_loss_partials_max(), **self.f32) if target is not None else None
        self._fn = getattr(lib(), self._name)
        self._conv = model.conv_layers[0]


class BlockForwardCall(_OneCall):
    """`gadapt_block_forward_loss`: the compact block behind the zero-pad identity encoder (layer 0 reads the node fields, the last
    layer writes the [N,4] head `out` is a view of).  With `target` it also writes the loss derivative `seed` and the loss partials
    (`training.FusedIteration`); without, it is the evaluation forward (`inference.GraphedForward`).  `coeffs` (A, p0) are inputs,
    except where the layer-0 launch computes them from weights laid out back to back (`in_forward`: hidden 64 on wide-forward graphs)."""

    _name, _at = 'gadapt_block_forward_loss', 2
    _top = None                                                     # (dxd_ws, edge_ws, slab): see with_backward_buffers

    def __init__(self, model, graph, target=None, l1=False, coeffs=None, store=False, narrow=False):
        self.narrow = bool(narrow)                                 # the route's `narrow`: every slot holds [N,4] rows at its start
        if self.narrow:
            self._name = 'gadapt_block_forward_loss_narrow'
        self._buffers(model, graph, target, l1, target is not None or store)
        n, c, f32 = self.n, self.c, self.f32
        self.x_all = torch.empty(self.L, n, c, **f32)            # slot l = input of layer l (slot 0: the compact [N,4] rows at its start)
        self.x_top4 = torch.empty(n, 4, **f32)
        self.out = self.x_top4[:, :self.d]
        self.coeffs = coeffs if coeffs is not None else (torch.empty(c, c, **f32), torch.empty(c, **f32))
        self.lp = model._layer_params(f32['device']).contiguous()
        self._computes = bool(lib().gadapt_forward_computes_coeffs(graph.c_ref, c))
        self._fn_coeffs = lib().gadapt_coeffs_forward
        if store:
            model._publish_attention(graph, self.alpha)
        self.bind()

    def bind(self):
        cv, c = self._conv, self.c
        wq, bq, wk = self._w = (cv.lin_query.weight, cv.lin_query.bias, cv.lin_key.weight)
        self._live = [(t, t.data_ptr()) for t in self._w]
        self.bucket = flat_bucket(wq, bq, wk)
        self.in_forward = self._computes and self.bucket is not None
        # gadapt_block_forward_loss_narrow_top: + dxd_ws, edge_ws, slab, top_ran between the loss arguments and (c, stream)
        top = [] if self._top is None else [ptr(t) for t in self._top] + [ctypes.addressof(self._top_ran)]
        self.args = [self.graph.c_ref, ptr(self.x_all), None, self.d, None, None, self.L, ptr(self.coeffs[0]), ptr(self.coeffs[1]),
                     self.bucket if self.in_forward else None, ptr(self.lp), ptr(self.alpha), ptr(self.x_top4), ptr(self.target),
                     0 if self.target is None else self.d, self.l1, ptr(self.seed), ptr(self.partials)] + top + [c, None]

    def with_backward_buffers(self, dxd_ws, edge_ws, slab):
        """Narrow route of a fused step (`training.FusedIteration`): the call becomes `gadapt_block_forward_loss_narrow_top`, whose last
        forward launch also runs the top layer's backward target pass into the backward's buffers where the step is eligible;
        `top_ran` then says whether it did, i.e. which backward entry point follows."""
        assert self.narrow and self.target is not None
        self._top, self._top_ran = (dxd_ws, edge_ws, slab), ctypes.c_int(0)
        self._name = 'gadapt_block_forward_loss_narrow_top'
        self._fn = getattr(lib(), self._name)
        self.bind()

    @property
    def top_ran(self) -> bool:
        return self._top is not None and self._top_ran.value != 0

    def compute_coeffs(self, stream):
        """(A, p0) of the weights as they are now: one launch."""
        wq, bq, wk = self._w
        rc = self._fn_coeffs(wq.data_ptr(), bq.data_ptr(), wk.data_ptr(), self.args[7], self.args[8], self.c, stream)
        if rc != 0:
            check(rc, 'gadapt_coeffs_forward')


class SmallForwardCall(_OneCall):
    """`gadapt_small_forward` (evaluation: `inference.GraphedForward`) or, with `target`, `gadapt_small_forward_loss` (the head of a
    small-mesh `training.FusedIteration`, keeping x_all / alpha for its backward): encoder, every layer and the head as ONE launch.
    `route`: the model's route of the batch (`GNN._route`), of form 'small'."""

    _at = 6

    def __init__(self, model, route, target=None, l1=False):
        self._name = 'gadapt_small_forward' if target is None else 'gadapt_small_forward_loss'
        self._buffers(model, route.small['graph'], target, l1, target is not None or route.store)
        self.plan = route.small
        self.out_cols = self.d if (target is not None or route.ident) else self.c
        self.out = torch.empty(self.n, self.out_cols, **self.f32)
        self.x_all = torch.empty(self.L, self.n, self.c, **self.f32) if target is not None else None
        if route.store:
            model._publish_attention(self.graph, self.alpha)
        self.bind()

    def bind(self):
        w = (self._conv.lin_query.weight, self._conv.lin_query.bias, self._conv.lin_key.weight, self.model.enc.weight)
        self._live = [(t, t.data_ptr()) for t in w]
        self.args = _small_args(self.graph, self.plan['part'], None, self.d, None, None, w[3], *w[:3], 1, self.plan['lp'], self.L, self.out,
                                self.out_cols, self.alpha, self.x_all)
        if self.target is not None:
            self.args += [ptr(self.target), self.l1, ptr(self.seed), ptr(self.partials)]
        self.args += [self.c, None]
