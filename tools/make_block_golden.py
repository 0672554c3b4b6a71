"""Golden data of the message-passing block routes, recorded on the MI355X (tests/golden/block_routes/block_routes.npz).

    python tools/make_block_golden.py [--out tests/golden/block_routes/block_routes.npz] [--force]

The fixture was recorded from the build of commit 54d70d5, the parent of the commit that put one block and layer description
behind the message-passing C-ABI: tests/test_gpu_block_routes_golden.py asserts that every later build gives the same bits.
The block routes write per-workgroup partials and slab rows and sum them in a fixed order, so equality is exact; before
anything is written every case runs twice and an array whose two runs differ is refused by name.  The one exclusion is the
{d dt, d score_scale} pair of gadapt_layer_backward (float atomics; tests/test_gpu_ops.py keeps its tolerance).

Every case goes through the package's own callers - functional.grand_euler_block / grand_residual, training.FusedIteration,
inference.GraphedForward - so their argument lists are pinned too, and sets graph.WIDE_MIN_NODES itself.  CASES, by name:
    tiled{8,32}_shared          11 x 11 b2, L = 3, one shared conv (a_stride = 0, slab accumulated), dense slots
    tiled{8,32}_layers          ... per-layer convs, d layer_params (d dt and d scale) and d x0 wanted
    layer8                      grand_residual: gadapt_layer_forward / gadapt_layer_backward (without d scale: atomics)
    compact32_L3_{inplace,apart} hidden 32, compact x0 (4 columns), compact top gradient (2 columns): the 4-column pair on layer 1
    compact32_L2_learn          L = 2 with d layer_params: the corner that keeps the dense pair
    wide64_dense, wide64_compact hidden 64, row-major 23 x 23 b2 at WIDE_MIN_NODES = 0: the wide forward (four-wave workgroups), dense slots / compact x0
    wide64_compact_8waves       ... with WIDE_HALF_MAX_NODES = 0: the eight-wave geometry
    narrow64_L{4,6}_f{1,2,0}_b{1,0}  the narrow route: forward mode 1 (block launch: one group, groups of 4 + 2), 2, 0; backward fused / pairs
    tiled64_shuffled            hidden 64, shuffled node order (gadapt_narrow_route = 0): the tiled hidden-64 kernels
    h128_rowmajor, h128_shuffled hidden 128: the windowed source pass (wide_deg_s > 0) and the plain one
    fused_small_narrow          FusedIteration, 11 x 11 b2, hidden 64, narrow (packed slab; < 64 workgroups: the coefficient launch first)
    fused_small_tiled           ... without the wide kernels: the tiled compact route, gadapt_step_tail in its three forms
    fused_large_narrow          64 x 64 b8 (32768 nodes, 64 tiles: in-kernel coefficients), gadapt_step_tail_narrow in its two forms
    eval_narrow, eval_tiled     GraphedForward (gadapt_block_forward_loss[_narrow] without a target)
Each fused case records loss / parameters / moments after three steps, the flat gradient of the gradient-only tail and the
parameters / moments after the gradient-given tail.  Arrays of more than FULL_MAX elements are stored as the sha256 of their
bytes beside their shape and dtype.

The fixture has a directory of its own: other tests read every .npz directly under tests/golden as a fixture of theirs.
An existing fixture is not overwritten without --force: re-recording it from a build under test proves nothing.
"""
import argparse
import hashlib
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if os.path.abspath(p) not in sys.path:
        sys.path.insert(0, os.path.abspath(p))

DEFAULT_OUT = os.path.join(ROOT, 'tests', 'golden', 'block_routes', 'block_routes.npz')
TILED = 10 ** 9                       # graph.WIDE_MIN_NODES at which no batch gets the wide kernels
FULL_MAX = 2048                      # elements stored in full; above: a digest


def pack(a):
    """What the fixture stores of one result array: itself, or (sha256 of its bytes | shape | dtype) as a byte string."""
    a = np.ascontiguousarray(a)
    if a.size <= FULL_MAX:
        return a
    tag = f"{hashlib.sha256(a.tobytes()).hexdigest()} {a.shape} {a.dtype}"
    return np.frombuffer(tag.encode(), dtype=np.uint8).copy()


def _layer(C, seed, S, dev):
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / math.sqrt(C)
    r = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) * k).to(dev)
    return [r(S, C, C), r(S, C), r(S, C, C), r(S, C)]


def _mesh_graph(mesh_n, batch, dev, wide_min, shuffle=False, half_max=None):
    """(MeshGraph, n) of a batch of row-major mesh_n x mesh_n meshes, or of the same graph under a node permutation."""
    from g_adaptivity_amd import MeshDataset, MeshGraph, collate
    from g_adaptivity_amd import graph as graph_mod
    from oracle.pyg_restatement import masked_edge_index
    ds = MeshDataset([mesh_n, mesh_n], batch, seed=3)
    ei, n = masked_edge_index(collate(ds.samples), 2, mesh_n), batch * mesh_n * mesh_n
    if shuffle:
        ei = torch.randperm(n, generator=torch.Generator().manual_seed(9))[ei]
    keep = (graph_mod.WIDE_MIN_NODES, graph_mod.WIDE_HALF_MAX_NODES)
    graph_mod.WIDE_MIN_NODES = wide_min
    if half_max is not None:                                           # 0: no four-wave workgroups (gadapt_graph::wide_half_deg_t = 0)
        graph_mod.WIDE_HALF_MAX_NODES = half_max
    try:
        return MeshGraph(ei.contiguous(), n, dev), n
    finally:
        graph_mod.WIDE_MIN_NODES, graph_mod.WIDE_HALF_MAX_NODES = keep


def _block(dev, C, L, mesh_n=11, batch=2, S=1, compact=False, out_cols=None, lp_grad=False, x0_grad=False, narrow=False,
           wide_min=TILED, shuffle=False, expect_narrow=None, fwd_mode=1, bwd_fused=1, inplace=1, half_max=None):
    from g_adaptivity_amd import functional as Fn
    from g_adaptivity_amd._native import lib
    graph, n = _mesh_graph(mesh_n, batch, dev, wide_min, shuffle, half_max)
    if expect_narrow is not None:
        assert bool(graph.narrow_route(C)) == expect_narrow, "the case must (not) be a graph the wide forward takes"
    if narrow and fwd_mode == 1:
        assert graph.narrow_block_halo in (32, 64) and lib().gadapt_narrow_block_halo(graph.c_ref, C) == graph.narrow_block_halo
    gen = torch.Generator().manual_seed(5)
    ps = [t.requires_grad_(True) for t in _layer(C, 31, S, dev)]
    lp = torch.tensor([[0.1 + 0.02 * l, (1.0 + 0.1 * l) / math.sqrt(C)] for l in range(L)], device=dev).requires_grad_(lp_grad)
    tgt = torch.rand(n, out_cols or C, generator=gen).to(dev)
    lib().gadapt_debug_set_narrow_forward(fwd_mode)
    lib().gadapt_debug_set_narrow_backward_fused(bwd_fused)
    lib().gadapt_debug_set_backward_inplace(inplace)
    try:
        if compact:
            feats = torch.rand(n, 4, generator=gen).to(dev)
            x_all = torch.zeros(L + 1, n, C, device=dev)
            x0 = x_all[0].view(-1)[:4 * n].view(n, 4)
            x0.copy_(feats)
            out, alpha = Fn.grand_euler_block(x0, *ps, lp, graph, L, want_alpha=True, x_all=x_all, out_cols=out_cols, x0_cols=4, narrow=narrow)
        else:
            x0 = torch.randn(n, C, generator=gen).to(dev).requires_grad_(x0_grad)
            out, alpha = Fn.grand_euler_block(x0, *ps, lp, graph, L, want_alpha=True, out_cols=out_cols)
        ((out - tgt) ** 2).mean().backward()
        torch.cuda.synchronize()
    finally:
        lib().gadapt_debug_set_narrow_forward(1)
        lib().gadapt_debug_set_narrow_backward_fused(1)
        lib().gadapt_debug_set_backward_inplace(1)
    res = {'out': out.detach(), 'alpha': alpha, 'd_wq': ps[0].grad, 'd_bq': ps[1].grad, 'd_wk': ps[2].grad, 'd_bk': ps[3].grad}
    if lp_grad:
        res['d_lp'] = lp.grad
    if x0_grad:
        res['d_x0'] = x0.grad
    return res


def _layer_case(dev):
    from g_adaptivity_amd import functional as Fn
    C = 8
    graph, n = _mesh_graph(11, 2, dev, TILED)
    wq, bq, wk, bk = [t[0].requires_grad_(True) for t in _layer(C, 17, 1, dev)]
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(n, C, generator=gen).to(dev).requires_grad_(True)
    up = torch.randn(n, C, generator=gen).to(dev)
    scale = torch.tensor(1.0 / math.sqrt(C), device=dev, requires_grad=True)
    res, alpha = Fn.grand_residual(x, wq, bq, wk, bk, scale, graph, want_alpha=True)
    (res * up).sum().backward()
    torch.cuda.synchronize()
    return {'res': res.detach(), 'alpha': alpha, 'd_x': x.grad, 'd_wq': wq.grad, 'd_bq': bq.grad, 'd_wk': wk.grad, 'd_bk': bk.grad}


def _model(dev, mesh_n, batch, wide_min, train, half_max=None):
    """(model, batch) at hidden 64, L = 4; leaves graph.WIDE_MIN_NODES / WIDE_HALF_MAX_NODES set for the caller's graphs (_limits restores)."""
    from g_adaptivity_amd import GNN, MeshDataset, collate, hot_path_opt
    from g_adaptivity_amd import graph as graph_mod
    graph_mod.WIDE_MIN_NODES = wide_min
    if half_max is not None:
        graph_mod.WIDE_HALF_MAX_NODES = half_max
    opt = hot_path_opt(mesh_dims=[mesh_n, mesh_n], hidden_dim=64, num_layers=4, lr=1e-3, device=str(dev), show_mesh_evol_plots='False')
    ds = MeshDataset([mesh_n, mesh_n], batch, seed=11)
    data = collate(ds.samples).to(dev)
    torch.manual_seed(12)
    model = GNN(ds, opt).to(dev)
    return (model.train() if train else model.eval()), data


class _limits:
    """Restores the two graph limits a case sets."""
    def __enter__(self):
        from g_adaptivity_amd import graph as graph_mod
        self.keep = (graph_mod.WIDE_MIN_NODES, graph_mod.WIDE_HALF_MAX_NODES)

    def __exit__(self, *exc):
        from g_adaptivity_amd import graph as graph_mod
        graph_mod.WIDE_MIN_NODES, graph_mod.WIDE_HALF_MAX_NODES = self.keep


def _fused(dev, mesh_n, batch, wide_min, narrow, in_forward):
    """in_forward: no four-wave workgroups (WIDE_HALF_MAX_NODES = 0), so the layer-0 launch may compute the coefficients."""
    from g_adaptivity_amd import mse_loss, unit_gradient
    from g_adaptivity_amd.optim import FlatAdam
    from g_adaptivity_amd.training import FusedIteration
    with _limits():
        model, data = _model(dev, mesh_n, batch, wide_min, True, 0 if in_forward else None)
        optim = FlatAdam(model.parameters(), lr=1e-3, capturable=True)
        optim.zero_grad(); mse_loss(model(data), data.x_phys).backward(gradient=unit_gradient(dev)); optim.step()   # lays the bucket out
        assert FusedIteration.eligible(model, optim, mse_loss, data, 'x_phys') is None
        it = FusedIteration(model, optim, mse_loss, data, 'x_phys')
        assert bool(it.fwd.narrow) == narrow and bool(it.fwd.in_forward) == in_forward, (it.fwd.narrow, it.fwd.in_forward)
        it.refresh_coeffs()
        res = {}
        for step in range(3):
            it.run()
            res[f'loss{step}'] = it.loss.clone()
        torch.cuda.synchronize()
        res.update(out=it.out.clone(), param=optim.bucket.clone(), exp_avg=optim.exp_avg.clone(), exp_avg_sq=optim.exp_avg_sq.clone(),
                   a=it.coeffs[0].clone(), p0=it.coeffs[1].clone())
        it.forward_backward()                                           # the data-parallel order on one GPU: gradient only, then gradient given
        it.flat.fill_(float('nan'))
        it._tail(stop_after_gradient=True)
        res.update(flat=it.flat.clone(), loss_gradient_only=it.loss.clone())
        it._tail(gradient_given=True)
        torch.cuda.synchronize()
        res.update(param_given=optim.bucket.clone(), exp_avg_given=optim.exp_avg.clone(), exp_avg_sq_given=optim.exp_avg_sq.clone())
        return res


def _eval(dev, wide_min, narrow):
    from g_adaptivity_amd.inference import GraphedForward
    with _limits():
        model, data = _model(dev, 11, 2, wide_min, False)
        gf = GraphedForward(model, data)
        assert gf.issued and bool(gf._call.narrow) == narrow
        return {'out': gf(data).clone()}


def cases(dev):
    """name -> thunk returning a dict of tensors."""
    out = {}
    for C in (8, 32):
        out[f'tiled{C}_shared'] = lambda C=C: _block(dev, C, 3)
        out[f'tiled{C}_layers'] = lambda C=C: _block(dev, C, 3, S=3, lp_grad=True, x0_grad=True)
    out['layer8'] = lambda: _layer_case(dev)
    out['compact32_L3_inplace'] = lambda: _block(dev, 32, 3, compact=True, out_cols=2, inplace=1)
    out['compact32_L3_apart'] = lambda: _block(dev, 32, 3, compact=True, out_cols=2, inplace=0)
    out['compact32_L2_learn'] = lambda: _block(dev, 32, 2, compact=True, out_cols=2, lp_grad=True)
    wide = dict(mesh_n=23, batch=2, wide_min=0, expect_narrow=True)
    out['wide64_dense'] = lambda: _block(dev, 64, 3, **wide)
    out['wide64_compact'] = lambda: _block(dev, 64, 3, compact=True, out_cols=2, **wide)
    out['wide64_compact_8waves'] = lambda: _block(dev, 64, 3, compact=True, out_cols=2, half_max=0, **wide)
    for L in (4, 6):
        for fm, bf in ((1, 1), (2, 0), (0, 1)):
            out[f'narrow64_L{L}_f{fm}_b{bf}'] = lambda L=L, fm=fm, bf=bf: _block(dev, 64, L, compact=True, out_cols=2, narrow=True, fwd_mode=fm,
                                                                                 bwd_fused=bf, **wide)
    out['tiled64_shuffled'] = lambda: _block(dev, 64, 3, mesh_n=23, batch=2, wide_min=0, shuffle=True, expect_narrow=False, compact=True, out_cols=2)
    out['h128_rowmajor'] = lambda: _block(dev, 128, 2, mesh_n=23, batch=2, wide_min=0)
    out['h128_shuffled'] = lambda: _block(dev, 128, 2, mesh_n=23, batch=2, wide_min=0, shuffle=True)
    out['fused_small_narrow'] = lambda: _fused(dev, 11, 2, 0, True, True)
    out['fused_small_tiled'] = lambda: _fused(dev, 11, 2, TILED, False, False)
    out['fused_large_narrow'] = lambda: _fused(dev, 64, 8, 0, True, True)
    out['eval_narrow'] = lambda: _eval(dev, 0, True)
    out['eval_tiled'] = lambda: _eval(dev, TILED, False)
    return out


def compute(dev, only=None):
    """Every recorded result as a dict of numpy arrays named '<case>.<what>', packed as the fixture stores them."""
    res = {}
    for name, thunk in cases(dev).items():
        if only is not None and name not in only:
            continue
        for k, v in thunk().items():
            res[f'{name}.{k}'] = pack(v.detach().cpu().numpy())
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=DEFAULT_OUT)
    ap.add_argument('--force', action='store_true', help='overwrite an existing fixture')
    args = ap.parse_args()
    if os.path.exists(args.out) and not args.force:
        sys.exit(f"{os.path.normpath(args.out)} exists; --force overwrites it (only from a build that is not under test)")
    assert torch.cuda.is_available(), "the fixture is recorded on the MI355X"
    dev = torch.device('cuda:0')
    first, second = compute(dev), compute(dev)
    unstable = [k for k in first if not np.array_equal(first[k], second[k], equal_nan=True)]
    if unstable:
        sys.exit("two runs differ, nothing stored: " + ', '.join(unstable))
    for k, v in first.items():
        assert v.dtype == np.uint8 or np.isfinite(v).all(), k
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **first)
    print(f"{len(first)} arrays, {os.path.getsize(args.out)} bytes -> {os.path.normpath(args.out)}")
    for k in sorted(first):
        print(f"  {k:44s} {first[k].shape!s:14s} {first[k].dtype}")


if __name__ == '__main__':
    main()
