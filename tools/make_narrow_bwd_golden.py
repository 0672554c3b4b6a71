"""Golden data of the one-node-per-lane backward target passes, recorded on the MI355X (tests/golden/narrow_bwd/narrow_bwd.npz).

    GADAPT_LIB=<library of the commit to record from> python tools/make_narrow_bwd_golden.py [--out ...] [--force]

The fixture was recorded from the library of commit e8a08c0, the parent of the commit that moved the wave sums of the slab partials
(`bwd_target_compact_body`, the TOP pass of `wide::fwd_narrow_block_kernel`) from the LDS crossbar to DPP / lane-swap steps:
tests/test_gpu_narrow_bwd_golden.py asserts that every later build gives the same bits.  It reaches what
tests/golden/block_routes does not: workgroups with one partial wave, exactly one full workgroup, a second workgroup of 33 nodes,
slab rows without nodes, the ragged / self-looped / mixed / windowed / 1-D graphs of tests/narrow_graphs.py, each with the top
layer's target pass inside the forward launch and as a launch of its own, and the SUMS = 1 / 2 forms of the compact layer-0 kernel.

CASES, by name:
    sq{5,16,17}_b1, sq23_b7, sq32_b3   C-ABI level (the harness of tests/test_gpu_narrow_top_in_forward.py), hidden 64, 4 layers, packed slab
    ng_<id>                            ... every graph of tests/narrow_graphs.py
    learn32_sums{1,2}                  functional.grand_euler_block, hidden 32, 3 layers, compact x0, 11 x 11 b2: d dt alone (learn_step:
                                       SUMS = 1) and d dt with d score_scale (SUMS = 2), both through the per-workgroup partials (the
                                       atomic path of gadapt_layer_backward stays excluded, as in tests/golden/block_routes)
Per narrow case and switch position (`in_fwd`: gadapt_debug_set_narrow_top_in_forward(1), `apart`: 0): whether the pass ran in the
forward and, if so, the dxd rows, pairs and slab it left; after the backward call every row of the packed slab (rows without nodes
included), the dxd rows, both edge buffers and both gradient work buffers; after the gradient-only tail the flat gradient.  Buffers
are poisoned with NaN before every call and stored as their int32 bit patterns, so what no launch writes is pinned too.  Arrays of
more than FULL_MAX elements are stored as the sha256 of their bytes beside their shape and dtype.  Every case runs twice and an
array whose two runs differ is left out by name (the test then has nothing to compare it with).
"""
import argparse
import contextlib
import hashlib
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if os.path.abspath(p) not in sys.path:
        sys.path.insert(0, os.path.abspath(p))

DEFAULT_OUT = os.path.join(ROOT, 'tests', 'golden', 'narrow_bwd', 'narrow_bwd.npz')
FULL_MAX = 512                       # elements stored in full; above: a digest
C_ = 64
SQUARES = [(5, 1), (16, 1), (17, 1), (23, 7), (32, 3)]


def pack(a):
    a = np.ascontiguousarray(a)
    if a.size <= FULL_MAX:
        return a
    tag = f"{hashlib.sha256(a.tobytes()).hexdigest()} {a.shape} {a.dtype}"
    return np.frombuffer(tag.encode(), dtype=np.uint8).copy()


def bits(t):
    t = t.detach().contiguous()
    return (t.view(torch.int32) if t.dtype == torch.float32 else t).cpu().numpy()


@contextlib.contextmanager
def _patched(half_max=None):
    """The wide kernels for every batch size, no one-launch small-mesh pair (what the narrow tests patch)."""
    import g_adaptivity_amd.functional as Fn_mod
    from g_adaptivity_amd import graph as graph_mod
    keep = (Fn_mod.SMALL_MESH_FORWARD, graph_mod.WIDE_MIN_NODES, graph_mod.WIDE_HALF_MAX_NODES)
    Fn_mod.SMALL_MESH_FORWARD, graph_mod.WIDE_MIN_NODES = False, 0
    if half_max is not None:
        graph_mod.WIDE_HALF_MAX_NODES = half_max
    try:
        yield
    finally:
        Fn_mod.SMALL_MESH_FORWARD, graph_mod.WIDE_MIN_NODES, graph_mod.WIDE_HALF_MAX_NODES = keep


def _flat_gradient(h, model, slab, n_part):
    """The flat gradient [dWq | dbq | dWk | dbk] of gadapt_step_tail_narrow's gradient-only form on `slab`."""
    from g_adaptivity_amd._native import current_stream, lib, ptr
    from test_gpu_narrow_tail import ROW
    cv = model.conv_layers[0]
    bucket = torch.cat([cv.lin_query.weight.reshape(-1), cv.lin_query.bias, cv.lin_key.weight.reshape(-1), cv.lin_key.bias]).detach().contiguous()
    f32 = dict(device=h.dev, dtype=torch.float32)
    flat, scratch, loss = torch.full((2 * C_ * C_ + 2 * C_,), float('nan'), **f32), torch.empty(32 * ROW, **f32), torch.zeros((), **f32)
    state = torch.zeros(2, device=h.dev, dtype=torch.int32)
    args = [ptr(slab), h.rows, ptr(scratch), ptr(bucket), ptr(flat), None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, ptr(state), 1.0, None, None,
            ptr(h.fwd.partials), n_part, ptr(loss), h.n * h.d, C_, current_stream(h.dev)]
    assert lib().gadapt_step_tail_narrow(*args) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(flat).any() and flat.abs().max().item() > 0
    return flat, loss


def _narrow(h, model):
    n, e = h.n, h.e
    res = {}
    for tag, on in (('in_fwd', 1), ('apart', 0)):
        s = h.run(on, steps=1)[0]
        res[f'{tag}.ran'] = torch.tensor([int(s['ran'])], dtype=torch.int32)
        if s['ran']:
            res[f'{tag}.f_dxd'], res[f'{tag}.f_pairs'], res[f'{tag}.f_slab'] = s['f_dxd'], s['f_pairs'], s['f_slab']
        res[f'{tag}.slab'] = s['b_slab']
        res[f'{tag}.dxd'] = s['b_dxd'].view(-1)[:4 * n]
        res[f'{tag}.pairs0'] = s['b_edge'].view(-1)[:2 * e]
        res[f'{tag}.pairs1'] = s['b_dxd'].view(-1)[4 * n:4 * n + 2 * e]
        res[f'{tag}.g'] = s['b_g']
        res[f'{tag}.flat'], res[f'{tag}.loss'] = _flat_gradient(h, model, s['b_slab'].clone(), s['n_part'])
    return res


def _square(dev, mesh_n, batch):
    import test_gpu_narrow_top_in_forward as T
    from g_adaptivity_amd import GNN, MeshDataset, collate, hot_path_opt
    with _patched():
        opt = hot_path_opt(mesh_dims=[mesh_n, mesh_n], hidden_dim=64, num_layers=4, lr=1e-3, device=str(dev), show_mesh_evol_plots='False')
        ds = MeshDataset([mesh_n, mesh_n], batch, seed=11)
        data = collate(ds.samples).to(dev)
        torch.manual_seed(12)
        model = GNN(ds, opt).to(dev).train()
        h = T.Harness(model, data)
        assert h.n == batch * mesh_n * mesh_n
        return _narrow(h, model)


def _graph_case(dev, case_id):
    import narrow_graphs as ng
    import test_gpu_narrow_top_in_forward as T
    from helpers import hip_model_like
    b = ng.build(case_id)
    with _patched(b.case.half_max):
        model = hip_model_like(b.oracle, b.ds, b.opt, dev).train()
        data = b.data.clone().to(dev)                                     # (the harness keeps addresses of its fields: alive until the end)
        h = T.Harness(model, data)
        assert h.n == b.case.nodes
        return _narrow(h, model)


def _learn32(dev, sums):
    """hidden 32, compact x0, 3 layers: layer 0 runs grand_bwd_target_compact_kernel<sums> and writes one partial per workgroup."""
    import make_block_golden as B
    from g_adaptivity_amd import functional as Fn
    C, L = 32, 3
    graph, n = B._mesh_graph(11, 2, dev, B.TILED)
    gen = torch.Generator().manual_seed(5)
    ps = [t.requires_grad_(True) for t in B._layer(C, 31, 1, dev)]
    dts = [0.1 + 0.02 * l for l in range(L)]
    scales = [(1.0 + 0.1 * l) / math.sqrt(C) for l in range(L)]
    tgt = torch.rand(n, 2, generator=gen).to(dev)
    feats = torch.rand(n, 4, generator=gen).to(dev)
    x_all = torch.zeros(L + 1, n, C, device=dev)
    x0 = x_all[0].view(-1)[:4 * n].view(n, 4)
    x0.copy_(feats)
    if sums == 1:                                                          # learn_step: the steps are parameters, the scales are not
        steps = [torch.tensor([v], device=dev, requires_grad=True) for v in dts]
        lp = torch.tensor(scales, device=dev)
        out, _ = Fn.grand_euler_block(x0, *ps, lp, graph, L, want_alpha=True, x_all=x_all, out_cols=2, x0_cols=4, steps=steps)
    else:
        steps = None
        lp = torch.tensor(list(zip(dts, scales)), device=dev).requires_grad_(True)
        out, _ = Fn.grand_euler_block(x0, *ps, lp, graph, L, want_alpha=True, x_all=x_all, out_cols=2, x0_cols=4)
    ((out - tgt) ** 2).mean().backward()
    torch.cuda.synchronize()
    res = {'out': out.detach(), 'd_wq': ps[0].grad, 'd_bq': ps[1].grad, 'd_wk': ps[2].grad, 'd_bk': ps[3].grad}
    if sums == 1:
        res['d_steps'] = torch.cat([s.grad.reshape(1) for s in steps])
    else:
        res['d_lp'] = lp.grad
    return res


def cases(dev):
    """name -> thunk returning a dict of tensors."""
    import narrow_graphs as ng
    out = {}
    for mesh_n, batch in SQUARES:
        out[f'sq{mesh_n}_b{batch}'] = lambda m=mesh_n, b=batch: _square(dev, m, b)
    for cid in ng.IDS:
        out[f'ng_{cid}'] = lambda cid=cid: _graph_case(dev, cid)
    out['learn32_sums1'] = lambda: _learn32(dev, 1)
    out['learn32_sums2'] = lambda: _learn32(dev, 2)
    return out


def compute(dev, only=None):
    """Every recorded result as a dict of numpy arrays named '<case>.<what>', packed as the fixture stores them."""
    res = {}
    for name, thunk in cases(dev).items():
        if only is not None and name not in only:
            continue
        for k, v in thunk().items():
            res[f'{name}.{k}'] = pack(bits(v))
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
    unstable = [k for k in first if not np.array_equal(first[k], second[k])]
    for k in unstable:
        print(f"two runs differ, left out: {k}")
        del first[k]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **first)
    print(f"{len(first)} arrays, {os.path.getsize(args.out)} bytes -> {os.path.normpath(args.out)}")
    for k in sorted(first):
        print(f"  {k:44s} {first[k].shape!s:14s} {first[k].dtype}")


if __name__ == '__main__':
    main()
