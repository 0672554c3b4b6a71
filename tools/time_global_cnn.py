"""Time of the global CNN features, kernel='torch' (the Conv modules: MIOpen and ATen launches) beside kernel='hip' (one launch
forward, one backward: csrc/gadapt_cnn.inc), same weights, same session (docs/measurements.md, "Global CNN features in HIP").

(a) The extractor alone: forward under no_grad, and forward + backward (gradients accumulate into .grad in both arms, the seed
    d feat fixed), at the shapes SHAPES x batch 1 and 32.  Once as eager calls - the time is the host's issue rate where that is the
    slower side, which is what a caller outside a captured graph pays - and once captured in a hipGraph and replayed: the device's
    own time.
(b) The `GraphedTrainStep` step (forward, loss, backward, Adam in one replayed hipGraph: no host issue) of the reference's own model
    size with both extractors on, both ways.

Protocol: device events around CALLS back-to-back calls, WINDOWS such windows per arm after WARMUP untimed calls; the two arms
alternate window by window in one process; median per call with min - max of the windows.

    python tools/time_global_cnn.py            # prints markdown tables
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g_adaptivity_amd import GNN, DeviceMeshLoader, GraphedTrainStep, MeshDataset, hot_path_opt  # noqa: E402
from g_adaptivity_amd.features import GlobalFeatureExtractorCNN  # noqa: E402
from g_adaptivity_amd.optim import FlatAdam  # noqa: E402

WARMUP, WINDOWS, CALLS = 20, 9, 50
SHAPES = [('11 x 11, hidden 8', 2, (11, 11), 8), ('23 x 23, hidden 8', 2, (23, 23), 8), ('15 x 15, hidden 16', 2, (15, 15), 16),
          ('1-D 21 nodes, hidden 16', 1, (21,), 16)]
BATCHES = (1, 32)


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / CALLS                       # microseconds per call


def alternate(arms):
    """{name: fn} -> {name: (median, min, max)} in microseconds per call; the arms take turns window by window."""
    for fn in arms.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in arms}
    for _ in range(WINDOWS):
        for k, fn in arms.items():
            us[k].append(window(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in us.items()}


def captured(fn):
    """fn captured in a hipGraph after a warm-up on a side stream; returns the replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def fmt(t):
    return f"{t[0]:.1f} ({t[1]:.1f} - {t[2]:.1f})"


def extractor_arms(dim, shape, hidden, batch, dev):
    torch.manual_seed(0)
    mods = {k: GlobalFeatureExtractorCNN(1, hidden, 8, dim=dim, kernel=k).to(dev) for k in ('torch', 'hip')}
    mods['hip'].load_state_dict(mods['torch'].state_dict())
    u = torch.randn(batch, 1, *shape, device=dev)
    seed = torch.randn(batch, 8, device=dev)
    fwd, both = {}, {}
    for k, m in mods.items():
        def forward(m=m):
            with torch.no_grad():
                return m(u)

        def train(m=m):
            m(u).backward(seed)
        fwd[k], both[k] = forward, train
    err = (mods['hip'](u) - mods['torch'](u)).abs().max().item() / mods['torch'](u).abs().max().item()
    assert err < 1e-5, err                                       # the two arms compute the same thing
    return fwd, both


def graphed_arms(dev, batch):
    arms, keep = {}, []
    for kernel in ('torch', 'hip'):
        opt = hot_path_opt(mesh_dims=[11, 11], hidden_dim=8, gnn_inc_glob_feat_f=True, gnn_inc_glob_feat_uu=True, glob_feat_kernel=kernel,
                           device=str(dev))
        ds = MeshDataset([11, 11], batch, seed=0)
        torch.manual_seed(0)
        m = GNN(ds, opt).to(dev).train()
        step = GraphedTrainStep(m, FlatAdam(m.parameters(), lr=opt['lr'], capturable=True))
        d = next(iter(DeviceMeshLoader(ds, batch_size=batch, shuffle=False, device=dev)))
        keep.append((m, ds, d))
        arms[kernel] = lambda step=step, d=d: step(d)
    return arms, keep


def main():
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device('cuda:0')
    for mode in ('eager', 'replayed'):
        print(f"| extractor, {mode} | batch | forward, torch [us] | forward, hip [us] | torch / hip | forward + backward, torch [us] | "
              "forward + backward, hip [us] | torch / hip |")
        print("|---|---|---|---|---|---|---|---|")
        for label, dim, shape, hidden in SHAPES:
            for batch in BATCHES:
                fwd, both = extractor_arms(dim, shape, hidden, batch, dev)
                if mode == 'replayed':
                    fwd, both = {k: captured(fn) for k, fn in fwd.items()}, {k: captured(fn) for k, fn in both.items()}
                f, t = alternate(fwd), alternate(both)
                print(f"| {label} | {batch} | {fmt(f['torch'])} | {fmt(f['hip'])} | {f['torch'][0] / f['hip'][0]:.2f} | {fmt(t['torch'])} | "
                      f"{fmt(t['hip'])} | {t['torch'][0] / t['hip'][0]:.2f} |", flush=True)
        print()
    print("| `GraphedTrainStep` step, 11 x 11, hidden 8, both extractors | batch | torch [us] | hip [us] | torch / hip |")
    print("|---|---|---|---|---|")
    for batch in BATCHES:
        arms, keep = graphed_arms(dev, batch)
        g = alternate(arms)
        print(f"| replayed step | {batch} | {fmt(g['torch'])} | {fmt(g['hip'])} | {g['torch'][0] / g['hip'][0]:.2f} |", flush=True)


if __name__ == '__main__':
    main()
