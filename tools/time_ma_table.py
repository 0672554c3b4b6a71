"""Kernel time of 1 000 Monge-Ampere updates with a tabulated monitor beside the analytic monitor, same library, same session
(docs/measurements.md, "Monge-Ampere meshes from a tabulated monitor").

Device events around the one launch alone (`monge_ampere._prepare` / `_prepare_table` give the launch closure), WINDOWS timed
launches after WARMUP untimed ones, median with min - max.  tol = 0, two drawn Gaussians per mesh with mon_reg = 0.01,
mon_power = 0.2; the table is `monitor_table` of the same Gaussians, T = N and T = 101.  Candidate pairs that do not run their
1 000 updates under all three are dropped before timing; the kept ones are cycled over the batch.

    python tools/time_ma_table.py            # prints a markdown table
"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g_adaptivity_amd import monge_ampere as ma  # noqa: E402

UPDATES, WARMUP, WINDOWS, CANDIDATES = 1000, 3, 11, 32
REG = {'mon_reg': 0.01, 'mon_power': 0.2}
PLAN = [('lane', 11, 1024), ('lane', 23, 1024), ('lane', 32, 1024), ('strided', 32, 256), ('strided', 33, 256), ('strided', 64, 256),
        ('strided', 81, 256)]


def drawn(seed, count=2):
    rng = np.random.default_rng(seed)
    centers = [rng.uniform(0.0, 1.0, 2).astype('f') for _ in range(count)]
    scales = [rng.uniform(0.1, 0.5, 2).astype('f') for _ in range(count)]
    return dict({'centers': centers, 'scales': scales}, **REG)


def timed(launch):
    for _ in range(WARMUP):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def fmt(t):
    return f"{t[0]:.3f} ms ({t[1]:.3f} - {t[2]:.3f})"


def main():
    kw = dict(tol=0.0, max_steps=UPDATES)
    print("| route | side | meshes | `ma` | table, T = N | table, T = 101 | T = N / ma | T = 101 / ma |")
    print("|---|---|---|---|---|---|---|---|")
    for route, n, many in PLAN:
        cand = [drawn(5000 + 100 * n + k) for k in range(CANDIDATES)]
        tabs = {T: [ma.monitor_table(p, T) for p in cand] for T in (n, 101)}
        ok = torch.ones(CANDIDATES, dtype=torch.bool)
        for res in [ma.ma_batch([n] * CANDIDATES, cand, route=route, **kw)] + \
                   [ma.ma_table_batch([n] * CANDIDATES, tabs[T], route=route, **kw) for T in tabs]:
            ok &= (res.steps.cpu() == UPDATES) & (res.status.cpu() == ma.CAP)
        keep = [k for k in range(CANDIDATES) if ok[k]]
        assert keep, (route, n)
        for B in (1, many):
            pick = [keep[b % len(keep)] for b in range(B)]
            launch_a, collect_a = ma._prepare([n] * B, [cand[k] for k in pick], route=route, **kw)
            t_a = timed(launch_a)
            t_t = {}
            for T in tabs:
                launch_t, collect_t = ma._prepare_table([n] * B, [tabs[T][k] for k in pick], route=route, **kw)
                t_t[T] = timed(launch_t)
                assert collect_t().steps.tolist() == [UPDATES] * B
            assert collect_a().steps.tolist() == [UPDATES] * B
            print(f"| {route} | {n} | {B} | {fmt(t_a)} | {fmt(t_t[n])} | {fmt(t_t[101])} | {t_t[n][0] / t_a[0]:.2f} | "
                  f"{t_t[101][0] / t_a[0]:.2f} |", flush=True)
        print(f"<!-- {route} {n}: {len(keep)} of {CANDIDATES} candidate pairs kept -->", flush=True)


if __name__ == '__main__':
    main()
