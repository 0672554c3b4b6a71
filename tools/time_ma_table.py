"""Kernel time of 1 000 Monge-Ampere updates on all seven kernels, same library, same session: the analytic monitor, the M2N
'fast' monitor and a tabulated monitor on both routes, and the M2N 'slow' monitor on the lane route (docs/measurements.md,
"Monge-Ampere meshes from a tabulated monitor" and "The shared iteration stated once: kernel time against the parent").

Device events around the one launch alone (`monge_ampere._prepare` / `_prepare_table` give the launch closure), WINDOWS timed
launches after WARMUP untimed ones, median with min - max.  tol = 0, two drawn Gaussians per mesh with mon_reg = 0.01,
mon_power = 0.2 (`ma`), mon_reg = 0.1, beta = 1.5 (M2N 'fast') and alpha = 1 beside them ('slow'); the table is `monitor_table`
of the `ma` monitor, T = N and T = 101.  Candidate pairs that do not run their 1 000 updates under every monitor of the row are
dropped before timing; the kept ones are cycled over the batch.

    python tools/time_ma_table.py [--json FILE]     # prints a markdown table; FILE gets {row: {column: [median, min, max]}}
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g_adaptivity_amd import monge_ampere as ma  # noqa: E402

UPDATES, WARMUP, WINDOWS, CANDIDATES, MANY = 1000, 3, 11, 32, 256
REG = {'mon_reg': 0.01, 'mon_power': 0.2}
M2N = {'mesh_type': 'M2N', 'fast_M2N_monitor': 'fast', 'mon_reg': 0.1, 'M2N_beta': 1.5}
SLOW = {'mesh_type': 'M2N', 'fast_M2N_monitor': 'slow', 'mon_reg': 0.1, 'M2N_alpha': 1.0, 'M2N_beta': 1.5}
PLAN = [('lane', 11), ('lane', 32), ('strided', 33), ('strided', 81)]
SLOW_PLAN = [11, 24]                                                     # lane route only, up to 24 a side


def drawn(seed, count=2):
    rng = np.random.default_rng(seed)
    centers = [rng.uniform(0.0, 1.0, 2).astype('f') for _ in range(count)]
    scales = [rng.uniform(0.1, 0.5, 2).astype('f') for _ in range(count)]
    return {'centers': centers, 'scales': scales}


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


def kept(results):
    ok = torch.ones(CANDIDATES, dtype=torch.bool)
    for res in results:
        ok &= (res.steps.cpu() == UPDATES) & (res.status.cpu() == ma.CAP)
    keep = [k for k in range(CANDIDATES) if ok[k]]
    assert keep
    return keep


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--json', default=None, help='also write the figures to this file')
    args = ap.parse_args()
    kw = dict(tol=0.0, max_steps=UPDATES)
    out = {}
    print("| route | side | meshes | `ma` | M2N 'fast' | table, T = N | table, T = 101 | T = N / ma | T = 101 / ma |")
    print("|---|---|---|---|---|---|---|---|---|")
    for route, n in PLAN:
        cand = [drawn(5000 + 100 * n + k) for k in range(CANDIDATES)]
        tabs = {T: [ma.monitor_table(dict(p, **REG), T) for p in cand] for T in (n, 101)}
        keep = kept([ma.ma_batch([n] * CANDIDATES, [dict(p, **mon) for p in cand], route=route, **kw) for mon in (REG, M2N)] +
                    [ma.ma_table_batch([n] * CANDIDATES, tabs[T], route=route, **kw) for T in tabs])
        for B in (1, MANY):
            pick = [keep[b % len(keep)] for b in range(B)]
            t = {}
            for name, mon in (('ma', REG), ('m2n', M2N)):
                launch, collect = ma._prepare([n] * B, [dict(cand[k], **mon) for k in pick], route=route, **kw)
                t[name] = timed(launch)
                assert collect().steps.tolist() == [UPDATES] * B
            for T in tabs:
                launch, collect = ma._prepare_table([n] * B, [tabs[T][k] for k in pick], route=route, **kw)
                t['table_N' if T == n else 'table_101'] = timed(launch)
                assert collect().steps.tolist() == [UPDATES] * B
            out[f'{route} {n} x{B}'] = t
            print(f"| {route} | {n} | {B} | {fmt(t['ma'])} | {fmt(t['m2n'])} | {fmt(t['table_N'])} | {fmt(t['table_101'])} | "
                  f"{t['table_N'][0] / t['ma'][0]:.2f} | {t['table_101'][0] / t['ma'][0]:.2f} |", flush=True)
        print(f"<!-- {route} {n}: {len(keep)} of {CANDIDATES} candidate pairs kept -->", flush=True)
    print("\n| side | meshes | M2N 'slow' |\n|---|---|---|")
    for n in SLOW_PLAN:
        cand = [dict(drawn(5000 + 100 * n + k), **SLOW) for k in range(CANDIDATES)]
        keep = kept([ma.ma_batch([n] * CANDIDATES, cand, m2n_solve='p1', **kw)])
        for B in (1, MANY):
            launch, collect = ma._prepare([n] * B, [cand[keep[b % len(keep)]] for b in range(B)], m2n_solve='p1', **kw)
            t = timed(launch)
            assert collect().steps.tolist() == [UPDATES] * B
            out[f'slow {n} x{B}'] = {'slow': t}
            print(f"| {n} | {B} | {fmt(t)} |", flush=True)
        print(f"<!-- slow {n}: {len(keep)} of {CANDIDATES} candidate pairs kept -->", flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
