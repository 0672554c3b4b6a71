"""cubic_spline_1d on the MI355X against the fp64 test-side restatement (tests/spline_restatement.py, itself pinned to scipy
by tests/test_spline_host.py).  Sizes are where the kernel can go wrong: the smallest systems, around a wave, the workload's
101, the cap; uniform and 100:1 graded abscissae; both query modes; queries on knots, on the ends and slightly outside.

Bound (the project's rule): err <= max(FLOOR[deriv], 1.5 * noise), err and noise relative to the largest reference value of
the case, noise the fp32 run of the same restatement against its fp64 twin.  The kernel works in fp64 and rounds its output
to fp32, so its error is one fp32 rounding of the value; FLOOR is one decade above the worst case measured on the MI355X
over these cases (docs/measurements.md, "Spline kernel")."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spline_restatement as S  # noqa: E402

from g_adaptivity_amd import cubic_spline_1d  # noqa: E402
from g_adaptivity_amd.spline import SPLINE_NOT_FINITE, SPLINE_NOT_INCREASING, SPLINE_OK  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]

# worst measured over the cases of this file on the MI355X: 5.74e-8 (deriv 0), 5.73e-8 (deriv 1), 5.73e-8 (deriv 2): half an
# fp32 ulp of the value, the rounding of the fp64 result; one decade above
FLOOR = {0: 5.8e-7, 1: 5.8e-7, 2: 5.8e-7}
SIZES = [4, 5, 6, 63, 64, 65, 101, 1024]


def abscissae(n, kind):
    if kind == 'uniform':
        return torch.linspace(0, 1, n)
    h = 100.0 ** (np.arange(n - 1) / max(n - 2, 1))               # spacing grows 100-fold from the first interval to the last
    x = np.concatenate([[0.0], np.cumsum(h)])
    return torch.from_numpy((x / x[-1]).astype(np.float32))


def ordinates(x):
    return (0.25 * torch.exp(-(x - 0.45) ** 2 / 0.02) + 0.1 * torch.sin(7 * x)).float()


_REF = {}


def reference(x, y):
    """(M64, M32) of a data set, computed once per set and shared."""
    key = (x.numpy().tobytes(), y.numpy().tobytes())
    if key not in _REF:
        _REF[key] = (S.second_derivatives(x, y, torch.float64), S.second_derivatives(x, y, torch.float32))
    return _REF[key]


def err_and_noise(got, x, y, q, deriv):
    M64, M32 = reference(x, y)
    r64 = S.spline(x, y, q, deriv, torch.float64, M64)
    r32 = S.spline(x, y, q, deriv, torch.float32, M32).double()
    scale = r64.abs().max().clamp_min(1e-30)
    return float((got.double().cpu() - r64).abs().max() / scale), float((r32 - r64).abs().max() / scale)


def check(got, x, y, q, deriv, label):
    err, noise = err_and_noise(got, x, y, q, deriv)
    print(f"spline {label} deriv {deriv}: err {err:.3e} noise {noise:.3e}")
    assert err <= max(FLOOR[deriv], 1.5 * noise), (label, deriv, err, noise)


def lattice(x, Q):
    lo, hi = float(x[0]), float(x[-1])
    if Q == 1:
        return torch.tensor([0.5 * (lo + hi)])
    return torch.linspace(lo - 0.01, hi + 0.01, Q)                 # reaches slightly outside the data on both sides


@pytest.mark.parametrize('kind', ['uniform', 'graded'])
@pytest.mark.parametrize('n', SIZES)
def test_shared_queries_against_restatement(gpu_device, n, kind):
    x = abscissae(n, kind)
    y = ordinates(x)
    xd, yd = x.to(gpu_device), y.to(gpu_device)
    for Q in (1, 41, 101):
        q = lattice(x, Q)
        for deriv in (0, 1, 2):
            v, st = cubic_spline_1d(xd, yd, [n], q.to(gpu_device), deriv=deriv)
            assert v.shape == (1, Q) and st.tolist() == [SPLINE_OK]
            check(v[0], x, y, q, deriv, f"n={n} {kind} Q={Q}")


def _own_queries(x):
    """Every knot (the ends among them), points slightly outside, and the interval midpoints."""
    return torch.cat([x, torch.tensor([float(x[0]) - 0.005, float(x[-1]) + 0.005]), 0.5 * (x[1:] + x[:-1])])


@pytest.mark.parametrize('kind', ['uniform', 'graded'])
def test_mixed_launch_with_per_set_queries(gpu_device, kind):
    sizes = [4, 21, 65, 1024]
    xs = [abscissae(n, kind) for n in sizes]
    ys = [ordinates(x) for x in xs]
    qs = [_own_queries(x) for x in xs]
    X, Y, Qc = (torch.cat(t).to(gpu_device) for t in (xs, ys, qs))
    for deriv in (0, 1, 2):
        v, st = cubic_spline_1d(X, Y, sizes, Qc, q_counts=[q.numel() for q in qs], deriv=deriv)
        assert st.tolist() == [SPLINE_OK] * 4 and v.shape == Qc.shape
        for x, y, q, got in zip(xs, ys, qs, torch.split(v, [q.numel() for q in qs])):
            check(got, x, y, q, deriv, f"mixed n={x.numel()} {kind}")
            if deriv == 0:                                       # at the data points the spline returns y, to fp32 rounding
                n = x.numel()
                assert torch.equal(got[:n - 1].cpu(), y[:n - 1])            # t = 0: exactly
                assert abs(float(got[n - 1]) - float(y[n - 1])) <= 2 ** -23 * abs(float(y[n - 1]))   # x[n-1]: t = h, one ulp
    # the same sets with one shared lattice: [B, Q]
    q = torch.linspace(-0.01, 1.01, 41)
    v, st = cubic_spline_1d(X, Y, sizes, q.to(gpu_device), deriv=2)
    assert v.shape == (4, 41)
    for b, (x, y) in enumerate(zip(xs, ys)):
        check(v[b], x, y, q, 2, f"mixed shared n={x.numel()} {kind}")


@pytest.mark.parametrize('shared', [True, False])
def test_flagged_sets_are_nan_and_leave_the_others_alone(gpu_device, shared):
    sizes = [21, 65, 4, 101]
    xs = [abscissae(n, 'graded' if i % 2 else 'uniform') for i, n in enumerate(sizes)]
    ys = [ordinates(x) for x in xs]
    xs[1] = xs[1].clone(); xs[1][30] = xs[1][29]                  # two equal abscissae
    ys[3] = ys[3].clone(); ys[3][50] = float('nan')               # a NaN ordinate
    good = [0, 2]

    def run(idx):
        X, Y = (torch.cat([t[i] for i in idx]).to(gpu_device) for t in (xs, ys))
        cnt = [sizes[i] for i in idx]
        if shared:
            return cubic_spline_1d(X, Y, cnt, torch.linspace(-0.01, 1.01, 41).to(gpu_device), deriv=2)
        qs = [_own_queries(abscissae(sizes[i], 'uniform')) for i in idx]
        v, st = cubic_spline_1d(X, Y, cnt, torch.cat(qs).to(gpu_device), q_counts=[q.numel() for q in qs], deriv=0)
        return list(torch.split(v, [q.numel() for q in qs])), st

    v_all, st_all = run([0, 1, 2, 3])
    v_good, st_good = run(good)
    torch.cuda.synchronize()
    assert st_all.tolist() == [SPLINE_OK, SPLINE_NOT_INCREASING, SPLINE_OK, SPLINE_NOT_FINITE] and st_good.tolist() == [SPLINE_OK] * 2
    assert torch.isnan(v_all[1]).all() and torch.isnan(v_all[3]).all()
    for k, b in enumerate(good):
        assert torch.equal(v_all[b], v_good[k]) and torch.isfinite(v_all[b]).all()


def test_decreasing_and_infinite_abscissae_are_flagged(gpu_device):
    x = torch.linspace(0, 1, 9)
    bad = [x.flip(0), x.clone().index_fill_(0, torch.tensor([4]), float('inf')), x]
    v, st = cubic_spline_1d(torch.cat(bad).to(gpu_device), ordinates(torch.cat(bad)).to(gpu_device), [9, 9, 9],
                            torch.linspace(0, 1, 7).to(gpu_device))
    torch.cuda.synchronize()
    assert st.tolist() == [SPLINE_NOT_INCREASING, SPLINE_NOT_FINITE, SPLINE_OK]
    assert torch.isnan(v[:2]).all() and torch.isfinite(v[2]).all()


def test_a_set_does_not_depend_on_its_batch(gpu_device):
    sizes = [4, 21, 65, 1024, 101]
    xs = [abscissae(n, 'graded' if i % 2 else 'uniform') for i, n in enumerate(sizes)]
    ys = [ordinates(x) for x in xs]
    q = torch.linspace(-0.01, 1.01, 101).to(gpu_device)
    for deriv in (0, 2):
        together, _ = cubic_spline_1d(torch.cat(xs).to(gpu_device), torch.cat(ys).to(gpu_device), sizes, q, deriv=deriv)
        for b, (x, y) in enumerate(zip(xs, ys)):
            alone, _ = cubic_spline_1d(x.to(gpu_device), y.to(gpu_device), [sizes[b]], q, deriv=deriv)
            assert torch.equal(alone[0], together[b]), (sizes[b], deriv)
