"""fp64 restatements, bars and case tables of the per-step kernels (composite coefficients and their chain rule, slab sums,
layer-parameter sums, Adam, losses, encoder, copies).

Written from include/gadapt_hip.h and the reference lines it cites - GRAND_plus.py:146-147 (A = Wk^T Wq, p0 = Wk^T bq),
GNN.py:72-98,225-239 (encoder and feature concatenation), GNN.py:299 (x_phys = x[:, :dim]), run_GNN.py:80-84,106 (mean squared / mean
absolute error), run_GNN.py:88,128-131 (torch.optim.Adam) - not from the kernels.  tests/test_step_kernels_host.py proves on the CPU
what tests/test_gpu_step_kernels.py assumes about every family below; the GPU test then only swaps the evaluation.

A FAMILY is one operation: `cases` (dicts with an `id`), `make(case)` -> fp32 CPU inputs (seeded by the id), `ref(case, inp, dtype,
flip, variant)` -> outputs, `bars(case, inp, ref)` -> one bar per output, `variants` -> the planted wrong restatements.

BARS (u = 2^-24, gamma_n = n u / (1 - n u); all inputs are fp32 values and the fp64 reference is computed from those same values):
  * sums and dot products: |got - ref| <= gamma_m S + TINY, S = the fp64 sum of the absolute values of all terms (the restatement on
    |inputs|), m = number of terms + the roundings outside the sum (listed per family below, never more than 10).  Higham, Accuracy
    and Stability of Numerical Algorithms, eq. (3.4)-(3.5): holds for every summation order, with or without FMA.  TINY = 2^-126, the
    smallest normal fp32, is the absolute floor.
  * sharp cases - every term zero but one row / entry / partial of magnitude 1: gamma_4 |ref| + TINY (a product, a scale factor and
    additions of zeros: at most four roundings), which a dropped or doubled term misses by 100 %.
  * copies: bar 0.
  * loss seed: gamma_3 |ref| + TINY (the difference, 1 / (N d), one product; grad_scale = 0.5 is exact).
  * Adam: |p_new - ref| <= u |p_new| + rho(t) |delta_ref|, rho(t) = (16 + 4 b1^t / (1 - b1^t) + 2 b2^t / (1 - b2^t)) u: sixteen
    roundings of the update formula, and the cancellation of 1 - b^t formed in fp32 from a powf of up to 2 ulp (bias correction 1
    enters once: 2 ulp + the subtraction and half-ulp slack -> 4; bias correction 2 under a square root: half of that -> 2).
    |delta_ref| and |m_ref| below are taken on the TERMS of exp_avg, b1 |m| + (1 - b1) |g'|: the same numbers on every case whose
    exp_avg does not cancel against the gradient - all the cases but the 'cancel' ones, which are there to show the difference
    (tests/test_step_kernels_host.py::test_adam_bars_are_the_literal_ones_where_exp_avg_does_not_cancel).
    Moments: gamma_4 of their own fp64 values - the moment update in fp64 from ITS fp32 inputs, the old moment and the fp32 gradient
    after scale and decay g' = fl(wd p + g grad_scale) (one fused rounding): (1 - b), two products and the sum are the four roundings.
    From p and g instead, g' enters exp_avg_sq squared with a rounding of its own and gamma_4 is no bound: the fp32 restatement itself
    reaches 4.08 u at weight decay 1e-2 (adam-n4160-t1000-gs1.0-wd0.01-b0.9-normal, element 1969).  For exp_avg_sq, whose terms are
    non-negative, the value is |v_ref|; for exp_avg it is that of its terms, b1 |m| + (1 - b1) |g'|, because no fp32 evaluation meets
    gamma_4 |m_ref| where b1 m and (1 - b1) g' cancel (tests/test_step_kernels_host.py::test_exp_avg_bar_is_on_its_terms shows the
    fp32 restatement itself failing that).  A wrong g' still shows: in p, whose reference never rounds it, and in both moments.
"""
import zlib

import torch

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24
TINY = 2.0 ** -126
C_ALL = (4, 8, 16, 32, 64, 128)
SLAB_CHUNKS = 8              # first-level chunks of the slab sums (the spike rows sit at their edges)


def gamma(n):
    return n * U / (1.0 - n * U)


def f32(x):
    """The fp32 value the C-ABI receives for a Python float, as a Python float."""
    return float(torch.tensor(x, dtype=F32))


def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(case['id'].encode()))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F32)


def _mm(a, b, flip):
    """a @ b; flip: the contraction index runs the other way."""
    return a.flip(1) @ b.flip(0) if flip else a @ b


def _sum0(x, flip):
    """Sum over dim 0; flip: strictly sequential from the last row to the first (cumsum), not torch's blocked order."""
    if x.shape[0] == 0:
        return torch.zeros(x.shape[1:], dtype=x.dtype)
    return x.flip(0).cumsum(0)[-1] if flip else x.sum(0)


def inside(got, ref, bar):
    """(ok, worst |got - ref| / bar).  A zero bar asks for equality; NaN or inf anywhere is outside."""
    got, ref, bar = got.detach().cpu().to(F64), ref.to(F64), torch.as_tensor(bar, dtype=F64)
    if got.shape != ref.shape:
        return False, float('inf')
    err = (got - ref).abs()
    bar = bar.expand_as(err) if bar.dim() else bar.expand(err.shape)
    bad = ~(err <= bar)                                           # (NaN compares false)
    ratio = torch.where(bar > 0, err / bar.clamp_min(TINY * U), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float('inf'))))
    ratio = torch.nan_to_num(ratio, nan=float('inf'))
    return not bool(bad.any()), float(ratio.max()) if ratio.numel() else 0.0


class Family:
    def __init__(self, name, cases, make, ref, bars, variants=()):
        self.name, self.cases, self.make, self.ref, self.bars, self.variants = name, cases, make, ref, bars, tuple(variants)

    def check(self, case, inp, got, ref=None):
        """{output: (ok, ratio)} of `got` against the fp64 restatement."""
        ref = self.ref(case, inp) if ref is None else ref
        bars = self.bars(case, inp, ref, got) if self is ADAM else self.bars(case, inp, ref)
        return {k: inside(got[k], ref[k], bars[k]) for k in bars if k in got}


def _t(x, dtype, absolute=False):
    return (x.abs() if absolute else x).to(dtype)


# ------------------------------------------------------------------------------------------------ coefficients and chain rule
# A[o][c] = sum_r Wk[r][o] Wq[r][c], p0[o] = sum_r Wk[r][o] bq[r] (C terms each: m = C);
# d_wq[r][c] = sum_o Wk[r][o] dA[o][c] (C), d_wk[r][o] = sum_c Wq[r][c] dA[o][c] + bq[r] dp0[o] (C + 1), d_bq[r] = sum_o Wk[r][o] dp0[o] (C),
# d_bk = 0 exactly.
COEFF_KINDS = ('random', 'bq0', 'one_wk_row', 'spike_da', 'spike_dp0')
COEFFS_CASES = [dict(id=f'coeffs-C{c}-{k}', c=c, kind=k) for c in C_ALL for k in COEFF_KINDS]


def coeffs_make(case):
    g, c, kind = _gen(case), case['c'], case['kind']
    inp = dict(wq=_randn(g, c, c), bq=_randn(g, c), wk=_randn(g, c, c), da=_randn(g, c, c), dp0=_randn(g, c))
    if kind == 'bq0':
        inp['bq'].zero_()
    elif kind == 'one_wk_row':
        keep = inp['wk'][c - 1].clone()
        inp['wk'].zero_()
        inp['wk'][c - 1] = keep
    elif kind == 'spike_da':
        inp['da'].zero_(); inp['dp0'].zero_()
        inp['da'][c - 1, 0] = 1.0
    elif kind == 'spike_dp0':
        inp['da'].zero_(); inp['dp0'].zero_()
        inp['dp0'][c - 1] = 1.0
    return inp


def coeffs_ref(case, inp, dtype=F64, flip=False, variant=None, absolute=False):
    wq, bq, wk, da, dp0 = (_t(inp[k], dtype, absolute) for k in ('wq', 'bq', 'wk', 'da', 'dp0'))
    a = _mm(wk.T.contiguous(), wq, flip)
    if variant == 'a_transposed':
        a, da = a.T.contiguous(), da.T.contiguous()
    d_wk = _mm(wq, da.T.contiguous(), flip)
    if variant != 'no_bq_dp0':
        d_wk = d_wk + bq[:, None] * dp0[None, :]
    return dict(a=a, p0=_mm(wk.T.contiguous(), bq[:, None], flip)[:, 0], d_wq=_mm(wk, da, flip), d_bq=_mm(wk, dp0[:, None], flip)[:, 0],
                d_wk=d_wk, d_bk=torch.zeros(case['c'], dtype=dtype))


def coeffs_bars(case, inp, ref):
    c, kind = case['c'], case['kind']
    s = coeffs_ref(case, inp, absolute=True)
    terms = dict(a=c, p0=c, d_wq=c, d_bq=c, d_wk=c + 1)
    sharp = {'one_wk_row': ('a', 'p0'), 'spike_da': ('d_wq', 'd_bq', 'd_wk'), 'spike_dp0': ('d_wq', 'd_bq', 'd_wk')}.get(kind, ())
    bars = {k: (gamma(4) * ref[k].abs() if k in sharp else gamma(m) * s[k]) + TINY for k, m in terms.items()}
    bars['d_bk'] = torch.zeros(c, dtype=F64)
    return bars


COEFFS = Family('coeffs', COEFFS_CASES, coeffs_make, coeffs_ref, coeffs_bars, ('a_transposed', 'no_bq_dp0'))


# ------------------------------------------------------------------------------------------------ slab sums
# slab [n_rows][C*C + C] -> dA [C,C], dp0 [C]: n_rows terms per entry, no products, no scale: m = n_rows.
SLAB_ROWS = (1, 3, 8, 9, 15, 65, 300, 512)


def slab_spike_rows(n):
    """Row 0, the last row, the first and last row of a middle chunk and, where the chunk is longer than 32 rows, both sides of
    its first 32-row group."""
    per = -(-n // SLAB_CHUNKS)
    q = min(3, (n - 1) // per)
    lo, hi = q * per, min(n, (q + 1) * per) - 1
    rows = {0, n - 1, lo, hi}
    if hi - lo >= 32:
        rows |= {lo + 31, lo + 32}
    return sorted(rows)


def _rows_variant(x, variant, row=0):
    """The rows a wrong sum takes."""
    if variant == 'drop_last_row':
        return x[:-1]
    if variant == 'double_row':
        return torch.cat([x, x[row:row + 1]], 0)
    return x


SLAB_CASES = [dict(id=f'slab-C{c}-n{n}-{k}', c=c, n=n, row=r) for c in C_ALL for n in SLAB_ROWS
              for k, r in [('dense', None)] + [(f'spike{r}', r) for r in slab_spike_rows(n)]]


def slab_make(case):
    c, n, row = case['c'], case['n'], case['row']
    if row is None:
        return dict(slab=_randn(_gen(case), n, c * c + c))
    slab = torch.zeros(n, c * c + c, dtype=F32)
    slab[row] = 1.0
    return dict(slab=slab)


def slab_ref(case, inp, dtype=F64, flip=False, variant=None, absolute=False):
    c = case['c']
    s = _sum0(_rows_variant(_t(inp['slab'], dtype, absolute), variant, case['row'] or 0), flip)
    return dict(d_a=s[:c * c].reshape(c, c), d_p0=s[c * c:])


def slab_bars(case, inp, ref):
    if case['row'] is not None:
        return {k: gamma(4) * v.abs() + TINY for k, v in ref.items()}
    s = slab_ref(case, inp, absolute=True)
    return {k: gamma(case['n']) * s[k] + TINY for k in ref}


SLAB = Family('slab_reduce', SLAB_CASES, slab_make, slab_ref, slab_bars, ('drop_last_row', 'double_row'))

# partials [2][L][n_rows] -> d_layer_params [2][L] (row 1 exact zeros when want_d_scale = 0): m = n_rows.
LP_LAYERS, LP_ROWS = (1, 4, 20), (1, 255, 256, 257, 1024, 1025, 2049)


def lp_spike_rows(n):
    return sorted({r for r in (0, 255, 256, 1023, 1024, n - 1) if r < n})


LP_CASES = [dict(id=f'lp-L{L}-n{n}-w{w}-{k}', L=L, n=n, want=w, row=r) for L in LP_LAYERS for n in LP_ROWS for w in (1, 0)
            for k, r in [('dense', None)] + [(f'spike{r}', r) for r in lp_spike_rows(n)]]


def lp_make(case):
    L, n, row = case['L'], case['n'], case['row']
    if row is None:
        return dict(partials=_randn(_gen(case), 2, L, n))
    p = torch.zeros(2, L, n, dtype=F32)
    p[:, :, row] = 1.0
    return dict(partials=p)


def lp_ref(case, inp, dtype=F64, flip=False, variant=None, absolute=False):
    x = _t(inp['partials'], dtype, absolute).permute(2, 0, 1)             # rows first
    s = _sum0(_rows_variant(x, variant, case['row'] or 0), flip).clone()
    if not case['want']:
        s[1] = 0
    return dict(d_layer_params=s)


def lp_bars(case, inp, ref):
    if case['row'] is not None:
        bar = gamma(4) * ref['d_layer_params'].abs() + TINY
    else:
        bar = gamma(case['n']) * lp_ref(case, inp, absolute=True)['d_layer_params'] + TINY
    if not case['want']:
        bar[1] = 0
    return dict(d_layer_params=bar)


LAYER_PARAMS = Family('layer_params_reduce', LP_CASES, lp_make, lp_ref, lp_bars, ('drop_last_row', 'double_row'))

# loss partials of the step tail: loss_out = sum / loss_count: n terms + (count -> float, reciprocal, product): m = n + 3.
LOSS_COUNT = 4 * 1234
LOSSP_CASES = [dict(id=f'lossp-n{n}-{k}', n=n, row=r) for n in (1, 7, 256, 1025, 4096)
               for k, r in (('dense', None), ('spike_first', 0), ('spike_last', n - 1))]


def lossp_make(case):
    if case['row'] is None:
        return dict(partials=_randn(_gen(case), case['n']).abs())
    p = torch.zeros(case['n'], dtype=F32)
    p[case['row']] = 1.0
    return dict(partials=p)


def lossp_ref(case, inp, dtype=F64, flip=False, variant=None, absolute=False):
    x = _rows_variant(_t(inp['partials'], dtype, absolute)[:, None], variant, case['row'] or 0)
    return dict(loss=_sum0(x, flip)[0] * (torch.ones((), dtype=dtype) / LOSS_COUNT))


def lossp_bars(case, inp, ref):
    if case['row'] is not None:
        return dict(loss=gamma(4) * ref['loss'].abs() + TINY)
    return dict(loss=gamma(case['n'] + 3) * lossp_ref(case, inp, absolute=True)['loss'] + TINY)


LOSS_PARTIALS = Family('loss_partials', LOSSP_CASES, lossp_make, lossp_ref, lossp_bars, ('drop_last_row', 'double_row'))


# ------------------------------------------------------------------------------------------------ Adam
# torch.optim.Adam (run_GNN.py:88,128-131), single tensor, no amsgrad: g' = g grad_scale + wd p; m = b1 m + (1 - b1) g';
# v = b2 v + (1 - b2) g'^2; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).
ADAM_N, ADAM_T = (1, 255, 256, 257, 4160, 70001), (1, 2, 3, 10, 1000, 20000)
ADAM_BETAS = ((0.9, 0.999), (0.5, 0.9))
ADAM_LR, ADAM_EPS = 1e-3, 1e-8
ADAM_CASES = [dict(id=f'adam-n{n}-t{t}-gs{gs}-wd{wd}-b{b1}-normal', n=n, t=t, gs=gs, wd=wd, betas=(b1, b2), grads='normal')
              for n in ADAM_N for t in ADAM_T for gs in (1.0, 0.25) for wd in (0.0, 1e-2) for b1, b2 in ADAM_BETAS]
ADAM_CASES += [dict(id=f'adam-n{n}-t{t}-wd{wd}-tiny', n=n, t=t, gs=1.0, wd=wd, betas=ADAM_BETAS[0], grads='tiny')
               for n in (257, 4160) for t in ADAM_T for wd in (0.0, 1e-2)]
ADAM_CASES += [dict(id=f'adam-n4160-t{t}-wd{wd}-cancel', n=4160, t=t, gs=0.25, wd=wd, betas=ADAM_BETAS[0], grads='cancel')
               for t in ADAM_T for wd in (0.0, 1e-2)]
ADAM_CASES += [dict(id=f'adam-n{n}-t{t}-zero', n=n, t=t, gs=1.0, wd=0.0, betas=ADAM_BETAS[0], grads='zero') for n in (257,) for t in ADAM_T]


def adam_make(case):
    g, n = _gen(case), case['n']
    inp = dict(p=0.1 * _randn(g, n), g=_randn(g, n), m=0.01 * _randn(g, n), v=(0.01 * _randn(g, n)) ** 2)
    if case['grads'] == 'normal':
        # exp_avg has the sign of the gradient it meets: the bars below are relative to |m_ref| and |delta_ref|, which bound nothing
        # where b1 m and (1 - b1) g' cancel ('cancel' keeps the independent signs and shows that they then differ from the terms)
        g_eff = inp['g'].to(F64) * f32(case['gs']) + f32(case['wd']) * inp['p'].to(F64)
        inp['m'] = (inp['m'].abs().to(F64) * torch.where(g_eff < 0, -1.0, 1.0)).to(F32)
    elif case['grads'] in ('tiny', 'zero'):                            # eps decides the denominator / nothing moves
        inp['m'].zero_(); inp['v'].zero_()
        inp['g'] = 1e-9 * inp['g'] if case['grads'] == 'tiny' else torch.zeros(n, dtype=F32)
    return inp


def adam_hyper(case):
    """The fp32-rounded hyper-parameters, as Python floats."""
    return dict(lr=f32(ADAM_LR), b1=f32(case['betas'][0]), b2=f32(case['betas'][1]), eps=f32(ADAM_EPS), wd=f32(case['wd']), gs=f32(case['gs']))


def adam_ref(case, inp, dtype=F64, flip=False, variant=None, absolute=False):
    """dtype fp32: every operation of the formula rounded to fp32 once - a x + y as one fused operation, as an fp32 evaluation with
    FMA does it - and the powers b^t from torch's fp32 pow."""
    rnd = (lambda x: x.to(F32).to(F64)) if dtype == F32 else (lambda x: x)
    h = {k: torch.tensor(v, dtype=F64) for k, v in adam_hyper(case).items()}
    p, g, m, v = (inp[k].to(F64) for k in ('p', 'g', 'm', 'v'))
    one = torch.ones((), dtype=F64)
    decay = case['wd'] != 0.0
    gg = rnd(g * h['gs'])
    if decay and variant != 'wd_after_moments':
        gg = rnd(h['wd'] * p + gg)
    mn = rnd(h['b1'] * m + rnd(rnd(one - h['b1']) * gg))
    vn = rnd(h['b2'] * v + rnd(rnd(rnd(one - h['b2']) * gg) * gg))
    # the moments' OWN values: their update in fp64 from its fp32 inputs - the old moment and the fp32 gradient after scale and decay
    g_in = gg.to(F32).to(F64)
    m_own = rnd(h['b1'] * m + rnd(rnd(one - h['b1']) * g_in))
    v_own = rnd(h['b2'] * v + rnd(rnd(rnd(one - h['b2']) * g_in) * g_in))
    t = torch.tensor(float(case['t'] - (1 if variant == 'bias_t_minus_1' else 0)), dtype=dtype)
    bc1, bc2 = (rnd(one - (h[k].to(dtype) ** t).to(F64)) for k in ('b1', 'b2'))
    if variant == 'eps_inside_sqrt':
        denom = rnd(rnd(rnd(vn / bc2) + h['eps']).sqrt())
    else:
        denom = rnd(rnd(rnd(vn.sqrt()) / rnd(bc2.sqrt())) + h['eps'])
    delta = -rnd(rnd(h['lr'] / bc1) * rnd(mn / denom))
    if decay and variant == 'wd_after_moments':
        delta = rnd(delta - rnd(h['lr'] * h['wd']) * p)
    # |delta| with exp_avg replaced by the value of its terms: |delta| itself unless b1 m and (1 - b1) g' cancel
    delta_terms = (h['lr'] / bc1).abs() * (h['b1'] * m.abs() + (one - h['b1']) * gg.abs()) / denom
    return dict(p=rnd(p + delta), m=m_own, v=v_own, delta=delta, g_in=g_in, m_exact=mn, v_exact=vn, delta_terms=delta_terms)


def adam_rho(case):
    h, t = adam_hyper(case), case['t']
    return (16.0 + 4.0 * h['b1'] ** t / (1.0 - h['b1'] ** t) + 2.0 * h['b2'] ** t / (1.0 - h['b2'] ** t)) * U


def adam_bars(case, inp, ref, got):
    h = adam_hyper(case)
    s_m = h['b1'] * inp['m'].to(F64).abs() + (1.0 - h['b1']) * ref['g_in'].abs()
    return dict(p=U * got['p'].detach().cpu().to(F64).abs() + adam_rho(case) * ref['delta_terms'], m=gamma(4) * s_m, v=gamma(4) * ref['v'].abs())


ADAM = Family('adam', ADAM_CASES, adam_make, adam_ref, adam_bars, ('eps_inside_sqrt', 'bias_t_minus_1', 'wd_after_moments'))


# ------------------------------------------------------------------------------------------------ losses
# loss = mean over the N d entries of (pred - target)^2 or |pred - target|; seed = d loss / d pred = 2 diff / (N d) or sign(diff) / (N d),
# sign(0) = 0 (torch's l1_loss backward).  Per term: the difference, its square and the product (3 roundings), N d - 1 additions,
# then 1 / (N d) and the product with it (2): m = N d + 5.  Targets are multiples of 1/8 so that a spike of +1 is exact.
LOSS_D, LOSS_ROWS = (1, 2, 3, 4, 5), (1, 255, 256, 257, 32768, 32769, 131073)
LOSS_STRIDES = (None, 4, 64)                                   # None: d.  (the row stride is not part of the operation: GPU test only)


def loss_spike_rows(n):
    return sorted({r for r in (0, 255, 256, 32767, 32768, n - 1) if r < n})


LOSS_CASES = [dict(id=f'loss-d{d}-n{n}-{"l1" if l1 else "mse"}-{k}', d=d, n=n, l1=l1, kind=k.rstrip('0123456789'), row=r)
              for d in LOSS_D for n in LOSS_ROWS for l1 in (0, 1)
              for k, r in [('random', None), ('half_equal', None)] + [(f'spike{r}', r) for r in loss_spike_rows(n)]]


def loss_make(case):
    g, n, d = _gen(case), case['n'], case['d']
    target = torch.randint(-32, 33, (n, d), generator=g).to(F32) / 8
    if case['kind'] == 'spike':
        pred = target.clone()
        pred[case['row'], 0] += 1.0
    else:
        pred = target + _randn(g, n, d)
        if case['kind'] == 'half_equal':
            pred[::2] = target[::2]
    return dict(pred=pred, target=target)


def _loss_core(diff, l1, n_entries, dtype, flip, variant, row):
    """(sum of the terms / n_entries, seed) of a difference matrix."""
    count = diff.shape[0] if variant == 'mean_over_n' else n_entries
    inv = torch.ones((), dtype=dtype) / count
    terms = _rows_variant(diff.abs() if l1 else diff * diff, variant, row)
    loss = _sum0(terms.reshape(-1, 1), flip)[0] * inv
    if l1:
        sign = torch.sign(diff)
        if variant == 'sign0_is_1':
            sign = torch.where(diff == 0, torch.ones_like(diff), sign)
        return loss, sign * inv
    return loss, 2.0 * diff * inv


def loss_ref(case, inp, dtype=F64, flip=False, variant=None, absolute=False):
    diff = inp['pred'].to(dtype) - inp['target'].to(dtype)
    loss, seed = _loss_core(diff, case['l1'], diff.numel(), dtype, flip, variant, case['row'] or 0)
    return dict(loss=loss, seed=seed)


def loss_bars(case, inp, ref):
    sharp = case['kind'] == 'spike'
    return dict(loss=gamma(4 if sharp else case['n'] * case['d'] + 5) * ref['loss'].abs() + TINY,      # (non-negative terms: S = the value)
                seed=gamma(3) * ref['seed'].abs() + TINY)


LOSS = Family('loss_forward', LOSS_CASES, loss_make, loss_ref, loss_bars, ('drop_last_row', 'double_row', 'sign0_is_1', 'mean_over_n'))

# gadapt_mesh_loss_seed: x_phys = x_top[:, :d] (a copy), g_top [N,C] = grad_scale * seed zero-padded, loss_out += loss.  Per term five
# roundings at most (difference, square, product, 1 / (N d), product with it) and the value loss_out held before: m = N d + 1 + 5.
SEED_L0, SEED_GS = 0.75, 0.5
SEED_C = (4, 8, 64)
SEED_CASES = [dict(id=f'seed-d{d}-c{c}-n{n}-{"l1" if l1 else "mse"}-{k}', d=d, c=c, n=n, l1=l1, kind=k, row=None)
              for d in LOSS_D for c in SEED_C if d <= c for n in (768 // c - 1, 768 // c, 768 // c + 1) for l1 in (0, 1)
              for k in ('random', 'half_equal', 'all_equal')]


def seed_make(case):
    g, n, d, c = _gen(case), case['n'], case['d'], case['c']
    x_top = _randn(g, n, c)
    target = _randn(g, n, d)
    if case['kind'] == 'half_equal':
        target[::2] = x_top[::2, :d]
    elif case['kind'] == 'all_equal':
        target = x_top[:, :d].clone()
    return dict(x_top=x_top, target=target)


def seed_ref(case, inp, dtype=F64, flip=False, variant=None, absolute=False):
    d = case['d']
    x = inp['x_top'].to(dtype)
    diff = x[:, :d] - inp['target'].to(dtype)
    loss, seed = _loss_core(diff, case['l1'], diff.numel(), dtype, flip, variant, 0)
    g_top = torch.zeros_like(x)
    g_top[:, :d] = seed * SEED_GS
    return dict(x_phys=x[:, :d].clone(), g_top=g_top, loss_out=loss + SEED_L0, added=loss)


def seed_bars(case, inp, ref):
    added = float(ref['added'])
    bar = gamma(case['n'] * case['d'] + 6) * (SEED_L0 + added) + TINY if added > 0 else 0.0
    return dict(x_phys=torch.zeros_like(ref['x_phys']), g_top=gamma(3) * ref['g_top'].abs() + TINY, loss_out=torch.tensor(bar, dtype=F64),
                added=torch.tensor(float('inf'), dtype=F64))
    # (`added` is judged through loss_out)


MESH_LOSS_SEED = Family('mesh_loss_seed', SEED_CASES, seed_make, seed_ref, seed_bars, ('drop_last_row', 'double_row', 'sign0_is_1', 'mean_over_n'))


# ------------------------------------------------------------------------------------------------ encoder
# x0[i][o] = sum_k feats[i][k] W[o][k] (+ b[o]), feats = [x_comp | f | uu] (GNN.py:225-239): F products and the bias: m = F + 1.
ENC_C = (4, 8, 16, 32, 64, 128, 256)
ENC_CONFIGS = [(dim, f, uu, b) for dim in (1, 2, 3) for f in (1, 0) for uu in (1, 0) for b in (1, 0)]


def enc_rows(c):
    r = 1024 // c                                                  # rows per workgroup
    return (1, r - 1, r, 4 * r - 1, 4 * r, 4 * r + 1, 4096 * r + 1)


def _enc_feature_cases():
    out, i = [], 0
    for c in ENC_C:
        for n in enc_rows(c):
            if n < 1:
                continue
            dim, f, uu, b = ENC_CONFIGS[(5 * i) % len(ENC_CONFIGS)]
            i += 1
            out.append(dict(id=f'encf-C{c}-n{n}-dim{dim}-f{f}-uu{uu}-b{b}', c=c, n=n, dim=dim, f=f, uu=uu, bias=b, linear=False))
    # both extras together at every dim and C (the column order is what a swap would break)
    for c in ENC_C:
        for dim in (1, 2, 3):
            out.append(dict(id=f'encf-C{c}-n{4 * (1024 // c) + 1}-dim{dim}-f1-uu1-b1-both', c=c, n=4 * (1024 // c) + 1, dim=dim, f=1, uu=1, bias=1, linear=False))
    return out


ENC_LINEAR_SHAPES = ((1, 4), (4, 64), (5, 8), (5, 128), (16, 16), (16, 256), (4, 256))      # (f, C); 16 * 256 = 4096 floats of LDS: the most


def _enc_linear_cases():
    out = []
    for f, c in ENC_LINEAR_SHAPES:
        rows = enc_rows(c) if (f, c) in ((1, 4), (5, 128), (16, 256)) else enc_rows(c)[:-1]
        for j, n in enumerate(rows):
            if n < 1:
                continue
            out.append(dict(id=f'encl-f{f}-C{c}-n{n}-b{j % 2}', c=c, n=n, dim=f, f=0, uu=0, bias=j % 2, linear=True))
    return out


ENC_CASES = _enc_feature_cases() + _enc_linear_cases()


def enc_make(case):
    g, n, c, dim = _gen(case), case['n'], case['c'], case['dim']
    nf = dim + case['f'] + case['uu']
    return dict(x_comp=_randn(g, n, dim), f=_randn(g, n) if case['f'] else None, uu=_randn(g, n) if case['uu'] else None,
                w=_randn(g, c, nf), b=_randn(g, c) if case['bias'] else None)


def enc_feats(inp, swap=False):
    extras = [inp[k][:, None] for k in (('uu', 'f') if swap else ('f', 'uu')) if inp[k] is not None]
    return torch.cat([inp['x_comp']] + extras, 1)


def enc_ref(case, inp, dtype=F64, flip=False, variant=None, absolute=False):
    feats = _t(enc_feats(inp, swap=variant == 'f_uu_swapped'), dtype, absolute)
    x0 = _mm(feats, _t(inp['w'], dtype, absolute).T.contiguous(), flip)
    if inp['b'] is not None:
        x0 = x0 + _t(inp['b'], dtype, absolute)
    return dict(x0=x0)


def enc_bars(case, inp, ref):
    nf = case['dim'] + case['f'] + case['uu']
    return dict(x0=gamma(nf + 1) * enc_ref(case, inp, absolute=True)['x0'] + TINY)


ENCODER = Family('encoder', ENC_CASES, enc_make, enc_ref, enc_bars, ('f_uu_swapped',))


# ------------------------------------------------------------------------------------------------ copies
# g_top [N,C] = g_phys [N,d] zero-padded (backward of GNN.py:299); dst[k][b] = src[k][idx[b]] (DataLoader collation, run_GNN.py:72-76).
PAD_SHAPES = ((1, 4), (2, 64), (3, 8), (4, 4), (5, 8), (7, 8), (8, 8))
PAD_CASES = [dict(id=f'pad-d{d}-c{c}-n{n}', d=d, c=c, n=n) for d, c in PAD_SHAPES for n in (2048 // c - 1, 2048 // c, 2048 // c + 1)]


def pad_make(case):
    return dict(g_phys=_randn(_gen(case), case['n'], case['d']))


def pad_ref(case, inp, dtype=F64, flip=False, variant=None, absolute=False):
    out = torch.zeros(case['n'], case['c'], dtype=dtype)
    out[:, :case['d']] = inp['g_phys'].to(dtype)
    return dict(g_top=out)


PAD = Family('pad_columns', PAD_CASES, pad_make, pad_ref, lambda case, inp, ref: dict(g_top=torch.zeros_like(ref['g_top'])))

GATHER_ROWS = (1, 3, 4, 21, 4100, 32 * 256 * 4 + 4)             # the last: one float4 more than 32 workgroups cover in one pass
GATHER_SAMPLES = 5
GATHER_CASES = ([dict(id=f'gather-row{r}-{o}', rows=(r,), order=o) for r in GATHER_ROWS for o in ('repeated', 'descending', 'one')]
                + [dict(id=f'gather-8-fields-{o}', rows=(1, 3, 4, 21, 4100, 8, 7, 32 * 256 * 4 + 4), order=o) for o in ('repeated', 'descending')])
GATHER_ORDERS = {'repeated': [3, 0, 3, 3, 1, 4, 0], 'descending': [4, 3, 2, 1, 0], 'one': [2]}


def gather_make(case):
    g = _gen(case)
    return dict(src=[_randn(g, GATHER_SAMPLES, r) for r in case['rows']], idx=torch.tensor(GATHER_ORDERS[case['order']], dtype=torch.int64))


def gather_ref(case, inp, dtype=F64, flip=False, variant=None, absolute=False):
    return {f'dst{k}': torch.stack([s[int(i)] for i in inp['idx']]).to(dtype) for k, s in enumerate(inp['src'])}


GATHER = Family('gather_fields', GATHER_CASES, gather_make, gather_ref, lambda case, inp, ref: {k: torch.zeros_like(v) for k, v in ref.items()})

FAMILIES = (COEFFS, SLAB, LAYER_PARAMS, LOSS_PARTIALS, ADAM, LOSS, MESH_LOSS_SEED, ENCODER, PAD, GATHER)
