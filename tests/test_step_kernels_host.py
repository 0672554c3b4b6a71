"""What tests/test_gpu_step_kernels.py assumes about tests/step_kernels_restatement.py, proved on the CPU.

For every entry of every case table: the restatement evaluated in fp32 in another summation order (contraction indices reversed,
rows added strictly one after the other from the last to the first) stays inside the bar - the bar is one a correct fp32
evaluation meets, whatever its order - and every planted wrong variant of the restatement leaves the bar on at least one case of
its operation - the bar and the cases see the mistakes they are there for.  The restatements of the coefficients, their chain rule
and both losses agree with torch autograd in fp64 to 1e-12."""
import pytest
import torch
import torch.nn.functional as F

import step_kernels_restatement as R
from step_kernels_restatement import F32, F64, FAMILIES, U, gamma


@pytest.mark.parametrize('family', FAMILIES, ids=lambda f: f.name)
def test_reordered_fp32_restatement_stays_inside_the_bar(family):
    worst = (0.0, '')
    for case in family.cases:
        inp = family.make(case)
        ref = family.ref(case, inp)
        got = family.ref(case, inp, dtype=F32, flip=True)
        for k, (ok, ratio) in family.check(case, inp, got, ref).items():
            assert ok, (case['id'], k, ratio)
            worst = max(worst, (ratio, case['id'] + ':' + k))
    print(f"{family.name}: {len(family.cases)} cases, worst error / bar of the reordered fp32 restatement {worst[0]:.3f} ({worst[1]})")


@pytest.mark.parametrize('family,variant', [(f, v) for f in FAMILIES for v in f.variants], ids=lambda x: x if isinstance(x, str) else x.name)
def test_each_planted_variant_leaves_the_bar(family, variant):
    seen = 0
    for case in family.cases:
        inp = family.make(case)
        ref = family.ref(case, inp)
        wrong = family.ref(case, inp, variant=variant)
        seen += 1
        if not all(ok for ok, _ in family.check(case, inp, wrong, ref).values()):
            print(f"{family.name} / {variant}: outside the bar at {case['id']} (case {seen} of {len(family.cases)})")
            return
    pytest.fail(f"{family.name}: no case sees the variant {variant}")


# the variants every SHARP case must see: a spike sits exactly where the variant acts
@pytest.mark.parametrize('family', [R.SLAB, R.LAYER_PARAMS, R.LOSS_PARTIALS], ids=lambda f: f.name)
def test_a_spike_in_the_last_row_sees_the_dropped_row_and_a_spike_anywhere_its_double(family):
    for case in family.cases:
        if case['row'] is None or (family is R.LAYER_PARAMS and case['L'] != 4):
            continue
        inp = family.make(case)
        ref = family.ref(case, inp)
        doubled = family.check(case, inp, family.ref(case, inp, variant='double_row'), ref)
        assert not all(ok for ok, _ in doubled.values()), case['id']
        if case['row'] == case['n'] - 1:
            dropped = family.check(case, inp, family.ref(case, inp, variant='drop_last_row'), ref)
            assert not all(ok for ok, _ in dropped.values()), case['id']


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('case', R.COEFFS_CASES, ids=lambda c: c['id'])
def test_coefficients_and_chain_rule_agree_with_autograd(case):
    inp = R.coeffs_make(case)
    wq, bq, wk = (inp[k].to(F64).requires_grad_() for k in ('wq', 'bq', 'wk'))
    bk = torch.zeros(case['c'], dtype=F64, requires_grad=True)
    # the attention score of GRAND_plus.py:146-147,225-260 sees the weights through q_i . k_j = x_i^T Wq^T (Wk x_j + bk) + bq . (Wk x_j + bk):
    # per target i the bk terms are the same for every j and drop out of the softmax, which leaves A = Wk^T Wq and p0 = Wk^T bq
    a, p0 = wk.T @ wq, wk.T @ bq
    ((a * inp['da'].to(F64)).sum() + (p0 * inp['dp0'].to(F64)).sum() + 0.0 * bk.sum()).backward()
    ref = R.coeffs_ref(case, inp)
    assert _close(ref['a'], a.detach()) and _close(ref['p0'], p0.detach())
    assert _close(ref['d_wq'], wq.grad) and _close(ref['d_bq'], bq.grad) and _close(ref['d_wk'], wk.grad)
    assert torch.equal(ref['d_bk'], bk.grad)


@pytest.mark.parametrize('case', [c for c in R.LOSS_CASES if c['n'] in (1, 257, 32769) and c['row'] in (None, 0)], ids=lambda c: c['id'])
def test_losses_agree_with_autograd(case):
    inp = R.loss_make(case)
    pred = inp['pred'].to(F64).requires_grad_()
    loss = (F.l1_loss if case['l1'] else F.mse_loss)(pred, inp['target'].to(F64))
    loss.backward()
    ref = R.loss_ref(case, inp)
    assert _close(ref['loss'], loss.detach()) and _close(ref['seed'], pred.grad)


@pytest.mark.parametrize('case', [c for c in R.SEED_CASES if c['c'] == 8], ids=lambda c: c['id'])
def test_mesh_loss_seed_agrees_with_autograd(case):
    inp = R.seed_make(case)
    x = inp['x_top'].to(F64).requires_grad_()
    x_phys = x[:, :case['d']]
    loss = (F.l1_loss if case['l1'] else F.mse_loss)(x_phys, inp['target'].to(F64))
    loss.backward(gradient=torch.tensor(R.SEED_GS, dtype=F64))
    ref = R.seed_ref(case, inp)
    assert _close(ref['added'], loss.detach()) and _close(ref['g_top'], x.grad) and torch.equal(ref['x_phys'], x_phys.detach())
    if case['kind'] == 'all_equal':
        assert float(ref['added']) == 0.0 and not ref['g_top'].any()


@pytest.mark.parametrize('case', [c for c in R.ADAM_CASES if c['n'] == 257 and c['gs'] == 1.0], ids=lambda c: c['id'])
def test_adam_restatement_is_torch_optim_adam(case):
    """One step of torch.optim.Adam in fp64 from the same state (step count t - 1), with the fp32-rounded hyper-parameters."""
    inp, h = R.adam_make(case), R.adam_hyper(case)
    p = inp['p'].to(F64).clone().requires_grad_()
    opt = torch.optim.Adam([p], lr=h['lr'], betas=(h['b1'], h['b2']), eps=h['eps'], weight_decay=h['wd'])
    opt.state[p] = dict(step=torch.tensor(float(case['t'] - 1)), exp_avg=inp['m'].to(F64).clone(), exp_avg_sq=inp['v'].to(F64).clone())
    p.grad = inp['g'].to(F64).clone()
    opt.step()
    ref = R.adam_ref(case, inp)
    assert _close(ref['p'], p.detach()) and _close(ref['m_exact'], opt.state[p]['exp_avg']) and _close(ref['v_exact'], opt.state[p]['exp_avg_sq'])
    # the moments' own references differ from those only by the one rounding of the decayed gradient they take as their input
    assert float((ref['g_in'] - (inp['g'].to(F64) + h['wd'] * inp['p'].to(F64))).abs().max()) <= U * float(ref['g_in'].abs().max())
    assert float((ref['delta'] - (p.detach() - inp['p'].to(F64))).abs().max()) <= 1e-12 * float(ref['delta'].abs().max() + 1e-300) + 1e-17
    if case['grads'] == 'zero':
        assert torch.equal(ref['p'], inp['p'].to(F64))
    if case['grads'] == 'tiny' and case['wd'] == 0.0:                      # eps decides the denominator
        assert float((ref['v'].sqrt()).max()) < 0.1 * h['eps'] or case['t'] < 10


def test_exp_avg_bar_is_on_its_terms():
    """gamma_4 |m_ref| and rho |delta_ref| are not bounds an fp32 evaluation can meet where b1 m and (1 - b1) g' cancel: the fp32
    restatement itself leaves them on a 'cancel' case, and stays inside the same factors of the value of the terms."""
    case = next(c for c in R.ADAM_CASES if c['grads'] == 'cancel' and c['t'] == 1000 and c['wd'] == 0.0)
    inp = R.adam_make(case)
    ref, got = R.adam_ref(case, inp), R.adam_ref(case, inp, dtype=F32, flip=True)
    bars = R.adam_bars(case, inp, ref, got)
    err_m, err_p = (got['m'] - ref['m']).abs(), (got['p'] - ref['p']).abs()
    assert bool((err_m > gamma(4) * ref['m'].abs()).any()) and bool((err_m <= bars['m']).all())
    # (p leaves rho |delta_ref| only where |p| is too small for u |p_new| to cover the cancelled exp_avg: rare, so not asserted)
    assert bool((err_p <= bars['p']).all())


@pytest.mark.parametrize('case', [c for c in R.ADAM_CASES if c['grads'] != 'cancel' and c['n'] in (257, 70001)], ids=lambda c: c['id'])
def test_adam_bars_are_the_literal_ones_where_exp_avg_does_not_cancel(case):
    """u |p_new| + rho(t) |delta_ref| and gamma_4 |m_ref|, gamma_4 |v_ref| as the bars are stated."""
    inp = R.adam_make(case)
    ref = R.adam_ref(case, inp)
    bars = R.adam_bars(case, inp, ref, ref)
    assert _close(bars['p'], U * ref['p'].abs() + R.adam_rho(case) * ref['delta'].abs())
    assert _close(bars['m'] / gamma(4), ref['m'].abs()) and torch.equal(bars['v'], gamma(4) * ref['v'].abs())


def test_rho_is_what_the_cancellation_of_the_bias_corrections_allows():
    case = dict(t=1, betas=(0.9, 0.999), wd=0.0, gs=1.0)
    assert 1900 * U < R.adam_rho(case) < 2100 * U                         # b2 = 0.999, t = 1: 2 * 0.999 / 0.001 u
    assert R.adam_rho(dict(case, t=700)) < 20 * U and R.adam_rho(dict(case, t=20000)) < 16.001 * U
    # the fp32 corrections as the library forms them (1 - powf) against fp64, in units of what rho grants them
    for b1, b2 in R.ADAM_BETAS:
        for t in R.ADAM_T:
            b1f, b2f = R.f32(b1), R.f32(b2)
            bc1 = float(1.0 - torch.tensor(b1f, dtype=F32) ** torch.tensor(float(t), dtype=F32))
            bc2 = float(1.0 - torch.tensor(b2f, dtype=F32) ** torch.tensor(float(t), dtype=F32))
            assert abs(bc1 - (1.0 - b1f ** t)) / (1.0 - b1f ** t) <= (1.0 + 4.0 * b1f ** t / (1.0 - b1f ** t)) * U
            assert abs(bc2 - (1.0 - b2f ** t)) / (1.0 - b2f ** t) <= (1.0 + 4.0 * b2f ** t / (1.0 - b2f ** t)) * U


def test_case_tables_reach_the_launch_edges():
    assert R.slab_spike_rows(1) == [0] and R.slab_spike_rows(3) == [0, 2]
    assert R.slab_spike_rows(9) == [0, 6, 7, 8]                           # per = 2: chunk 3 = rows 6, 7; chunk 4 = row 8 alone; chunks 5.. empty
    assert R.slab_spike_rows(300) == [0, 114, 145, 146, 151, 299]         # per = 38: one 32-row group (114..145) and six leftover rows
    assert R.slab_spike_rows(512) == [0, 192, 223, 224, 255, 511]         # per = 64: two full groups
    assert {c['n'] for c in R.SLAB_CASES} == set(R.SLAB_ROWS) and {c['c'] for c in R.SLAB_CASES} == set(R.C_ALL)
    assert R.enc_rows(64)[-1] == 4096 * 16 + 1 and R.enc_rows(256)[:3] == (1, 3, 4)
    assert {(c['dim'], c['f'], c['uu'], c['bias']) for c in R.ENC_CASES if not c['linear']} == set(R.ENC_CONFIGS)
    assert {c['c'] for c in R.ENC_CASES if not c['linear'] and c['n'] == 4096 * (1024 // c['c']) + 1} == set(R.ENC_C)
    assert max(c['c'] * c['dim'] for c in R.ENC_CASES if c['linear']) == 4096
    assert {c['dim'] for c in R.ENC_CASES if c['linear']} == {1, 4, 5, 16}
    for c in R.PAD_CASES:                                                 # n c / 4 float4 stores: below, at and over two workgroups of 256
        assert c['n'] * c['c'] // 4 in range(512 - c['c'] // 4, 512 + c['c'] // 4 + 1)
    for c in R.SEED_CASES:                                                # n c threads: below, at and over three workgroups of 256
        assert abs(c['n'] * c['c'] - 768) <= c['c']
    assert {c['n'] for c in R.ADAM_CASES if c['grads'] == 'normal'} == set(R.ADAM_N)
    assert {c['t'] for c in R.ADAM_CASES} == set(R.ADAM_T)
    assert {c['n'] for c in R.LOSS_CASES} == set(R.LOSS_ROWS) and R.loss_spike_rows(131073) == [0, 255, 256, 32767, 32768, 131072]
    ids = [c['id'] for f in FAMILIES for c in f.cases]
    assert len(ids) == len(set(ids))
