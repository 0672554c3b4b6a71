"""The per-step kernels (csrc/gadapt_small.inc and their entry points) against fp64 at their launch edges.

Every bit-identity test of the training step - spread tail == narrow tail == step tail, fused == autograd iteration - rests on
gadapt_coeffs_forward / _backward, gadapt_slab_reduce[_coeffs_backward], gadapt_layer_params_reduce, gadapt_adam_step[_dev],
gadapt_loss_forward, gadapt_mesh_loss_seed, gadapt_encode_*, gadapt_pad_columns and gadapt_gather_fields.  Here each of them is
called through the C-ABI (and `mse_loss` / `l1_loss` where a wrapper exists) and compared with the plain fp64 restatement of
tests/step_kernels_restatement.py on that file's case tables: the rows per workgroup that do not divide the row count, the
four-rows-per-iteration prefetch, the grid caps (1024 encoder, 128 loss, 32 gather workgroups), the 32-row groups and empty chunks
of the slab sums, the workgroups that ride in another kernel's grid, the ticket counters, and the d > 4 / f > 4 loop paths.

BARS - derived, none fitted to an output (u = 2^-24, gamma_n = n u / (1 - n u); the inputs are fp32 values and the fp64 reference is
computed from those same values; tests/test_step_kernels_host.py shows on the CPU that a reordered fp32 evaluation of the
restatement meets every one of them on every case, and that each planted mistake leaves them):
  sums and dot products   |got - ref| <= gamma_m S + 2^-126, S = the fp64 sum of |terms|, m = terms + roundings outside the sum:
                          coefficients and chain rule C (d_wk: C + 1), slab and layer-parameter sums n_rows, loss partials n + 3,
                          loss N d + 5, mesh_loss_seed N d + 6, encoder F + 1.  Any summation order, with or without FMA.
  sharp cases             all terms zero but one row / entry / partial of magnitude 1: gamma_4 |ref| + 2^-126.
  copies                  torch.equal (gather_fields, pad_columns, x_phys).
  loss seed / g_top       gamma_3 |ref| + 2^-126; entries with pred == target exactly 0.
  Adam                    |p_new - ref| <= u |p_new| + rho(t) |delta_ref|, rho(t) = (16 + 4 b1^t / (1 - b1^t) + 2 b2^t / (1 - b2^t)) u;
                          both moments gamma_4 of their own fp64 values (what "own" means, and why |delta_ref| and |m_ref| are
                          taken on the terms of exp_avg: the restatement's docstring).
Claims of the header checked with torch.equal: gadapt_slab_reduce + gadapt_coeffs_backward == gadapt_slab_reduce_coeffs_backward;
gadapt_layer_params_reduce == the same sums riding in that call; gadapt_step_tail == gadapt_slab_reduce_coeffs_backward, then
gadapt_adam_step_dev, then gadapt_coeffs_forward; gadapt_encode_features == gadapt_encode_linear on the concatenation;
gadapt_encode_features_coeffs == gadapt_encode_features and gadapt_coeffs_forward.

Every case prints `[step-kernels] family case output error/bar` before it asserts (docs/measurements.md, "Per-step kernels against fp64")."""
import ctypes as C

import pytest
import torch

import step_kernels_restatement as R
from g_adaptivity_amd import l1_loss, mse_loss, unit_gradient
from g_adaptivity_amd._native import current_stream, lib, ptr
from step_kernels_restatement import F32, F64, U, gamma

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]
BADARG = -1
GUARD = 8
NAN = float('nan')


def _guarded(n, dev, dtype=F32):
    """(buffer, view of n elements) with GUARD NaN elements on both sides of the view."""
    buf = torch.full((n + 2 * GUARD,), NAN if dtype == F32 else -77, device=dev, dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
    head, tail = buf[:GUARD], buf[-GUARD:]
    return bool(torch.isnan(head).all() and torch.isnan(tail).all()) if buf.dtype == F32 else bool((head == -77).all() and (tail == -77).all())


def _to(inp, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}


def _judge(family, case, inp, got, ref=None, tag=''):
    res = family.check(case, inp, got, ref)
    for k, (ok, ratio) in res.items():
        print(f"[step-kernels] {family.name} {case['id']}{tag} {k} {ratio:.4f}")
    bad = {k: ratio for k, (ok, ratio) in res.items() if not ok}
    assert not bad, (case['id'] + tag, bad)
    assert set(res) >= set(got), (set(res), set(got))


def _weights(c, dev, seed=5):
    g = torch.Generator().manual_seed(seed + c)
    return [torch.randn(*s, generator=g).to(dev) for s in ((c, c), (c,), (c, c))]


def _bucket_views(flat, c):
    """[Wq | bq | Wk | bk] views of a flat bucket."""
    c2 = c * c
    return flat[:c2], flat[c2:c2 + c], flat[c2 + c:2 * c2 + c], flat[2 * c2 + c:2 * c2 + 2 * c]


# ------------------------------------------------------------------------------------------------ 1. coefficients and chain rule
@pytest.mark.parametrize('case', R.COEFFS_CASES, ids=lambda c: c['id'])
def test_coefficients_and_chain_rule(gpu_device, case):
    c, st = case['c'], current_stream(gpu_device)
    inp = R.coeffs_make(case)
    d = _to(inp, gpu_device)
    fbuf, fwd = _guarded(c * c + c, gpu_device)
    bbuf, bwd = _guarded(2 * c * c + 2 * c, gpu_device)
    assert lib().gadapt_coeffs_forward(ptr(d['wq']), ptr(d['bq']), ptr(d['wk']), ptr(fwd[:c * c]), ptr(fwd[c * c:]), c, st) == 0
    d_wq, d_bq, d_wk, d_bk = _bucket_views(bwd, c)
    assert lib().gadapt_coeffs_backward(ptr(d['wq']), ptr(d['bq']), ptr(d['wk']), ptr(d['da']), ptr(d['dp0']), ptr(d_wq), ptr(d_bq), ptr(d_wk),
                                        ptr(d_bk), c, st) == 0
    torch.cuda.synchronize()
    assert _guards_intact(fbuf) and _guards_intact(bbuf)
    got = dict(a=fwd[:c * c].view(c, c), p0=fwd[c * c:], d_wq=d_wq.view(c, c), d_bq=d_bq, d_wk=d_wk.view(c, c), d_bk=d_bk)
    assert bool((d_bk == 0).all())
    _judge(R.COEFFS, case, inp, got)


# ------------------------------------------------------------------------------------------------ 2. slab sums
@pytest.mark.parametrize('n_rows', R.SLAB_ROWS)
@pytest.mark.parametrize('c', R.C_ALL)
def test_slab_reduce(gpu_device, c, n_rows):
    st, row = current_stream(gpu_device), c * c + c
    wq, bq, wk = _weights(c, gpu_device)
    scratch = torch.full((32 * row,), NAN, device=gpu_device)
    for case in (k for k in R.SLAB_CASES if k['c'] == c and k['n'] == n_rows):
        inp = R.slab_make(case)
        slab = inp['slab'].to(gpu_device)
        sbuf, sums = _guarded(row, gpu_device)
        assert lib().gadapt_slab_reduce(ptr(slab), n_rows, ptr(scratch), ptr(sums[:c * c]), ptr(sums[c * c:]), c, st) == 0
        two, one = (torch.full((2 * row,), NAN, device=gpu_device) for _ in range(2))
        assert lib().gadapt_coeffs_backward(ptr(wq), ptr(bq), ptr(wk), ptr(sums[:c * c]), ptr(sums[c * c:]), *(ptr(v) for v in _bucket_views(two, c)), c, st) == 0
        scratch.fill_(NAN)
        assert lib().gadapt_slab_reduce_coeffs_backward(ptr(slab), n_rows, ptr(scratch), ptr(wq), ptr(bq), ptr(wk),
                                                        *(ptr(v) for v in _bucket_views(one, c)), c, st, None, 0, 0, None) == 0
        torch.cuda.synchronize()
        assert _guards_intact(sbuf)
        _judge(R.SLAB, case, inp, dict(d_a=sums[:c * c].view(c, c), d_p0=sums[c * c:]))
        assert not torch.isnan(one).any() and torch.equal(one, two), case['id']      # "the same results bit for bit"


@pytest.mark.parametrize('n_rows', R.LP_ROWS)
@pytest.mark.parametrize('n_layers', R.LP_LAYERS)
def test_layer_params_reduce(gpu_device, n_layers, n_rows):
    st, c = current_stream(gpu_device), 4
    wq, bq, wk = _weights(c, gpu_device)
    slab = torch.randn(n_rows, c * c + c, generator=torch.Generator().manual_seed(n_rows)).to(gpu_device)
    scratch, grads = torch.empty(32 * (c * c + c), device=gpu_device), torch.empty(2 * c * c + 2 * c, device=gpu_device)
    for case in (k for k in R.LP_CASES if k['L'] == n_layers and k['n'] == n_rows):
        inp = R.lp_make(case)
        partials = inp['partials'].to(gpu_device)
        obuf, out = _guarded(2 * n_layers, gpu_device)
        rbuf, ride = _guarded(2 * n_layers, gpu_device)
        assert lib().gadapt_layer_params_reduce(ptr(partials), n_rows, n_layers, case['want'], ptr(out), st) == 0
        assert lib().gadapt_slab_reduce_coeffs_backward(ptr(slab), n_rows, ptr(scratch), ptr(wq), ptr(bq), ptr(wk), *(ptr(v) for v in _bucket_views(grads, c)),
                                                        c, st, ptr(partials), n_layers, case['want'], ptr(ride)) == 0
        torch.cuda.synchronize()
        assert _guards_intact(obuf) and _guards_intact(rbuf)
        _judge(R.LAYER_PARAMS, case, inp, dict(d_layer_params=out.view(2, n_layers)))
        assert torch.equal(out, ride), case['id']
        if not case['want']:
            assert bool((out[n_layers:] == 0).all())


# ------------------------------------------------------------------------------------------------ 3. step tail on dense slabs
def _tail(fn, slab, n_rows, scratch, param, grad, m, v, state, wd, gs, a_out, p0_out, partials, loss, c, st):
    return fn(ptr(slab), n_rows, ptr(scratch), ptr(param), ptr(grad), ptr(m), ptr(v), R.ADAM_LR, 0.9, 0.999, R.ADAM_EPS, wd, ptr(state), gs,
              ptr(a_out), ptr(p0_out), ptr(partials), 0 if partials is None else partials.numel(), ptr(loss), R.LOSS_COUNT, c, st)


@pytest.mark.parametrize('weight_decay', [0.0, 1e-2])
@pytest.mark.parametrize('n_rows', [1, 65, 512])
@pytest.mark.parametrize('c', R.C_ALL)
def test_step_tail_is_its_three_parts(gpu_device, c, n_rows, weight_decay):
    st, row, npar, gs = current_stream(gpu_device), c * c + c, 2 * c * c + 2 * c, 0.5
    gen = torch.Generator().manual_seed(1000 * c + n_rows)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(gpu_device)
    slab, partials = rnd(n_rows, row), rnd(300).abs()
    param0, m0, v0 = 0.1 * rnd(npar), 0.01 * rnd(npar), (0.01 * rnd(npar)) ** 2
    scratch = torch.empty(32 * row, device=gpu_device)
    nan = lambda n: torch.full((n,), NAN, device=gpu_device)
    adam = lambda param, grad, m, v, state: lib().gadapt_adam_step_dev(ptr(param), ptr(grad), ptr(m), ptr(v), npar, R.ADAM_LR, 0.9, 0.999, R.ADAM_EPS,
                                                                         weight_decay, ptr(state), gs, st)

    # the whole tail, two steps in a row, against its parts run one by one from the same state
    param, m, v = param0.clone(), m0.clone(), v0.clone()
    state = torch.zeros(2, dtype=torch.int32, device=gpu_device)
    steps = []
    for step in range(2):
        before = [t.clone() for t in (param, m, v, state)]
        grad, a_out, p0_out, loss = nan(npar), nan(c * c), nan(c), nan(1)
        assert _tail(lib().gadapt_step_tail, slab, n_rows, scratch, param, grad, m, v, state, weight_decay, gs, a_out, p0_out, partials, loss, c, st) == 0
        torch.cuda.synchronize()
        bp, bm, bv, bstate = (t.clone() for t in before)           # (the parts below advance these copies)
        want_grad = nan(npar)
        assert lib().gadapt_slab_reduce_coeffs_backward(ptr(slab), n_rows, ptr(scratch), *(ptr(t) for t in _bucket_views(bp, c)[:3]),
                                                        *(ptr(t) for t in _bucket_views(want_grad, c)), c, st, None, 0, 0, None) == 0
        assert adam(bp, want_grad, bm, bv, bstate) == 0
        want_a, want_p0 = nan(c * c), nan(c)
        assert lib().gadapt_coeffs_forward(*(ptr(t) for t in _bucket_views(bp, c)[:3]), ptr(want_a), ptr(want_p0), c, st) == 0
        torch.cuda.synchronize()
        for name, w, g in (('grad', want_grad, grad), ('param', bp, param), ('m', bm, m), ('v', bv, v), ('state', bstate, state), ('a', want_a, a_out),
                           ('p0', want_p0, p0_out)):
            assert not torch.isnan(g.float()).any() and torch.equal(w, g), (step, name, (w.float() - g.float()).abs().max().item())
        assert state.tolist() == [step + 1, 0] and not torch.isnan(loss).any()
        steps.append(dict(grad=grad, before=before, param=param.clone(), m=m.clone(), v=v.clone(), loss=loss))
    assert not torch.equal(steps[0]['param'], param0) and not torch.equal(steps[1]['param'], steps[0]['param'])

    # gradient only: nothing but the flat gradient and the loss is written
    for step in range(2):
        bp, bm, bv, bstate = steps[step]['before']
        param, state = bp.clone(), bstate.clone()
        grad, a_out, p0_out, loss = nan(npar), nan(c * c), nan(c), nan(1)
        assert _tail(lib().gadapt_step_tail, slab, n_rows, scratch, param, grad, None, None, state, weight_decay, gs, a_out, p0_out, partials, loss, c, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(grad, steps[step]['grad']) and torch.equal(loss, steps[step]['loss'])
        assert torch.equal(param, bp) and torch.equal(state, bstate) and torch.isnan(a_out).all() and torch.isnan(p0_out).all()
        # gradient given: the Adam half and the coefficients
        param, m, v, state = (t.clone() for t in (bp, bm, bv, bstate))
        a_out, p0_out, grad_in = nan(c * c), nan(c), grad.clone()
        assert _tail(lib().gadapt_step_tail, None, 0, None, param, grad_in, m, v, state, weight_decay, gs, a_out, p0_out, None, None, c, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(grad_in, grad) and state.tolist() == [step + 1, 0]
        for name in ('param', 'm', 'v'):
            assert torch.equal(dict(param=param, m=m, v=v)[name], steps[step][name]), (step, name)
        want_a, want_p0 = nan(c * c), nan(c)
        assert lib().gadapt_coeffs_forward(*(ptr(t) for t in _bucket_views(param, c)[:3]), ptr(want_a), ptr(want_p0), c, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(a_out, want_a) and torch.equal(p0_out, want_p0)


@pytest.mark.parametrize('n', [1, 7, 256, 1025, 4096])
def test_step_tail_loss_partials(gpu_device, n):
    st, c = current_stream(gpu_device), 4
    slab, scratch = torch.zeros(3, c * c + c, device=gpu_device), torch.empty(32 * (c * c + c), device=gpu_device)
    param, grad = torch.zeros(2 * c * c + 2 * c, device=gpu_device), torch.empty(2 * c * c + 2 * c, device=gpu_device)
    for case in (k for k in R.LOSSP_CASES if k['n'] == n):
        inp = R.lossp_make(case)
        pbuf, partials = _guarded(n, gpu_device)
        partials.copy_(inp['partials'])
        lbuf, loss = _guarded(1, gpu_device)
        assert _tail(lib().gadapt_step_tail, slab, 3, scratch, param, grad, None, None, None, 0.0, 1.0, None, None, partials, loss, c, st) == 0
        torch.cuda.synchronize()
        assert _guards_intact(lbuf)
        _judge(R.LOSS_PARTIALS, case, inp, dict(loss=loss[0]))


# ------------------------------------------------------------------------------------------------ 4. Adam
@pytest.mark.parametrize('n', sorted({k['n'] for k in R.ADAM_CASES}))
@pytest.mark.parametrize('entry', ['adam_step', 'adam_step_dev'])
def test_adam(gpu_device, entry, n):
    st = current_stream(gpu_device)
    early = {}
    for case in (k for k in R.ADAM_CASES if k['n'] == n):
        inp, t, b = R.adam_make(case), case['t'], case['betas']
        bufs = {k: _guarded(n, gpu_device) for k in ('p', 'm', 'v')}
        for k, (_, view) in bufs.items():
            view.copy_(inp[k])
        p, m, v = (bufs[k][1] for k in ('p', 'm', 'v'))
        grad = inp['g'].to(gpu_device)
        if entry == 'adam_step':
            assert lib().gadapt_adam_step(ptr(p), ptr(grad), ptr(m), ptr(v), n, R.ADAM_LR, b[0], b[1], R.ADAM_EPS, case['wd'], t, case['gs'], st) == 0
        else:
            sbuf, state = _guarded(2, gpu_device, torch.int32)
            state.copy_(torch.tensor([t - 1, 0], dtype=torch.int32))
            assert lib().gadapt_adam_step_dev(ptr(p), ptr(grad), ptr(m), ptr(v), n, R.ADAM_LR, b[0], b[1], R.ADAM_EPS, case['wd'], ptr(state), case['gs'], st) == 0
            torch.cuda.synchronize()
            assert state.tolist() == [t, 0] and _guards_intact(sbuf), case['id']
        torch.cuda.synchronize()
        assert all(_guards_intact(buf) for buf, _ in bufs.values()), case['id']        # elements beyond n untouched
        assert torch.equal(grad.cpu(), inp['g'])
        ref = R.adam_ref(case, inp)
        _judge(R.ADAM, case, inp, dict(p=p, m=m, v=v), ref, tag='/' + entry)
        if case['grads'] == 'zero':
            assert torch.equal(p.cpu(), inp['p']) and not m.any() and not v.any()
        if case['grads'] == 'normal' and ref['delta'].abs().min() > 0:
            # what is left of |p_new - ref| after the rounding of the last subtraction, in units of rho(t) |delta_ref|
            over = ((p.cpu().to(F64) - ref['p']).abs() - U * p.cpu().to(F64).abs()).clamp_min(0) / (R.adam_rho(case) * ref['delta'].abs())
            early[t] = max(early.get(t, 0.0), float(over.max()))
    for t, frac in sorted(early.items()):
        print(f"[step-kernels-adam] {entry} n={n} t={t} rho={R.adam_rho(dict(t=t, betas=R.ADAM_BETAS[0], wd=0.0, gs=1.0)) / U:.1f}u "
              f"worst (|p-ref| - u|p|)+ / (rho |delta|) over both beta pairs = {frac:.4f}")


# ------------------------------------------------------------------------------------------------ 5. loss and seed
@pytest.mark.parametrize('n_rows', R.LOSS_ROWS)
@pytest.mark.parametrize('d', R.LOSS_D)
def test_loss_forward(gpu_device, d, n_rows):
    st = current_stream(gpu_device)
    scratch = torch.zeros(lib().gadapt_loss_scratch_floats(), device=gpu_device)
    for case in (k for k in R.LOSS_CASES if k['d'] == d and k['n'] == n_rows):
        inp = R.loss_make(case)
        ref = R.loss_ref(case, inp)
        target = inp['target'].to(gpu_device)
        for stride in sorted({d, 4, 64} - set(range(d))):
            pred = torch.full((n_rows, stride), NAN, device=gpu_device)
            pred[:, :d] = inp['pred'].to(gpu_device)
            runs = []
            for _ in range(2 if case['kind'] == 'random' else 1):
                sbuf, seed = _guarded(n_rows * d, gpu_device)
                lbuf, loss = _guarded(1, gpu_device)
                assert lib().gadapt_loss_forward(ptr(pred), stride, ptr(target), n_rows, d, case['l1'], ptr(seed), ptr(loss), ptr(scratch), st) == 0
                torch.cuda.synchronize()
                assert _guards_intact(sbuf) and _guards_intact(lbuf)
                assert scratch[0].item() == 0, "the ticket counter comes back to zero"
                runs.append((seed, loss))
            seed, loss = runs[0]
            _judge(R.LOSS, case, inp, dict(loss=loss[0], seed=seed.view(n_rows, d)), ref, tag=f'/stride{stride}')
            assert bool((seed.view(n_rows, d)[(inp['pred'] == inp['target']).to(gpu_device)] == 0).all())
            if len(runs) == 2:
                assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert bool((scratch.view(torch.int32)[0] == 0))


@pytest.mark.parametrize('l1', [0, 1], ids=['mse', 'l1'])
@pytest.mark.parametrize('d,n_rows', [(2, 257), (3, 32769), (5, 1000)])
def test_loss_wrappers(gpu_device, d, n_rows, l1):
    case = dict(id=f'wrap-d{d}-n{n_rows}-{l1}', d=d, n=n_rows, l1=l1, kind='half_equal', row=None)
    inp = R.loss_make(case)
    ref = R.loss_ref(case, inp)
    fn = l1_loss if l1 else mse_loss
    target = inp['target'].to(gpu_device)
    for upstream in (None, 0.5, 0.37):
        x = torch.zeros(n_rows, 64, device=gpu_device)
        x[:, :d] = inp['pred'].to(gpu_device)
        x.requires_grad_()
        loss = fn(x[:, :d], target)                                  # the strided view of GNN.py:299
        if upstream is None:
            loss.backward(gradient=unit_gradient(gpu_device))
        else:
            loss.backward(gradient=torch.tensor(upstream, device=gpu_device))
        scale = 1.0 if upstream is None else R.f32(upstream)
        _judge(R.LOSS, case, inp, dict(loss=loss.detach()), ref, tag=f'/upstream{upstream}')
        # the unit gradient hands the seed on as it is, a power of two scales it exactly, anything else is one more rounding
        ok, ratio = R.inside(x.grad[:, :d], ref['seed'] * scale, gamma(4 if upstream == 0.37 else 3) * (ref['seed'] * scale).abs() + R.TINY)
        print(f"[step-kernels] loss_wrapper {case['id']}/upstream{upstream} seed {ratio:.4f}")
        assert ok and not x.grad[:, d:].any()


@pytest.mark.parametrize('d,c', [(d, c) for d in R.LOSS_D for c in R.SEED_C if d <= c])
def test_mesh_loss_seed(gpu_device, d, c):
    st = current_stream(gpu_device)
    for case in (k for k in R.SEED_CASES if k['d'] == d and k['c'] == c):
        n, inp = case['n'], R.seed_make(case)
        x_top, target = inp['x_top'].to(gpu_device), inp['target'].to(gpu_device)
        xbuf, x_phys = _guarded(n * d, gpu_device)
        gbuf, g_top = _guarded(n * c, gpu_device)
        lbuf, loss = _guarded(1, gpu_device)
        loss.fill_(R.SEED_L0)
        assert lib().gadapt_mesh_loss_seed(ptr(x_top), ptr(target), ptr(x_phys), ptr(g_top), ptr(loss), n, d, c, case['l1'], R.SEED_GS, st) == 0
        torch.cuda.synchronize()
        assert _guards_intact(xbuf) and _guards_intact(gbuf) and _guards_intact(lbuf)
        _judge(R.MESH_LOSS_SEED, case, inp, dict(x_phys=x_phys.view(n, d), g_top=g_top.view(n, c), loss_out=loss[0]))
        if case['kind'] == 'all_equal':
            assert loss.item() == R.SEED_L0 and not g_top.any()


# ------------------------------------------------------------------------------------------------ 6. encoder
def _encode_features(inp, x0, n, c, dev, coeffs=None):
    d = _to(inp, dev)
    head = (ptr(d['x_comp']), inp['x_comp'].shape[1], ptr(d['f']), ptr(d['uu']), ptr(d['w']), ptr(d['b']), ptr(x0), n, c)
    if coeffs is None:
        return lib().gadapt_encode_features(*head, current_stream(dev))
    return lib().gadapt_encode_features_coeffs(*head, *coeffs, current_stream(dev))


@pytest.mark.parametrize('case', R.ENC_CASES, ids=lambda c: c['id'])
def test_encoder(gpu_device, case):
    n, c = case['n'], case['c']
    inp = R.enc_make(case)
    feats = R.enc_feats(inp).contiguous().to(gpu_device)
    w, b = inp['w'].to(gpu_device), None if inp['b'] is None else inp['b'].to(gpu_device)
    lbuf, lin = _guarded(n * c, gpu_device)
    assert lib().gadapt_encode_linear(ptr(feats), ptr(w), ptr(b), ptr(lin), n, feats.shape[1], c, current_stream(gpu_device)) == 0
    torch.cuda.synchronize()
    assert _guards_intact(lbuf)                                       # one float beyond x0 (and in front of it) stays NaN
    ref = R.enc_ref(case, inp)
    _judge(R.ENCODER, case, inp, dict(x0=lin.view(n, c)), ref, tag='/linear')
    if not case['linear']:
        fbuf, x0 = _guarded(n * c, gpu_device)
        assert _encode_features(inp, x0, n, c, gpu_device) == 0
        torch.cuda.synchronize()
        assert _guards_intact(fbuf)
        _judge(R.ENCODER, case, inp, dict(x0=x0.view(n, c)), ref, tag='/features')
        assert torch.equal(x0, lin)


@pytest.mark.parametrize('c_conv', [4, 64, 128])
@pytest.mark.parametrize('case', [k for k in R.ENC_CASES if not k['linear'] and k['c'] in (8, 64, 256) and k['n'] >= 4 * (1024 // k['c']) + 1], ids=lambda c: c['id'])
def test_encode_features_coeffs(gpu_device, case, c_conv):
    n, c, st = case['n'], case['c'], current_stream(gpu_device)
    inp = R.enc_make(case)
    ccase = dict(id=f'coeffs-C{c_conv}-random', c=c_conv, kind='random')
    cinp = R.coeffs_make(ccase)
    wq, bq, wk = (cinp[k].to(gpu_device) for k in ('wq', 'bq', 'wk'))
    fbuf, x0 = _guarded(n * c, gpu_device)
    cbuf, x0c = _guarded(n * c, gpu_device)
    abuf, ap = _guarded(c_conv * c_conv + c_conv, gpu_device)
    wbuf, want = _guarded(c_conv * c_conv + c_conv, gpu_device)
    a, p0 = ap[:c_conv * c_conv], ap[c_conv * c_conv:]
    assert _encode_features(inp, x0, n, c, gpu_device) == 0
    assert _encode_features(inp, x0c, n, c, gpu_device, coeffs=(ptr(wq), ptr(bq), ptr(wk), ptr(a), ptr(p0), c_conv)) == 0
    assert lib().gadapt_coeffs_forward(ptr(wq), ptr(bq), ptr(wk), ptr(want[:c_conv * c_conv]), ptr(want[c_conv * c_conv:]), c_conv, st) == 0
    torch.cuda.synchronize()
    assert all(_guards_intact(t) for t in (fbuf, cbuf, abuf, wbuf))
    assert not torch.isnan(x0c).any() and torch.equal(x0c, x0) and not torch.isnan(ap).any() and torch.equal(ap, want)
    _judge(R.ENCODER, case, inp, dict(x0=x0c.view(n, c)), tag=f'/coeffs{c_conv}')
    res = R.COEFFS.check(ccase, cinp, dict(a=a.view(c_conv, c_conv), p0=p0))
    assert all(ok for ok, _ in res.values()), res


# ------------------------------------------------------------------------------------------------ 7. copies
@pytest.mark.parametrize('case', R.PAD_CASES, ids=lambda c: c['id'])
def test_pad_columns(gpu_device, case):
    n, d, c = case['n'], case['d'], case['c']
    inp = R.pad_make(case)
    gbuf, g_top = _guarded(n * c, gpu_device)
    assert lib().gadapt_pad_columns(ptr(inp['g_phys'].to(gpu_device)), ptr(g_top), n, d, c, current_stream(gpu_device)) == 0
    torch.cuda.synchronize()
    assert _guards_intact(gbuf)
    _judge(R.PAD, case, inp, dict(g_top=g_top.view(n, c)))
    assert torch.equal(g_top.view(n, c).cpu(), torch.nn.functional.pad(inp['g_phys'], (0, c - d)))


def _gather(src, dst, idx, dev):
    k = len(src)
    return lib().gadapt_gather_fields(k, (C.c_void_p * k)(*[s.data_ptr() for s in src]), (C.c_void_p * k)(*[t.data_ptr() for t in dst]),
                                      (C.c_int64 * k)(*[s[0].numel() for s in src]), ptr(idx), int(idx.numel()), current_stream(dev))


@pytest.mark.parametrize('case', R.GATHER_CASES, ids=lambda c: c['id'])
def test_gather_fields(gpu_device, case):
    inp = R.gather_make(case)
    idx = inp['idx'].to(gpu_device)
    src = [s.to(gpu_device) for s in inp['src']]
    out = [_guarded(idx.numel() * s.shape[1], gpu_device) for s in src]
    assert _gather(src, [view for _, view in out], idx, gpu_device) == 0
    torch.cuda.synchronize()
    assert all(_guards_intact(buf) for buf, _ in out)
    _judge(R.GATHER, case, inp, {f'dst{k}': view.view(idx.numel(), -1) for k, (_, view) in enumerate(out)})
    for s, (_, view) in zip(src, out):
        assert torch.equal(view.view(idx.numel(), -1), torch.index_select(s, 0, idx))


def test_gather_fields_unaligned_source_and_too_many_fields(gpu_device):
    row, idx = 4100, torch.tensor([3, 0, 3, 1], device=gpu_device)
    storage = torch.randn(R.GATHER_SAMPLES * row + 1, device=gpu_device)
    src = storage[1:].view(R.GATHER_SAMPLES, row)                     # row length a multiple of 4, rows 4 bytes off a 16-byte line
    assert src.data_ptr() % 16 == 4 and row % 4 == 0
    buf, dst = _guarded(idx.numel() * row, gpu_device)
    assert _gather([src], [dst], idx, gpu_device) == 0
    torch.cuda.synchronize()
    assert _guards_intact(buf) and torch.equal(dst.view(idx.numel(), row), torch.index_select(src, 0, idx))
    nine = [torch.randn(R.GATHER_SAMPLES, 4, device=gpu_device) for _ in range(9)]
    outs = [torch.full((idx.numel(), 4), NAN, device=gpu_device) for _ in range(9)]
    assert _gather(nine, outs, idx, gpu_device) == BADARG
    assert b'gather_fields' in lib().gadapt_last_error()
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all() for o in outs)                    # nothing was launched
