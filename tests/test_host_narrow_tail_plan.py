"""The entry map of the narrow route's spread step tail (csrc/gadapt_tail_plan.h, step_tail_narrow_spread_kernel), on
the host.  `gadapt_narrow_tail_entry_host` / `gadapt_narrow_tail_owner_host` are the arithmetic the kernel and its launcher use: every
entry of the flat bucket [Wq | bq | Wk | bk] (hidden 64: 8320 entries) is owned by exactly one (workgroup, thread, slot), a workgroup owns
whole rows, so every operand of an entry's chain rule belongs to the workgroup that owns the entry, the last workgroup's short row count
is handled, and one ticket is taken per parameter workgroup."""
import ctypes as C

from g_adaptivity_amd import _native

C_ = 64
C2 = C_ * C_
NPAR = 2 * C2 + 2 * C_
WQ, BQ, WK, BK = 0, C2, C2 + C_, 2 * C2 + C_          # offsets of the flat bucket's parts


def _plan(has_loss):
    out = (C.c_int32 * 6)()
    assert _native.lib().gadapt_narrow_tail_plan_host(has_loss, out) == 0
    return dict(zip(('rows', 'threads', 'wgs', 'slots', 'grid', 'tickets'), out))


def _entry(wg, thread, slot):
    out = (C.c_int32 * 3)()
    assert _native.lib().gadapt_narrow_tail_entry_host(wg, thread, slot, out) == 0
    return tuple(out)


def _owner(e):
    out = (C.c_int32 * 3)()
    assert _native.lib().gadapt_narrow_tail_owner_host(e, out) == 0
    return tuple(out)


def _all_entries():
    """entry -> [(wg, thread, slot, ri, k)] over every slot of the launch"""
    p = _plan(0)
    owned = {}
    for wg in range(p['wgs']):
        for thread in range(p['threads']):
            for slot in range(p['slots']):
                e, ri, k = _entry(wg, thread, slot)
                if e >= 0:
                    owned.setdefault(e, []).append((wg, thread, slot, ri, k))
    return p, owned


def test_geometry():
    p = _plan(0)
    assert 1 <= p['rows'] <= C_ and p['threads'] % 256 == 0 and 256 <= p['threads'] <= 1024
    assert p['wgs'] == -(-C_ // p['rows'])
    assert p['slots'] in (1, 2) and p['slots'] == -(-p['rows'] * (2 * C_ + 2) // p['threads'])     # one or two entries per thread


def test_every_entry_has_exactly_one_owner():
    p, owned = _all_entries()
    assert sorted(owned) == list(range(NPAR))
    assert all(len(v) == 1 for v in owned.values())
    for e, ((wg, thread, slot, ri, k),) in owned.items():
        assert _owner(e) == (wg, thread, slot), e
        r = wg * p['rows'] + ri                                  # the place in the row says which part of the bucket the entry is
        want = WQ + r * C_ + k if k < C_ else (BQ + r if k == C_ else (WK + r * C_ + k - C_ - 1 if k < 2 * C_ + 1 else BK + r))
        assert e == want and 0 <= ri < p['rows'] and 0 <= k <= 2 * C_ + 1, (e, wg, ri, k)


def test_chain_rule_operands_belong_to_the_owning_workgroup():
    p, owned = _all_entries()
    wg_of = {e: v[0][0] for e, v in owned.items()}
    for r in range(C_):
        wq4 = [WQ + r * C_ + c for c in range(4)]
        wk4 = [WK + r * C_ + o for o in range(4)]
        for c in range(C_):                                      # d Wq[r][c] = sum_o Wk[r][o] dA[o][c]
            assert all(wg_of[x] == wg_of[WQ + r * C_ + c] for x in wk4)
        assert all(wg_of[x] == wg_of[BQ + r] for x in wk4)       # d bq[r] = sum_o Wk[r][o] dp0[o]
        for o in range(C_):                                      # d Wk[r][o] = sum_c Wq[r][c] dA[o][c] + bq[r] dp0[o]
            assert all(wg_of[x] == wg_of[WK + r * C_ + o] for x in wq4 + [BQ + r])
        # a workgroup owns the whole row: Wq[r][:], bq[r], Wk[r][:], bk[r]
        row = [WQ + r * C_ + c for c in range(C_)] + [BQ + r] + [WK + r * C_ + o for o in range(C_)] + [BK + r]
        assert len({wg_of[x] for x in row}) == 1 and wg_of[row[0]] == r // p['rows']


def test_the_last_workgroup_may_be_short():
    lib = _native.lib()
    p, owned = _all_entries()
    rows = [lib.gadapt_narrow_tail_rows_host(wg) for wg in range(p['wgs'])]
    assert sum(rows) == C_ and all(n == p['rows'] for n in rows[:-1]) and 1 <= rows[-1] <= p['rows']
    assert rows[-1] == C_ - p['rows'] * (p['wgs'] - 1)
    per_wg = [0] * p['wgs']
    for v in owned.values():
        per_wg[v[0][0]] += 1
    assert per_wg == [n * (2 * C_ + 2) for n in rows]             # 130 entries per owned row, none for a row that is not there
    last = p['wgs'] - 1
    live = [_entry(last, t, s) for t in range(p['threads']) for s in range(p['slots'])]
    assert all(e < 0 or ri < rows[-1] for e, ri, k in live)
    assert lib.gadapt_narrow_tail_rows_host(-1) == -1 and lib.gadapt_narrow_tail_rows_host(p['wgs']) == -1


def test_one_ticket_per_parameter_workgroup():
    without, with_loss = _plan(0), _plan(1)
    assert without['tickets'] == without['wgs'] == without['grid']
    assert with_loss['tickets'] == with_loss['wgs'] == without['wgs'] and with_loss['grid'] == with_loss['wgs'] + 1   # the loss workgroup takes none


def test_bad_arguments_are_refused():
    lib = _native.lib()
    p = _plan(0)
    out = (C.c_int32 * 3)()
    assert lib.gadapt_narrow_tail_plan_host(0, None) == -1
    for args in ((-1, 0, 0), (p['wgs'], 0, 0), (0, -1, 0), (0, p['threads'], 0), (0, 0, -1), (0, 0, p['slots'])):
        assert lib.gadapt_narrow_tail_entry_host(*args, out) == -1, args
    assert lib.gadapt_narrow_tail_entry_host(0, 0, 0, None) == -1
    assert lib.gadapt_narrow_tail_owner_host(-1, out) == -1 and lib.gadapt_narrow_tail_owner_host(NPAR, out) == -1
    assert lib.gadapt_narrow_tail_owner_host(0, None) == -1
