"""`wave_sum_scatter` (csrc/gadapt_common.inc): the wave sum the narrow block kernels run on their 20 slab partials - every exchange
hands over half of the values, so each total ends in ONE lane - against `wave_sum_desc`, through `gadapt_debug_wave_sum_scatter`: one
small kernel that runs both on the same 20 values per lane.  The claim is that the total a documented lane ends with has the bits
`wave_sum_desc` leaves in lane 0 for that entry, so the comparison is on int32 patterns; where +inf meets -inf both must be NaN (the
payload is not pinned).  The lane of every entry is restated here from the header's text (include/gadapt_hip.h) and compared with
what the kernel reports, so a total read from another lane than the documented one fails.

Inputs, one per wave slot in turn (those of tests/test_gpu_wave_sum_desc.py, whose generator this reuses): random values over 12
decades with both signs; a single non-zero lane (0, 31, 32, 63); lanes 16..31 only; one row of 16 lanes; signed zeros; denormals;
infinities.  One wave and four waves per workgroup."""
import pytest
import torch

from g_adaptivity_amd._native import current_stream, lib, ptr
from test_gpu_wave_sum_desc import _wave

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]                    # no graph: nothing for the kernel choice to change
PATTERNS = ['wide-exponents', 'lane-0', 'lane-31', 'lane-32', 'lane-63', 'lanes-16-31', 'row-2', 'zeros', 'denormals', 'infinities']


def _documented_entry(lane):
    """The entry whose total lane `lane` holds (-1: none), as include/gadapt_hip.h states it."""
    base, c = 10 * (lane >> 5) + 5 * ((lane >> 4) & 1), lane & 15
    if c == 1:
        return base + 4
    return base + {0: 0, 4: 2, 8: 1, 12: 3}[c] if c in (0, 4, 8, 12) else -1


def _pattern(kind, gen):
    if kind in ('lane-31', 'lane-32'):
        x = _wave('wide-exponents', 20, gen)
        lanes = torch.arange(64).unsqueeze(1).expand(64, 20)
        return torch.where(lanes == int(kind[5:]), x, torch.zeros_like(x))
    return _wave(kind, 20, gen)


def test_documented_lanes_hold_each_entry_once():
    entries = [_documented_entry(l) for l in range(64)]
    assert sorted(e for e in entries if e >= 0) == list(range(20))


@pytest.mark.parametrize("n_waves", [1, 4])
def test_wave_sum_scatter_totals_are_wave_sum_desc_bit_for_bit(gpu_device, n_waves):
    gen = torch.Generator().manual_seed(977 + n_waves)
    st = current_stream(gpu_device)
    want_entry = torch.tensor([_documented_entry(l) for l in range(64)], dtype=torch.int32)
    lanes_of = torch.tensor([int((want_entry == e).nonzero()[0, 0]) for e in range(20)])
    for first in range(0, len(PATTERNS), n_waves):                          # every pattern, n_waves of them per launch
        kinds = [PATTERNS[(first + w) % len(PATTERNS)] for w in range(n_waves)]
        x = torch.stack([_pattern(k, gen) for k in kinds]).contiguous()     # [n_waves, 64, 20]
        xd = x.to(gpu_device)
        desc = torch.full_like(xd, 9.0)
        scat = torch.full((n_waves, 64), 7.0, device=gpu_device)
        entry = torch.full((n_waves, 64), -5, dtype=torch.int32, device=gpu_device)
        assert lib().gadapt_debug_wave_sum_scatter(ptr(xd), ptr(desc), ptr(scat), ptr(entry), n_waves, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(entry.cpu(), want_entry.expand(n_waves, 64)), kinds      # the helper's own map is the documented one
        ref = desc.cpu()[:, 0, :]                                           # wave_sum_desc's lane-0 value of every entry  [n_waves, 20]
        got = scat.cpu()[:, lanes_of]                                       # the documented lane of every entry           [n_waves, 20]
        print(kinds, 'entries differing:', int((ref.view(torch.int32) != got.view(torch.int32)).sum()))
        both_nan = torch.isnan(ref) & torch.isnan(got)
        same = (ref.view(torch.int32) == got.view(torch.int32)) | both_nan
        assert same.all(), (kinds, (~same).nonzero()[:4].tolist())
        assert not torch.isnan(got[~torch.isnan(ref)]).any(), kinds
        if 'infinities' in kinds:                                           # +inf and -inf do meet in some entry: the NaN rule is exercised
            w = kinds.index('infinities')
            assert torch.isnan(ref[w]).any() and torch.isinf(ref[w]).any()


def test_wave_sum_scatter_entry_point_checks_its_arguments(gpu_device):
    x = torch.zeros(64, 20, device=gpu_device)
    st = current_stream(gpu_device)
    assert lib().gadapt_debug_wave_sum_scatter(ptr(x), ptr(x), ptr(x), ptr(x), 17, st) != 0 and b'wave_sum_scatter' in lib().gadapt_last_error()
    assert lib().gadapt_debug_wave_sum_scatter(None, ptr(x), ptr(x), ptr(x), 1, st) != 0
