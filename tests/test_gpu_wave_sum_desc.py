"""`wave_sum_desc` (csrc/gadapt_common.inc): the wave sum of the slab partials on DPP and lane-swap steps against the xor butterfly
32, 16, .., 1 on `__shfl_xor` that defines those partials, through `gadapt_debug_wave_sum_desc` - one small kernel that runs both on the
same registers and writes what every lane ends with.  The claim is equality of bits in all 64 lanes, so the comparison is `torch.equal`
on the int32 patterns, for 1, 20 and 22 values per lane (a single value: nothing separates a stage from the next; 20 and 22: the two
counts the kernels use) and one and four waves per workgroup.

Inputs, one per wave slot in turn: random values over 12 decades of magnitude with both signs; a single non-zero lane (0, 63); lanes
16..31 only (one half of a row pair); one row of 16 lanes; signed zeros alone (the sum of -0 and -0 keeps its sign) and mixed; denormals
(alone, and beside normal numbers that absorb them); +inf / -inf among finite values (sums that are inf, and NaN where both signs meet)."""
import pytest
import torch

from g_adaptivity_amd._native import current_stream, lib, ptr

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]                    # no graph: nothing for the kernel choice to change
PATTERNS = ['wide-exponents', 'lane-0', 'lane-63', 'lanes-16-31', 'row-2', 'zeros', 'denormals', 'infinities']


def _wave(kind, n_values, gen):
    """[64, n_values] fp32 (CPU)."""
    mag = 10.0 ** (torch.rand(64, n_values, generator=gen) * 12 - 6)
    sign = torch.where(torch.rand(64, n_values, generator=gen) < 0.5, -1.0, 1.0)
    x = (mag * sign).float()
    lanes = torch.arange(64).unsqueeze(1).expand(64, n_values)
    if kind == 'wide-exponents':
        return x
    if kind == 'lane-0':
        return torch.where(lanes == 0, x, torch.zeros_like(x))
    if kind == 'lane-63':
        return torch.where(lanes == 63, x, torch.zeros_like(x))
    if kind == 'lanes-16-31':
        return torch.where((lanes >= 16) & (lanes < 32), x, torch.zeros_like(x))
    if kind == 'row-2':
        return torch.where((lanes >= 32) & (lanes < 48), x, torch.zeros_like(x))
    if kind == 'zeros':                                                     # column 0: every lane -0; the others: +0 / -0 mixed, a few values
        z = torch.where(torch.rand(64, n_values, generator=gen) < 0.5, -0.0, 0.0).float()
        z = torch.where(torch.rand(64, n_values, generator=gen) < 0.05, x, z)
        z[:, 0] = -0.0
        return z
    if kind == 'denormals':                                                 # column 0: denormals alone; the others: some lanes normal
        tiny = (torch.randint(1, 1 << 20, (64, n_values), generator=gen).int()).view(torch.float32) * sign
        d = torch.where(torch.rand(64, n_values, generator=gen) < 0.2, x * 1e-30, tiny)
        d[:, 0] = tiny[:, 0]
        return d
    if kind == 'infinities':
        r = torch.rand(64, n_values, generator=gen)
        inf = torch.full_like(x, float('inf'))
        y = torch.where(r < 0.03, inf, torch.where(r < 0.06, -inf, x))
        if n_values > 1:
            y[:, 1] = torch.where(lanes[:, 1] == 37, inf[:, 1], x[:, 1])     # one +inf, no -inf: the sum is +inf in every lane
        return y
    raise AssertionError(kind)


@pytest.mark.parametrize("n_waves", [1, 4])
@pytest.mark.parametrize("n_values", [1, 20, 22])
def test_wave_sum_desc_is_the_xor_butterfly_bit_for_bit(gpu_device, n_values, n_waves):
    gen = torch.Generator().manual_seed(100 * n_values + n_waves)
    st = current_stream(gpu_device)
    for first in range(0, len(PATTERNS), n_waves):                          # every pattern, n_waves of them per launch
        kinds = [PATTERNS[(first + w) % len(PATTERNS)] for w in range(n_waves)]
        x = torch.stack([_wave(k, n_values, gen) for k in kinds]).contiguous()
        xd = x.to(gpu_device)
        shfl, desc = torch.full_like(xd, 7.0), torch.full_like(xd, 9.0)
        assert lib().gadapt_debug_wave_sum_desc(ptr(xd), ptr(shfl), ptr(desc), n_waves, n_values, st) == 0
        torch.cuda.synchronize()
        a, b = shfl.view(torch.int32).cpu(), desc.view(torch.int32).cpu()
        bad = (a != b).nonzero()[:4].tolist()
        assert torch.equal(a, b), (kinds, bad)
        # the butterfly itself is the definition; that it IS a sum of the wave, the same in all 64 lanes, anchors the kernel's indexing
        s = shfl.cpu()
        assert ((s.view(torch.int32) == s[:, :1].contiguous().view(torch.int32)) | torch.isnan(s)).all(), kinds
        want = x.double().sum(dim=1)
        fin = torch.isfinite(want)
        got = s[:, 0].double()
        tol = 64 * 2.0 ** -24 * x.double().abs().sum(dim=1)
        assert ((got - want).abs()[fin] <= tol[fin]).all(), kinds
        assert torch.equal(got[~fin & ~torch.isnan(want)], want[~fin & ~torch.isnan(want)]) and torch.isnan(got[torch.isnan(want)]).all(), kinds


def test_wave_sum_desc_entry_point_checks_its_arguments(gpu_device):
    x = torch.zeros(64, 3, device=gpu_device)
    st = current_stream(gpu_device)
    assert lib().gadapt_debug_wave_sum_desc(ptr(x), ptr(x), ptr(x), 1, 3, st) != 0 and b'wave_sum_desc' in lib().gadapt_last_error()
    assert lib().gadapt_debug_wave_sum_desc(ptr(x), ptr(x), ptr(x), 17, 1, st) != 0
    assert lib().gadapt_debug_wave_sum_desc(None, ptr(x), ptr(x), 1, 1, st) != 0
