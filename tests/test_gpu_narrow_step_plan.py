"""The plan of a narrow step is what runs (csrc/gadapt_narrow_plan.h, `gadapt_narrow_step_plan`; DESIGN.md "How a message-passing entry
point is put together"): one fused step through `FusedIteration` with the per-launch records on, under every combination of the four
launch-sequence switches.  Per kernel id (0 forward, 1 backward target pass, 2 backward source pass - `gadapt_profile_variants` lists
one id at a time) the recorded variants, in launch order, equal the ones derived from the plan's records, and the two reports of the
step (`fwd.top_ran`, `block_ran`) equal the plan's.  The plan is asked for as the step's two calls give their facts: the forward with a
target, the backward's buffers and - where the layer-0 launch computes them - the coefficients; the backward on the packed slab with
top_done as the forward reported it."""
import ctypes as C
import itertools

import pytest
import torch

from test_gpu_narrow_top_in_forward import _square
from g_adaptivity_amd import mse_loss
from g_adaptivity_amd._native import lib
from g_adaptivity_amd.training import FusedIteration

C_ = 64
HEAD, WORDS = 18, 13
SHARED, PACKED, TARGET, BUFFERS, COEFFS, TOP_DONE, MAY_BLOCK = 1, 2, 4, 8, 16, 32, 64
# (kernel id, variant) of a launch record by kind (include/gadapt_hip.h: the serialised plan; csrc/gadapt_internal.h: ProfScope - bit 0
# compact upstream gradient, bit 1 compact layer input, bit 2 head-only output, bit 3 [N,4] backward output, bit 5 several layers)
VARIANT = {0: lambda r: (0, 6), 1: lambda r: (0, 6), 2: lambda r: (0, 6 | 32), 3: lambda r: (1, 3 if r[10] else 2), 4: lambda r: (2, 8),
           5: lambda r: (1, 2), 6: lambda r: (1, 2), 7: lambda r: (1, 2 | 32)}


def _plan(graph, layers, flags):
    out = (C.c_int32 * (HEAD + 39 * layers))()
    n = lib().gadapt_narrow_step_plan(graph.c_ref, C_, layers, flags, out, len(out))
    assert n >= HEAD, lib().gadapt_last_error()
    return out[:HEAD], [out[HEAD + WORDS * i: HEAD + WORDS * (i + 1)] for i in range((n - HEAD) // WORDS)]


def _recorded(kernel_id):
    out = (C.c_int * 64)()
    n = lib().gadapt_profile_variants(kernel_id, out, 64)
    assert 0 <= n < 64
    return out[:n]


@pytest.mark.gpu
@pytest.mark.one_dispatch
@pytest.mark.parametrize("layers", [3, 4, 6])
@pytest.mark.parametrize("mesh_n,batch,halo", [(16, 1, 32), (23, 7, 32), (64, 2, 64)], ids=['16x16-b1', '23x23-b7', '64x64-b2'])
def test_the_launches_of_a_fused_step_are_the_plans(gpu_device, mesh_n, batch, halo, layers, monkeypatch):
    model, optim, data = _square(gpu_device, mesh_n, batch, layers, monkeypatch)
    assert FusedIteration.eligible(model, optim, mse_loss, data, 'x_phys') is None
    it = FusedIteration(model, optim, mse_loss, data, 'x_phys')
    g = it.graph
    assert it.fwd.narrow and g.narrow_block_halo == halo and g.narrow_block_halo_source == halo
    assert (mesh_n, batch) != (16, 1) or g.num_nodes < 512                          # one partial tile
    assert (mesh_n, batch) != (23, 7) or g.num_nodes % 512 % 64 != 0                # ragged last tile
    it.refresh_coeffs()
    call = SHARED | PACKED | TARGET | BUFFERS | MAY_BLOCK | (COEFFS if it.fwd.in_forward else 0)
    setters = (lib().gadapt_debug_set_narrow_forward, lib().gadapt_debug_set_narrow_backward_fused, lib().gadapt_debug_set_narrow_top_in_forward,
               lib().gadapt_debug_set_narrow_backward_block)
    kinds = set()
    try:
        for sw in itertools.product((1, 2, 0), (1, 0), (1, 0), (1, 0)):
            for fn, v in zip(setters, sw):
                assert fn(v) == 0
            head, recs = _plan(g, layers, call)
            top_ran = head[6]
            if top_ran:                                                             # the backward call is told so
                head, recs_b = _plan(g, layers, call | TOP_DONE)
                assert recs_b[:head[1]] == recs[:head[1]] and head[6] == 1 and head[9] == 1
                recs = recs_b
            assert head[0] == 1 and len(recs) == head[1] + head[2]
            want = {k: [VARIANT[r[0]](r)[1] for r in recs if VARIANT[r[0]](r)[0] == k] for k in (0, 1, 2)}
            lib().gadapt_profile_reset(); lib().gadapt_profile_enable(1)
            it.run()
            torch.cuda.synchronize()
            got = {k: _recorded(k) for k in (0, 1, 2)}
            lib().gadapt_profile_enable(0)
            assert got == want, (sw, got, want)
            assert int(it.fwd.top_ran) == top_ran and it.block_ran.value == head[10], (sw, it.fwd.top_ran, it.block_ran.value, head)
            assert bool(torch.isfinite(it.loss))
            kinds |= {r[0] for r in recs}
    finally:
        lib().gadapt_profile_enable(0); lib().gadapt_profile_reset()
        for fn in setters:
            fn(1)
    # every launch kind ran somewhere in the sweep, and the default is the shortest sequence: groups both ways, T_{L-1} in the forward
    assert kinds == set(range(8))
    head, recs = _plan(g, layers, call | TOP_DONE)
    assert (head[3], head[6], head[7], head[9], head[10]) == (2, 1, 2, 1, 1)
    assert [r[0] for r in recs] == [2] * (1 if layers <= 4 else 2) + [7] * (1 if layers <= 4 else 2)
