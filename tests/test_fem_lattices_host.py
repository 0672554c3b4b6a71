"""Host side of the 2-D FEM tail on other evaluation lattices (tests/fem_lattices.py): conditions on the inputs and on the
reference alone, and what the windowed launch plan refuses at the lattice limit.  No GPU.

    axes         every axis is one `fem.lattice_axes` takes; A, B and C keep 1e-3 away from 0 and 1 (the mesh boundary is a
                 discontinuity of sol: a point within rounding of it may be classed differently in fp32 and fp64)
    yardstick    the fp32 restatement's own deviation from fp64 is at most 6.6e-5 on every interior-node gradient, so the GPU
                 bar max(1e-4, 1.5 x it) never leaves its floor, and at most 1e-5 / 1.5 on coeffs and sol likewise
    losses       every fp64 loss that is compared relatively is above 1e-7
    refusals     in the style of tests/test_fem_abi_host.py: k = 360 and, at k = 359, a two-word slab"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fem_lattices as L  # noqa: E402
from test_fem_abi_host import RING, SLAB_MASK, _call  # noqa: E402  (the dummy argument lists, two refusal texts)

from g_adaptivity_amd import _native_fem as nf  # noqa: E402
from g_adaptivity_amd.fem import lattice_axes  # noqa: E402

GRAD_CAP = 6.6e-5                            # 1.5 x it stays under the gradient floor 1e-4 (1e-4 / 1.5, rounded down)
VALUE_CAP = 1e-5 / 1.5                       # the same for the floor of coeffs and sol
NO_ROOM = "windowed evaluation: the lattice's running sums leave no room for a triangle slab in the LDS budget"
ALL_CASES = L.CASES + L.LIMIT_CASES
IDS = [f"{m}-{lat}" for m, lat in ALL_CASES]


def test_case_list():
    ks = {m: sorted(L.unit_k(lat) for mm, lat in ALL_CASES if mm == m and L.unit_k(lat)) for m in L.MESHES}
    assert ks == {'J5': [2, 3, 4, 16, 17, 33, 255, 256, 257, 359], 'J7': [3, 17, 359]}
    assert all((m, o) in L.CASES for m in L.MESHES for o in 'ABC')
    for name, (side, unknowns, tris) in {'J5': (5, 9, 32), 'J7': (7, 25, 72)}.items():
        x, m = L.mesh(name)
        p = L.params(name, 'u17')
        assert x.dtype == torch.float32 and x.shape == (side * side, 2) and m.cells.shape[0] == tris
        assert int((~m.boundary_nodes).sum()) == unknowns and len(p['centers']) == 2
        assert not torch.equal(x, m.x_comp) and torch.equal(x[m.boundary_nodes], m.x_comp[m.boundary_nodes])   # jittered inside


@pytest.mark.parametrize('lat', sorted({lat for _, lat in ALL_CASES}))
def test_axes(lat):
    ax, ay = L.axes(lat)
    assert ax.dtype == ay.dtype == torch.float32 and ax.numel() == ay.numel() >= 2
    for quad in ((ax, ay), list(torch.meshgrid(ax, ay, indexing='ij'))):           # as a pair of axes and as GNN.quad_points
        lx, ly = lattice_axes(quad, 'cpu')
        assert torch.equal(lx, ax) and torch.equal(ly, ay)
    k = L.unit_k(lat)
    if k is None:
        for a in (ax, ay):
            assert float(torch.minimum((a - 0.0).abs(), (a - 1.0).abs()).min()) >= 1e-3, lat
    else:
        assert k == ax.numel() and torch.equal(ax, torch.linspace(0, 1, k)) and torch.equal(ay, ax)
    pts = L.points(ax, ay, torch.float64)
    n = ax.numel()
    assert pts.shape == (2, n * n) and pts[0, 1 * n + 0] == ax[1].double() and pts[1, 0 * n + 1] == ay[1].double()
    if lat == 'C':                                                                  # four points, all inside the mesh
        assert n * n < L.EVAL_CHUNKS and bool(((pts > 0) & (pts < 1)).all())
    if lat == 'B':
        assert float(ax[-1] - ax[0]) != float(ay[-1] - ay[0])
    if lat == 'A':
        assert float(ax[0]) < 0 and float(ax[-1]) > 1


@pytest.mark.parametrize('mesh,lat', ALL_CASES, ids=IDS)
def test_cap_on_the_yardstick(mesh, lat):
    x, m = L.mesh(mesh)
    r64, r32 = L.reference(mesh, lat)
    interior = ~m.boundary_nodes
    for key in ('coeffs', 'sol'):
        own = L.rel(r32[key], r64[key])
        print(f"FEM-LATTICES-HOST {mesh} {lat} {key}: fp32 restatement dev {own:.3e} cap {VALUE_CAP:.3e}")
        assert own <= VALUE_CAP, (mesh, lat, key, own)
    if lat == 'u2':                                    # the corner nodes: sol is their coefficients, u_true there; no loss
        corners = L.corner_nodes(mesh)
        assert torch.equal(r64['sol'], r64['coeffs'][corners]) and float(r64['loss_mse']) == 0.0
        return
    grads = ['grad_w'] + (['grad_mse'] if L.has_loss(lat) else []) + (['grad_simpson'] if L.has_simpson(lat) else [])
    for key in grads:
        own, own_all = L.rel(r32[key][interior], r64[key][interior]), L.rel(r32[key], r64[key])
        print(f"FEM-LATTICES-HOST {mesh} {lat} {key}: fp32 restatement dev interior {own:.3e} cap {GRAD_CAP:.3e} (all nodes {own_all:.3e})")
        assert r64[key][interior].abs().max().item() > 0
        assert own <= GRAD_CAP, (mesh, lat, key, own)
    for key in (['loss_mse'] if L.has_loss(lat) else []) + (['loss_simpson'] if L.has_simpson(lat) else []):
        print(f"FEM-LATTICES-HOST {mesh} {lat} {key}: fp64 {float(r64[key]):.6e} fp32 restatement dev {L.rel(r32[key], r64[key]):.3e}")
        assert float(r64[key]) > 1e-7, (mesh, lat, key)
    if lat == 'A':                                     # outside the unit square the reference's sol is exactly zero
        pts = L.points(*L.axes(lat), torch.float64)
        outside = ((pts < 0) | (pts > 1)).any(0)
        assert int(outside.sum()) == 17 * 17 - 13 * 13 and bool((r64['sol'][outside] == 0).all()) and bool((r64['sol'][~outside] != 0).all())


# ---------------------------------------------------------------------------------------------------- the window limit
WINDOWED_EVAL = ['gadapt_fem_forward_window', 'gadapt_fem_eval_errors_window', 'gadapt_fem_modular_forward_window']


def test_limit_follows_from_the_budget():
    """359 and 360 from the library's budget and win_plan's formula: ceil(k^2 / 8) floats of running sums, then whole mask
    words of 16 x 16 bins x 4 B."""
    budget = nf.lib().gadapt_fem_lds_budget()
    assert budget == 65536
    assert L.window_limit(budget) == (359, 1) and L.K_LIMIT == 359
    assert budget - 4 * -(-359 * 359 // 8) == 1092 and budget - 4 * -(-360 * 360 // 8) == 736       # one word is 1024 B


@pytest.mark.parametrize('entry', WINDOWED_EVAL)
def test_refusals_at_the_limit(entry):
    """Every call fails a check, so nothing is launched (dummy host pointers, tests/test_fem_abi_host.py).  The windowed entry
    points have no check after the plan, so a call that passes it cannot be shown here by a later refusal: that k = 359 with
    tri_slab = 0 passes is shown by the refusal of tri_slab = 64 at k = 359 - the slab check comes after the one for room,
    so the running sums left at least one word, and two do not fit - and by the GPU test, which runs it."""
    k = L.K_LIMIT
    for slab in (0, 32, 64):
        rc, msg = _call(entry, {'nlat': k + 1, 'tri_slab': slab})
        assert (rc, msg) == (-5, NO_ROOM), (entry, slab, rc, msg)
    rc, msg = _call(entry, {'nlat': k, 'tri_slab': 64})
    assert (rc, msg[:len(SLAB_MASK)]) == (-5, SLAB_MASK), (entry, rc, msg)
    rc, msg = _call(entry, {'nlat': k - 1, 'tri_slab': 64})
    assert (rc, msg[:len(SLAB_MASK)]) == (-5, SLAB_MASK), (entry, rc, msg)
    # the order: the ring before the lattice's room, the lattice's room before the slab; a broken pointer before all
    assert _call(entry, {'nlat': k + 1, 'max_lds_bytes': 0})[1][:len(RING)] == RING
    assert _call(entry, {'nlat': k + 1, 'tri_slab': 31})[1].endswith('tri_slab must be 0 or a positive multiple of 32')
    assert _call(entry, {'nlat': k + 1, 'meta': None})[0] == -1


def test_backward_window_has_no_lattice_limit():
    """The fourth windowed entry point evaluates nothing on the lattice through LDS: k = 360 reaches its ring check."""
    rc, msg = _call('gadapt_fem_backward_window', {'nlat': L.K_LIMIT + 1, 'max_lds_bytes': 0})
    assert (rc, msg[:len(RING)]) == (-5, RING)
