"""The 2-D FEM tail on the MI355X on node orders, triangulations and sizes that square_mesh's row-major numbering never reaches
(fem_csrc/fem_kernels.hip, fem_window_kernels.hip, fem_window_grad_kernels.hip through fem_poisson, modular_loss_2d and
poisson_eval_errors; the meshes are tests/fem_meshes.py's):

    wide band, band='lds'      12 x 12 renumbered (w = 91) and 11 x 11 with w = 80: the 64 lanes of the one-wave solve take
                               a column's entries in two trips
    tight ring, band='window'  11 x 11 with w = 77, 78, 79: ring slack S = 7, 4, 2 rows, R = w + S, the back substitution's two
                               stages fill most of it; 12 x 12 with the same bands (two nodes swapped): 100 rows wrap in
                               that ring; w = 80 is refused
    mixed batches, the smallest meshes (3 x 3: one unknown, w = 0, no pairs), the union-jack triangulation (valences 4, 8),
    another triangle order, the evaluation entry point, and the two documented maxima 26 x 26 and 81 x 81.

Rules (the project's own, no new tolerance), each against the fp64 restatement with the fp32 restatement's own deviation from
it on the same mesh and ordering as the yardstick (_assert_rule of tests/test_gpu_fem_window_grad.py):
    loss                 rel <= max(LOSS_FLOOR, 1.5 x fp32 deviation)
    gradient             rel <= max(1e-4, 1.5 x fp32 deviation)
    coefficients, sol    rel <= max(1e-5, 1.5 x fp32 deviation)
A renumbered call against the natural one (permutation undone) gets twice that bar - both sides carry the rounding of an
fp32 solve - and the kernels must have been launched on the renumbered mesh's band.  On 'lds' the two must not be bitwise
equal either (an fp32 elimination in another order); on 'window' they are, since the fp64 ring's result is rounded to fp32.
Calls of one route on one ordering among themselves - batches, slabs, repeats, a second backward - are compared bitwise.  The restatements run live, once per mesh (3 to 12 a side, seconds), shared by the tests; every mesh
is jittered (on unmoved grids fp32 and fp64 class edge points differently, docs/measurements.md).  The maxima come from
tests/golden/fem_limits/ (make_fem_limits_golden.py beside them).  Every figure is printed before it is asserted (-s);
docs/measurements.md has them."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_restatement as E  # noqa: E402
import fem_meshes as F  # noqa: E402
import fem_restatement as R  # noqa: E402
import modular2d_restatement as M  # noqa: E402
from test_gpu_evaluation_window import _check as _check_norms  # noqa: E402  (the evaluation's rule)
from test_gpu_fem_window_grad import _assert_rule, _u_true_nodes  # noqa: E402  (the rule; u_true as the boundary rows compute it)
from test_gpu_modular2d import LOSS_FLOOR, _coords, _params, _rel  # noqa: E402  (the mesh and Gaussian recipes, the floor)

from g_adaptivity_amd import _native_fem, fem_poisson, poisson_eval_errors  # noqa: E402
from g_adaptivity_amd.fem import _topology, modular_loss_2d  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
N_LAT = 101
LAT = torch.linspace(0, 1, N_LAT)
QUAD = list(torch.meshgrid(LAT, LAT, indexing='ij'))
FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fem_limits')
KINDS = {'mse': ('mse', N_LAT), 'L2': ('simpson', R.SIMPSON_N)}     # restatement kind -> (reduction, n_lat) of modular_loss_2d
# one Gaussian well inside the square: the single unknown of 3 x 3 is of order one, so the relative measures mean something
SMALL_PARAMS = {'centers': [np.array([0.45, 0.55], np.float32)], 'scales': [np.array([0.3, 0.35], np.float32)]}
RENUMBERED = {'n11w77': (11, F.SEED_N11_W77, 77), 'n11w78': (11, F.SEED_N11_W78, 78), 'n11w79': (11, F.SEED_N11_W79, 79),
              'n11w80': (11, F.SEED_N11_W80, 80), 'n12wide': (12, F.SEED_N12_WIDE, F.W_N12_WIDE),
              # two interior nodes swapped (fem_meshes.far_swap; no seed): 100 unknowns, more than the ring's R = w + S rows
              'n12s77': (12, None, 77), 'n12s78': (12, None, 78), 'n12s79': (12, None, 79)}


class Case:
    """One mesh: x [N,2] fp32 (jittered), cells, boundary, its Gaussians, and perm (old node i is node perm[i]; None: natural)."""

    def __init__(self, name, x, cells, boundary, params, perm=None):
        self.name, self.x, self.cells, self.boundary, self.params = name, x, cells, boundary, params
        self.perm = None if perm is None else torch.from_numpy(perm)
        self.n_nodes = x.shape[0]
        g = torch.Generator().manual_seed(self.n_nodes)               # the weights of _grad_case's functional, on the natural ids
        self.w_sol = torch.randn(N_LAT * N_LAT, generator=g)
        self.w_c = self.to_own(torch.randn(self.n_nodes, generator=g))

    def to_own(self, t):
        """A per-node tensor of the natural numbering in this case's."""
        if self.perm is None:
            return t
        out = torch.empty_like(t)
        out[self.perm] = t
        return out

    def to_natural(self, t):
        return t if self.perm is None else t[self.perm.to(t.device)]


@functools.lru_cache(maxsize=None)
def _case(name):
    """'n<k>': square_mesh(k) as it is; RENUMBERED's names; 'uj<k>': union_jack(k); 'n11tri': square_mesh(11), triangles
    shuffled; 'small<k>': square_mesh(k) with SMALL_PARAMS."""
    if name in RENUMBERED:
        n, seed, w = RENUMBERED[name]
        x, m = _coords(n, 'jittered', seed=n + 1)
        xp, cells, bnd, perm = F.permuted(m, x, seed=seed) if seed is not None else F.permuted(m, x, perm=F.far_swap(n, w))
        assert F.band_of(cells, bnd) == w
        return Case(name, xp, cells, bnd, _params(2, n), perm)
    if name.startswith('uj'):
        n = int(name[2:])
        x, _ = _coords(n, 'jittered', seed=n + 1)
        _, cells, bnd = F.union_jack(n)
        return Case(name, x, cells, bnd, _params(2, n))
    if name == 'n11tri':
        x, m = _coords(11, 'jittered', seed=12)
        return Case(name, x, F.shuffled_triangles(m.cells, 5), m.boundary_nodes, _params(2, 11))
    small = name.startswith('small')
    n = int(name[5:] if small else name[1:])
    x, m = _coords(n, 'jittered', seed=n + 1)
    return Case(name, x, m.cells, m.boundary_nodes, SMALL_PARAMS if small else _params(2, n))


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The restatements on one solve per precision (their own operations, the load vector and the dense solve shared): the
    coefficients, sol on the 101 x 101 lattice, both losses of modular2d_restatement with their gradients, and the gradient
    of tests/test_gpu_pde_loss.py::_grad_case's functional (sol . w_sol + coeffs . w_c).  (fp64, fp32), everything as fp64."""
    c = _case(name)
    p = c.params
    out = {}
    for dt in (torch.float64, torch.float32):
        xx = c.x.to(dt).clone().requires_grad_(True)
        A, rhs, cells = M._system(xx, c.cells, c.boundary, p['centers'], p['scales'], R.SIMPSON_N)
        co = torch.linalg.solve(A, rhs.unsqueeze(1)).squeeze(1)
        pts = M.grid(N_LAT, dt)
        sol = M.expand(co, pts, xx, cells)
        mse = torch.nn.functional.mse_loss(sol, R.u_true(pts, p['centers'], p['scales']))
        l2 = M.l2_error(co, xx, cells, p['centers'], p['scales'], R.SIMPSON_N)
        fw = (sol * c.w_sol.to(dt)).sum() + (co * c.w_c.to(dt)).sum()
        (g_mse,) = torch.autograd.grad(mse, xx, retain_graph=True)
        (g_w,) = torch.autograd.grad(fw, xx, retain_graph=True)
        (g_l2,) = torch.autograd.grad(l2, xx)
        out[dt] = dict(coeffs=co.detach().double(), sol=sol.detach().double(), loss_mse=mse.detach().double(), grad_mse=g_mse.double(),
                       loss_L2=l2.detach().double(), grad_L2=g_l2.double(), grad_w=g_w.double())
    return out[torch.float64], out[torch.float32]


@functools.lru_cache(maxsize=None)
def _eval_reference(name):
    """The (L1, L2) pair of tests/golden/eval_window/make_eval_window_golden.py (eval_restatement.errors_2d), fp64 and fp32."""
    c = _case(name)
    args = (c.x, c.cells, c.boundary, c.params['centers'], c.params['scales'], N_LAT)
    return E.errors_2d(*args, torch.float64), E.errors_2d(*args, torch.float32)


def _poisson(c, band, **kw):
    xg = c.x.to(DEV).requires_grad_(True)
    coeffs, sol = fem_poisson(xg, c.cells, c.boundary, [c.n_nodes], [c.params], QUAD, band=band, **kw)
    return xg, coeffs, sol


def _poisson_grad(c, band, **kw):
    """fem_poisson and the gradient of _grad_case's functional: (coeffs [N], sol, gradient [N,2])."""
    xg, coeffs, sol = _poisson(c, band, **kw)
    ((sol * c.w_sol.to(DEV)).sum() + (coeffs.view(-1) * c.w_c.to(DEV)).sum()).backward()
    return coeffs.detach().view(-1), sol.detach(), xg.grad


def _modular(c, kind, band, **kw):
    reduction, n_lat = KINDS[kind]
    return modular_loss_2d(c.x.to(DEV), c.cells, c.boundary, [c.n_nodes], [c.params], n_lat, reduction, band=band, **kw)


def _against_fp64(name, band, kinds=('mse', 'L2')):
    """Every output of the route on one mesh under the rules; returns what the GPU gave."""
    c = _case(name)
    r64, r32 = _reference(name)
    label = f"{name} band={band}"
    got = {}
    got['coeffs'], got['sol'], got['grad_w'] = _poisson_grad(c, band)
    _assert_rule(label + " fem_poisson", 'coeffs', got['coeffs'], r64['coeffs'], r32['coeffs'], 1e-5)
    _assert_rule(label + " fem_poisson", 'sol', got['sol'], r64['sol'], r32['sol'], 1e-5)
    _assert_rule(label + " fem_poisson", 'weighted-sum gradient', got['grad_w'], r64['grad_w'], r32['grad_w'], 1e-4)
    for k in kinds:
        loss, g = _modular(c, k, band)
        assert loss.shape == (1,) and g.shape == (c.n_nodes, 2)
        got['loss_' + k], got['grad_' + k] = loss[0], g
        _assert_rule(f"{label} modular {k}", 'loss', loss[0], r64['loss_' + k], r32['loss_' + k], LOSS_FLOOR)
        _assert_rule(f"{label} modular {k}", 'gradient', g, r64['grad_' + k], r32['grad_' + k], 1e-4)
    return got


FLOORS = {'coeffs': 1e-5, 'sol': 1e-5, 'grad_w': 1e-4, 'grad_mse': 1e-4, 'grad_L2': 1e-4, 'loss_mse': LOSS_FLOOR, 'loss_L2': LOSS_FLOOR}


def _against_other_call(label, c, got, other, r64, r32, factor, per_node=('coeffs', 'grad_w', 'grad_mse', 'grad_L2')):
    """`got` (on the case c) against `other` (the same mesh in its natural numbering or triangle order): within factor x the
    rule's bar of `got`'s mesh.  Returns the quantities that came out bitwise equal."""
    same = []
    for key, a in got.items():
        a = a.detach().cpu().double()
        if key in per_node:
            a = c.to_natural(a)
        b = other[key].detach().cpu().double().reshape(a.shape)
        dev, own = _rel(a, b), _rel(r32[key], r64[key])
        bound = factor * max(FLOORS[key], 1.5 * own)
        print(f"FEM-ORDERINGS {label} {key}: dev from the other call {dev:.3e} bound {bound:.3e}")
        assert np.isfinite(dev) and dev <= bound, (label, key, dev, bound)
        if torch.equal(a, b):
            same.append(key)
    return same


def _launched_band(c, band):
    """The half-bandwidth in the meta row the kernels of a single-mesh call on `c` read (fem_poisson's cached topology)."""
    topo = _topology(c.cells, c.boundary, [c.n_nodes], [c.cells.shape[0]], DEV, band)
    assert topo.route == band and int(topo.dev['meta'][0, _native_fem.M_BAND].item()) == int(topo.band[0])
    return int(topo.band[0])


def _natural_of(name, band, kinds=('mse', 'L2')):
    c = _case(f"n{RENUMBERED[name][0]}")
    out = {}
    out['coeffs'], out['sol'], out['grad_w'] = _poisson_grad(c, band)
    for k in kinds:
        loss, g = _modular(c, k, band)
        out['loss_' + k], out['grad_' + k] = loss[0], g
    return out


# ------------------------------------------------------------------------------------------------ 1. wide band, resident route
@pytest.mark.one_dispatch
@pytest.mark.parametrize('name', ['n12wide', 'n11w80'])
def test_wide_band_lds(name):
    """w = 91 and w = 80 > 64: band_factor, band_solve and the adjoint's band_solve take a column's entries in two trips of
    the 64 lanes, and the pair table has 4186 / 3240 entries."""
    c = _case(name)
    got = _against_fp64(name, 'lds')
    r64, r32 = _reference(name)
    assert _launched_band(c, 'lds') == RENUMBERED[name][2]
    same = _against_other_call(f"{name} band=lds vs natural", c, got, _natural_of(name, 'lds'), r64, r32, 2.0)
    assert not {'coeffs', 'grad_w', 'grad_mse', 'grad_L2'} & set(same), same      # an fp32 elimination in another order


# ------------------------------------------------------------------------------------------------ 2. tight ring, windowed route
@pytest.mark.one_dispatch
@pytest.mark.parametrize('name', ['n11w77', 'n11w78', 'n11w79', 'n12s77', 'n12s78', 'n12s79'])
def test_tight_ring_window(name):
    """A ring of R = w + S = 84 / 82 / 81 rows (S = 7 / 4 / 2); the back substitution's two stages take 2 S rows of it.
    11 x 11: 81 unknowns in 12 / 21 / 41 groups, the last one partial, every row in a slot of its own (81 <= R: no wrap).
    12 x 12 with two nodes swapped: 100 unknowns in 15 / 25 / 50 groups, rows R and beyond wrap into the slots of flushed
    ones, in the factorisation, in both substitutions and in the adjoint solve."""
    c = _case(name)
    got = _against_fp64(name, 'window')
    r64, r32 = _reference(name)
    # that the renumbering reached the kernel shows in the band of the topology it was launched on, not in the bits: the ring
    # eliminates in fp64, so another order moves a coefficient by ~1e-16 of itself and the fp32 it is rounded to stays the
    # same (measured: every quantity bitwise equal to the natural call's at w = 77, 78 and 79)
    assert _launched_band(c, 'window') == RENUMBERED[name][2]
    same = _against_other_call(f"{name} band=window vs natural", c, got, _natural_of(name, 'window'), r64, r32, 2.0)
    print(f"FEM-ORDERINGS {name} band=window vs natural: bitwise equal {same}")
    # backward twice on one forward: the kept workspace is only read
    xg, coeffs, sol = _poisson(c, 'window')
    fw = (sol * c.w_sol.to(DEV)).sum() + (coeffs.view(-1) * c.w_c.to(DEV)).sum()
    fw.backward(retain_graph=True)
    first = xg.grad.clone()
    xg.grad = None
    fw.backward(retain_graph=True)
    assert torch.equal(first, got['grad_w']) and torch.equal(xg.grad, first)
    # slabs of 32 and 64 triangle ids (200 triangles: seven and four slabs) against the default's one
    for tri_slab in (32, 64):
        for a, key in zip(_poisson_grad(c, 'window', tri_slab=tri_slab), ('coeffs', 'sol', 'grad_w')):
            assert torch.equal(a, got[key]), (tri_slab, key)
        for k in KINDS:
            loss, g = _modular(c, k, 'window', tri_slab=tri_slab)
            assert torch.equal(loss[0], got['loss_' + k]) and torch.equal(g, got['grad_' + k]), (tri_slab, k)


@pytest.mark.one_dispatch
def test_band_80_is_refused_by_the_window_route():
    c = _case('n11w80')
    with pytest.raises(NotImplementedError, match='half-bandwidth 80'):
        fem_poisson(c.x.to(DEV), c.cells, c.boundary, [c.n_nodes], [c.params], QUAD, band='window')
    with pytest.raises(NotImplementedError, match='half-bandwidth 80'):
        modular_loss_2d(c.x.to(DEV), c.cells, c.boundary, [c.n_nodes], [c.params], N_LAT, 'mse', band='window')
    with pytest.raises(NotImplementedError, match='half-bandwidth 80'):
        poisson_eval_errors(c.x.to(DEV), [c.n_nodes], [c.params], N_LAT, cells=c.cells, boundary=c.boundary, band='window')
    coeffs, sol = fem_poisson(c.x.to(DEV), c.cells, c.boundary, [c.n_nodes], [c.params], QUAD)      # the same mesh on 'lds'
    r64, r32 = _reference('n11w80')
    _assert_rule("n11w80 band=lds after the refusal", 'coeffs', coeffs, r64['coeffs'], r32['coeffs'], 1e-5)


# ------------------------------------------------------------------------------------------------ 3. mixed batches
@pytest.mark.one_dispatch
@pytest.mark.parametrize('band,names', [('window', ('n11', 'n11w79', 'n27')), ('lds', ('small3', 'n12wide', 'n15'))])
def test_mixed_batch_bitwise_equal_to_single_mesh_calls(band, names):
    """Natural and renumbered meshes in one call: every mesh as in its own call, whatever ring the launch was sized for."""
    cases = [_case(nm) for nm in names]
    counts = [c.n_nodes for c in cases]
    offs = np.cumsum([0] + counts[:-1]).tolist()
    cells = torch.cat([c.cells + o for c, o in zip(cases, offs)], 0)
    bnd = torch.cat([c.boundary for c in cases])
    ps = [c.params for c in cases]
    xg = torch.cat([c.x for c in cases]).to(DEV).requires_grad_(True)
    coeffs, sol = fem_poisson(xg, cells, bnd, counts, ps, QUAD, band=band)
    w_sol, w_c = torch.cat([c.w_sol for c in cases]).to(DEV), torch.cat([c.w_c for c in cases]).to(DEV)
    ((sol * w_sol).sum() + (coeffs.view(-1) * w_c).sum()).backward()
    batch = {k: modular_loss_2d(xg.detach(), cells, bnd, counts, ps, KINDS[k][1], KINDS[k][0], band=band) for k in KINDS}
    Q = N_LAT * N_LAT
    for b, (c, off) in enumerate(zip(cases, offs)):
        c1, s1, g1 = _poisson_grad(c, band)
        assert torch.equal(coeffs.detach().view(-1)[off:off + counts[b]], c1), (c.name, 'coeffs')
        assert torch.equal(sol.detach()[b * Q:(b + 1) * Q], s1), (c.name, 'sol')
        assert torch.equal(xg.grad[off:off + counts[b]], g1), (c.name, 'gradient')
        assert bool(torch.isfinite(g1).all()) and g1.abs().max().item() > 0
        for k in KINDS:
            l1, gk = _modular(c, k, band)
            assert torch.equal(batch[k][0][b:b + 1], l1), (c.name, k, 'loss')
            assert torch.equal(batch[k][1][off:off + counts[b]], gk), (c.name, k, 'gradient')


# ------------------------------------------------------------------------------------------------ 4. the smallest meshes
@pytest.mark.one_dispatch
@pytest.mark.parametrize('band', ['lds', 'window'])
@pytest.mark.parametrize('n', [3, 4, 5])
def test_smallest_meshes(n, band):
    """3 x 3: one unknown, w = 0, an empty pair table, 8 triangles; 4 x 4 (w = 2) and 5 x 5: 18 and 32 triangles, the latter
    exactly one mask word."""
    c = _case(f"small{n}")
    assert F.band_of(c.cells, c.boundary) == (n - 2 if n > 3 else 0) and c.cells.shape[0] == 2 * (n - 1) ** 2
    r64, _ = _reference(c.name)
    for key in ('coeffs', 'sol', 'grad_w'):
        assert r64[key].abs().max().item() >= 1e-3, key                 # _rel's denominator
    assert r64['coeffs'][~c.boundary].abs().min().item() >= 0.1         # the unknowns themselves are of order one
    _against_fp64(c.name, band, kinds=('mse',))


# ------------------------------------------------------------------------------------------------ 5. other triangulations
@pytest.mark.one_dispatch
@pytest.mark.parametrize('band', ['lds', 'window'])
@pytest.mark.parametrize('name', ['uj9', 'uj12', 'n11tri'])
def test_other_triangulations(name, band):
    """Union jack: incidence rows of 4 and 8 triangles (and 1 at two corners of 12 x 12) in phim_parts, simpson_box and the
    two gathers; shuffled triangles: the incidence rows and the bin mask's bits in another id order."""
    c = _case(name)
    got = _against_fp64(name, band, kinds=('mse',))
    if name == 'n11tri':
        r64, r32 = _reference(name)
        n11 = _case('n11')
        assert torch.equal(n11.x, c.x) and not torch.equal(n11.cells, c.cells)
        other = dict(zip(('coeffs', 'sol', 'grad_w'), _poisson_grad(n11, band)))
        loss, g = _modular(n11, 'mse', band)
        other['loss_mse'], other['grad_mse'] = loss[0], g
        _against_other_call(f"n11tri band={band} vs the natural triangle order", c, got, other, r64, r32, 1.0)


# ------------------------------------------------------------------------------------------------ 6. the evaluation
@pytest.mark.one_dispatch
@pytest.mark.parametrize('name,band', [('n12wide', 'lds'), ('n11w79', 'window')])
def test_poisson_eval_errors_on_renumbered_meshes(name, band):
    c = _case(name)
    e64, e32 = _eval_reference(name)
    l1, l2 = poisson_eval_errors(c.x.to(DEV), [c.n_nodes], [c.params], N_LAT, cells=c.cells, boundary=c.boundary, band=band)
    got = [l1.item(), l2.item()]
    assert np.isfinite(got).all()
    _check_norms(f"{name} band={band} (FEM-ORDERINGS)", got, e64, e32)


# ------------------------------------------------------------------------------------------------ 7. the documented maxima
@functools.lru_cache(maxsize=None)
def _fixture(n):
    x, m = _coords(n, 'jittered', seed=n + 1)
    z = np.load(os.path.join(FIXTURES, f'n{n}.npz'))
    assert int(z['n']) == n and int(z['n_lat_mse']) == N_LAT
    assert float(z['coords_sum']) == x.double().sum().item()       # the fixture's mesh
    r64, r32 = {}, {}
    for tag, r in (('64', r64), ('32', r32)):
        r['coeffs'] = torch.from_numpy(z['coeffs' + tag].astype(np.float64))
        r['loss_mse'] = torch.tensor(float(z[f'loss{tag}_mse']), dtype=torch.float64)
        if f'grad{tag}_mse' in z:
            r['grad_mse'] = torch.from_numpy(z[f'grad{tag}_mse'].astype(np.float64))
    return Case(f"n{n}", x, m.cells, m.boundary_nodes, _params(2, n)), r64, r32


@pytest.mark.one_dispatch
@pytest.mark.parametrize('band', ['lds', 'window'])
def test_maximum_of_the_resident_band_26(band):
    """26 x 26: 576 unknowns, w = 24, 61 104 B of the 64 KB budget on 'lds'; the same mesh on 'window' (S = 64)."""
    c, r64, r32 = _fixture(26)
    label = f"n=26 band={band}"
    _, coeffs, _ = _poisson(c, band)
    _assert_rule(label + " fem_poisson", 'coeffs', coeffs, r64['coeffs'], r32['coeffs'], 1e-5)
    loss, g = _modular(c, 'mse', band)
    print(f"FEM-ORDERINGS {label}: loss {loss.item():.9e} fp64 {r64['loss_mse'].item():.9e}")
    _assert_rule(label + " modular mse", 'loss', loss[0], r64['loss_mse'], r32['loss_mse'], LOSS_FLOOR)
    _assert_rule(label + " modular mse", 'gradient', g, r64['grad_mse'], r32['grad_mse'], 1e-4)


@pytest.mark.one_dispatch
def test_maximum_of_the_window_route_81():
    """81 x 81: 6241 columns, w = 79, S = 2, 12 800 triangles in seven default slabs, a 4 MB workspace.  Loss and coefficients
    against the fixture (one dense fp64 solve of the 6561-square system, no autograd through it).  The gradient has no fp64
    reference at this size: it is checked for being finite, nonzero on every interior node, repeatable and independent of the
    slab; its correctness rests on the w = 77 ... 79 cases of test_tight_ring_window, which run the same ring layout."""
    c, r64, r32 = _fixture(81)
    assert c.cells.shape[0] == 12800
    loss, g = _modular(c, 'mse', 'window')
    print(f"FEM-ORDERINGS n=81 band=window: loss {loss.item():.9e} fp64 {r64['loss_mse'].item():.9e}")
    _assert_rule("n=81 band=window modular mse", 'loss', loss[0], r64['loss_mse'], r32['loss_mse'], LOSS_FLOOR)
    _, coeffs, sol = _poisson(c, 'window')
    assert bool(torch.isfinite(sol).all())
    _assert_rule("n=81 band=window fem_poisson", 'coeffs', coeffs, r64['coeffs'], r32['coeffs'], 1e-5)
    bnd = c.boundary.to(DEV)
    assert torch.equal(coeffs.detach().view(-1)[bnd], _u_true_nodes(c.x.to(DEV), c.params)[bnd])
    assert g.shape == (81 * 81, 2) and bool(torch.isfinite(g).all()) and g.abs().max().item() > 0
    assert bool((g[~bnd] != 0).all())
    for kw in ({}, {'tri_slab': 512}):
        loss2, g2 = _modular(c, 'mse', 'window', **kw)
        assert torch.equal(loss2, loss) and torch.equal(g2, g), kw
