"""The wave-parallel FEM forward (fem_forward='wave': gadapt_fem_forward_wave, gadapt_fem_modular_forward_wave) against the lane
entry points on the same inputs: rhs, coeffs, the kept factor and sol - and the modular loss and its seed - bit for bit, no
tolerance.  The yardstick is gadapt_fem_forward / gadapt_fem_modular_forward itself; one test anchors the result outside the
project's kernels, on the fp64 restatement.  Cases: the smallest at which the wave kernels can go wrong - a Simpson box that is
the whole square, many workgroups with a part-filled last one, fewer lattice points than lanes, lattice points on vertices and
edges, mixed batches, overlapping triangles, the route's largest mesh, a lattice wider than the mesh, one and three Gaussians.

The evaluation notes the triangles that contain a lattice point in FEM_EVALW_CAP = 4 registers per lane before it evaluates
them, and evaluates early when a fifth turns up.  The cases beyond that capacity: an interior vertex of the unmoved 5 x 5 mesh
lies in its 6 incident triangles (the inclusive edge test; the lattice's 1/16 steps hit the vertices exactly), which
test_unmoved_mesh_exceeds_the_note counts on the host, and the folded meshes add the triangles folded over such points."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fem_restatement as R  # noqa: E402

from g_adaptivity_amd import GNN, GraphedTrainStep, MeshDataset, collate, fem, hot_path_opt, l1_loss  # noqa: E402
from g_adaptivity_amd import _native_fem as nf  # noqa: E402
from g_adaptivity_amd._native import current_stream  # noqa: E402
from g_adaptivity_amd.mesh_graph import MeshData, square_mesh  # noqa: E402
from g_adaptivity_amd.optim import FlatAdam  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NOTE_CAPACITY = 4                                            # FEM_EVALW_CAP of fem_csrc/fem_wave_fwd_kernels.hip


def _params(k, seed):
    rng = np.random.default_rng(seed)
    return {'centers': [rng.uniform(0, 1, 2).astype('f') for _ in range(k)],
            'scales': [rng.uniform(0.1, 0.5, 2).astype('f') for _ in range(k)]}


def _coords(n, kind, seed=0):
    """tests/test_gpu_fem_wave_grad.py::_coords; 'folded3' folds two more interior nodes over their neighbours."""
    m = square_mesh(n)
    x = m.x_comp.clone()
    if kind == 'jittered':
        g = torch.Generator().manual_seed(seed)
        d = (torch.rand(x.shape, generator=g) * 2 - 1) * 0.2 / (n - 1)
        d[m.boundary_nodes] = 0.0
        x = x + d
    elif kind in ('folded', 'folded3'):
        i = (n // 2) * n + n // 2
        x[i, 0] += 1.3 / (n - 1)
        if kind == 'folded3':
            x[i + n, 0] += 1.3 / (n - 1)
            x[i - n, 1] += 1.3 / (n - 1)
    return x, m


class _Batch:
    """A batch of square meshes on the device with its Gaussians and lattice, ready for either forward entry point."""

    def __init__(self, sizes, kind, nlat, gauss=2, lat=None):
        xs, ms = zip(*[_coords(n, kind, seed=n) for n in sizes])
        counts = [m.num_nodes for m in ms]
        off = np.cumsum([0] + counts[:-1])
        cells = np.concatenate([m.cells.numpy() + int(o) for m, o in zip(ms, off)])
        bnd = np.concatenate([m.boundary_nodes.numpy() for m in ms])
        self.sizes, self.counts = list(sizes), counts
        self.topo = fem.FemTopology(cells, bnd, counts, [m.cells.shape[0] for m in ms], DEV)
        self.gptr, self.gpar = fem.pack_gaussians([_params(gauss, 7 * n + b) for b, n in enumerate(sizes)], DEV)
        lat_x, lat_y = lat if lat is not None else (torch.linspace(0, 1, nlat), torch.linspace(0, 1, nlat))
        self.lat_x, self.lat_y, self.nlat = lat_x.to(DEV), lat_y.to(DEV), nlat
        self.x = torch.cat(xs).to(DEV)

    def forward(self, op, fill):
        """(rhs, coeffs, lfac, sol) of ENTRY_POINTS[op]['lds']; the outputs are pre-filled with `fill`, so an entry a kernel leaves
        unwritten shows when the two sides are filled differently."""
        N, t = self.topo.n_nodes, self.topo
        out = [torch.full((N,), fill, device=DEV), torch.full((N,), fill, device=DEV), t.factor_buffer(DEV).fill_(fill),
               torch.full((t.n_meshes * self.nlat * self.nlat,), fill, device=DEV)]
        nf.call(fem.ENTRY_POINTS[op]['lds'], *t.head(self.gptr, self.gpar, self.x, self.lat_x, self.lat_y, self.nlat),
                *fem._solve_tail(t, out[0], out[1], out[2], 0), out[3].data_ptr(), current_stream(DEV))
        torch.cuda.synchronize()
        return out

    def modular(self, op, reduction, fill):
        """(rhs, coeffs, lfac, sol, loss, g_sol) of the modular entry point."""
        N, t = self.topo.n_nodes, self.topo
        Q = t.n_meshes * self.nlat * self.nlat
        out = [torch.full((N,), fill, device=DEV), torch.full((N,), fill, device=DEV), t.factor_buffer(DEV).fill_(fill),
               torch.full((Q,), fill, device=DEV), torch.full((t.n_meshes,), fill, device=DEV), torch.full((Q,), fill, device=DEV)]
        nf.call(fem.ENTRY_POINTS[op]['lds'], *t.head(self.gptr, self.gpar, self.x, self.lat_x, self.lat_y, self.nlat),
                fem._REDUCTIONS[reduction], *fem._solve_tail(t, out[0], out[1], out[2], 0), out[3].data_ptr(), out[4].data_ptr(),
                out[5].data_ptr(), current_stream(DEV))
        torch.cuda.synchronize()
        return out


NAMES = ('rhs', 'coeffs', 'lfac', 'sol', 'loss', 'g_sol')


def _same_bits(got, want, what):
    assert len(got) == len(want)
    for name, a, b in zip(NAMES, got, want):
        assert torch.equal(a, b), (what, name, (a != b).sum().item(), (a - b).abs().max().item())
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, name, 'signs of zero')


# (sizes, kind, nlat, Gaussians): see the module docstring
CASES = {
    '3x3-nlat101': ([3], 'jittered', 101, 2),                # one interior node, its Simpson box the whole square; 160 workgroups
    '5x5-unmoved-nlat17': ([5], 'unmoved', 17, 2),           # lattice points exactly on vertices and edges: 2 to 6 triangles per point
    'mixed-4-7-6-nlat17': ([4, 7, 6], 'jittered', 17, 2),
    'two-11x11-nlat101': ([11, 11], 'jittered', 101, 2),     # the reference's case
    '5x5-nlat2': ([5], 'jittered', 2, 2),                    # fewer points than lanes
    '5x5-nlat3': ([5], 'jittered', 3, 2),
    'folded-11x11': ([11], 'folded', 101, 3),                # overlapping triangles
    'folded3-unmoved-5x5-nlat17': ([5], 'folded3', 17, 2),   # three folds over an unmoved mesh: vertices in more than 6 triangles
    '26x26-nlat17': ([26], 'jittered', 17, 2),               # the route's size limit: 1 250 triangles, W = 40
    '6x6-one-gaussian': ([6], 'jittered', 17, 1),
    '6x6-three-gaussians': ([6], 'jittered', 17, 3),
}


@pytest.fixture(scope='module')
def batches():
    cache = {}

    def get(name):
        if name not in cache:
            sizes, kind, nlat, gauss = CASES[name]
            cache[name] = _Batch(sizes, kind, nlat, gauss)
        return cache[name]
    return get


@pytest.mark.parametrize('name', list(CASES))
def test_wave_forward_is_the_lane_forward(batches, name):
    bt = batches(name)
    lane = bt.forward('forward', fill=1.0)
    wave = bt.forward('forward_wave', fill=2.0)
    assert all(torch.isfinite(t).all() for t in lane), name
    assert lane[3].abs().max() > 0
    _same_bits(wave, lane, name)


def _containing(x, cells, px, py):
    """How many triangles contain (px, py) by the inclusive edge test of fem_csrc/fem_common.h, in fp32 as written there."""
    f = np.float32
    count = 0
    for c in cells:
        a, b, cc = (x[c[2]], x[c[1]], x[c[0]])
        left = right = 1
        for p, q in ((a, b), (b, cc), (cc, a)):
            u, v = f(p[1] - q[1]), f(q[0] - p[0])
            lhs, rhs = f(f(u * f(px)) + f(v * f(py))), f(f(u * p[0]) + f(v * p[1]))
            left *= int(lhs >= rhs)
            right *= int(lhs <= rhs)
        count += left + right > 0
    return count


def test_unmoved_mesh_exceeds_the_note():
    """The capacity of the evaluation's note is 4 triangles; the largest count on the unmoved 5 x 5 mesh with the 17 x 17 lattice
    is 6 (every interior vertex), so '5x5-unmoved-nlat17' runs the early evaluation; with the three folds of 'folded3' the
    largest count is 8, which fills the note twice.  Counted here on the host, in fp32."""
    lat = np.linspace(0, 1, 17, dtype=np.float32)
    counts = {}
    for kind in ('unmoved', 'folded3'):
        x, m = _coords(5, kind)
        x, cells = x.numpy().astype(np.float32), m.cells.numpy()
        counts[kind] = max(_containing(x, cells, px, py) for px in lat for py in lat)
    print('largest number of containing triangles:', counts)
    assert counts['unmoved'] == 6 > NOTE_CAPACITY
    assert counts['folded3'] > counts['unmoved']


def test_each_mesh_alone_gives_its_bits_in_the_batch(batches):
    bt = batches('mixed-4-7-6-nlat17')
    rhs, coeffs, lfac, sol = bt.forward('forward_wave', fill=2.0)
    Q = bt.nlat * bt.nlat
    n_off = f_off = 0
    for b, n in enumerate(bt.sizes):
        one = _Batch([n], 'jittered', bt.nlat)
        one.gptr, one.gpar = fem.pack_gaussians([_params(2, 7 * n + b)], DEV)    # mesh b's Gaussians of the batch
        r1, c1, l1, s1 = one.forward('forward_wave', fill=3.0)
        nn, nf_ = n * n, int(one.topo.n_int[0]) * (int(one.topo.band[0]) + 1)
        _same_bits((r1, c1, l1[:nf_], s1), (rhs[n_off:n_off + nn], coeffs[n_off:n_off + nn], lfac[f_off:f_off + nf_], sol[b * Q:(b + 1) * Q]),
                   ('alone', n))
        n_off, f_off = n_off + nn, f_off + nf_


def test_lattice_wider_than_the_mesh(batches):
    """A square lattice with other ends is accepted by both; its points outside every triangle give sol = 0 with the lane
    kernel's sign.  A 9 x 7 lattice is refused by both in the same way (the lattice must be square)."""
    lat = (torch.linspace(-0.25, 1.25, 9), torch.linspace(-0.1, 1.1, 9))
    bt = _Batch([6], 'jittered', 9, lat=lat)
    lane = bt.forward('forward', fill=1.0)
    wave = bt.forward('forward_wave', fill=2.0)
    assert torch.isfinite(lane[3]).all() and (lane[3].view(9, 9)[0] == 0).all() and lane[3].abs().max() > 0
    _same_bits(wave, lane, 'wider lattice')
    x, m = _coords(6, 'jittered', seed=6)
    uneven = (torch.linspace(-0.25, 1.25, 9), torch.linspace(0.1, 0.9, 7))
    msgs = []
    for forward in ('lane', 'wave'):
        with pytest.raises(NotImplementedError, match='square') as e:
            fem.fem_poisson(x.to(DEV), m.cells, m.boundary_nodes, [m.num_nodes], [_params(2, 1)], uneven, forward=forward)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]


@pytest.mark.parametrize('reduction', ['mse', 'simpson'])
def test_modular_forward_wave_is_the_lane_modular_forward(batches, reduction):
    bt = batches('mixed-4-7-6-nlat17')
    lane = bt.modular('modular_forward', reduction, fill=1.0)
    wave = bt.modular('modular_forward_wave', reduction, fill=2.0)
    assert all(torch.isfinite(t).all() for t in lane) and lane[4].min() > 0
    _same_bits(wave, lane, reduction)


@pytest.mark.parametrize('adjoint', ['lane', 'wave'])
def test_fem_poisson_forward_keyword(adjoint):
    x, m = _coords(6, 'jittered', seed=3)
    lat = torch.linspace(0, 1, 17)
    res = {}
    for forward in ('lane', 'wave'):
        xg = x.to(DEV).requires_grad_(True)
        coeffs, sol = fem.fem_poisson(xg, m.cells, m.boundary_nodes, [m.num_nodes], [_params(2, 1)], (lat, lat), adjoint=adjoint,
                                      forward=forward)
        (sol.square().sum() + coeffs.sum()).backward()               # the backward reads what the forward kept
        res[forward] = (coeffs.detach(), sol.detach(), xg.grad)
    for a, b in zip(res['wave'], res['lane']):
        assert torch.equal(a, b) and torch.isfinite(b).all() and b.abs().max() > 0


def test_gradient_meshpoints_2D_with_the_wave_forward():
    x, m = _coords(7, 'jittered', seed=7)
    data = MeshData(x_comp=m.x_comp, cells=m.cells, boundary_nodes=m.boundary_nodes, batch=None, pde_params=[_params(2, 3)])
    res = {}
    for forward in ('lane', 'wave'):
        opt = hot_path_opt(mesh_dims=[7, 7], loss_type='modular', grad_type='PDE_loss_direct_mse', fem_forward=forward, device=str(DEV))
        loss, x_grads = fem.gradient_meshpoints_2D(opt, data, x.to(DEV))
        res[forward] = (loss, x_grads)
    assert res['lane'][0].item() > 0 and res['lane'][1].abs().max() > 0
    for a, b in zip(res['wave'], res['lane']):
        assert torch.equal(a, b)


def test_wave_forward_step_is_the_lane_step():
    """A 7 x 7 pde_loss GNN (hidden 8, 4 layers) steps three times through GraphedTrainStep with fem_forward='wave': parameters,
    Adam moments and losses are those of the same steps with 'lane' (tests/test_gpu_pde_step.py's wave-adjoint test)."""
    n, nlat = 7, 17
    ds = MeshDataset([n, n], 6, seed=22, num_gauss=2, pde_loss_fields=True, eval_quad_points=nlat)
    steps = [collate(ds.samples[2 * k:2 * k + 2]) for k in range(3)]
    runs = {}
    for forward in ('wave', 'lane'):
        opt = hot_path_opt(mesh_dims=[n, n], hidden_dim=8, num_layers=4, time_step=0.1, loss_type='pde_loss', eval_quad_points=nlat,
                           device=str(DEV), fem_forward=forward)
        torch.manual_seed(0)
        model = GNN(ds, opt).to(DEV).train()
        optim = FlatAdam(model.parameters(), lr=1e-2, capturable=True)
        step = GraphedTrainStep(model, optim, loss_fn=l1_loss)
        losses = [step(b.clone().to(DEV)).clone() for b in steps]
        torch.cuda.synchronize()
        assert len(step._captured) == 1 and next(iter(step._captured.values())).static._pde_batch.forward == forward
        runs[forward] = [p.detach().clone() for p in model.parameters()] + [optim.exp_avg.clone(), optim.exp_avg_sq.clone()] + losses
    assert len({l.item() for l in runs['lane'][-3:]}) == 3                       # three different batches
    for a, b in zip(runs['wave'], runs['lane']):
        assert torch.equal(a, b)


def test_wave_forward_against_the_fp64_restatement():
    """coeffs and sol of the wave forward on a jittered 11 x 11 mesh against the fp64 run of tests/fem_restatement.py, by the rule
    of tests/test_gpu_pde_loss.py: rel <= max(1e-5, 1.5 x noise), noise being the fp32 restatement's own distance from fp64.
    On a jittered mesh no Simpson or lattice point lies on an element edge, so the noise is that of an fp32 solve; it is
    asserted below 5e-2, the bound of tests/test_gpu_fem_wave_grad.py on the same quantity."""
    x, m = _coords(11, 'jittered', seed=11)
    p = _params(2, 11)
    lat = torch.linspace(0, 1, 101)
    coeffs, sol = fem.fem_poisson(x.to(DEV), m.cells, m.boundary_nodes, [m.num_nodes], [p], (lat, lat), forward='wave')
    ref = {}
    for dt in (torch.float32, torch.float64):
        c, s = R.fem2d(x.to(dt), m.cells, m.boundary_nodes, p['centers'], p['scales'], lat.to(dt))
        ref[dt] = (c.detach().double().view(-1), s.detach().double().view(-1))

    def rel(a, b):
        return ((a - b).abs().max() / b.abs().max()).item()
    for name, got, k in (('coeffs', coeffs, 0), ('sol', sol, 1)):
        noise = rel(ref[torch.float32][k], ref[torch.float64][k])
        err = rel(got.detach().cpu().double().view(-1), ref[torch.float64][k])
        print(f"{name}: wave vs fp64 {err:.3e}, fp32 restatement vs fp64 {noise:.3e}")
        assert noise < 5e-2, (name, noise, 'the restatement itself is ill-conditioned here')
        assert err <= max(1e-5, 1.5 * noise), (name, err, noise)
