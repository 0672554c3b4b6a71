"""CPU checks of the pde_loss FEM tail: the test-side restatement pinned from independent sides, the host topology builder,
and the model's refusal of what is out of scope."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fem_restatement as R  # noqa: E402

from g_adaptivity_amd import GNN, MeshDataset, hot_path_opt  # noqa: E402
from g_adaptivity_amd.mesh_graph import square_mesh  # noqa: E402

CENTERS = [np.array([0.4, 0.55], np.float32), np.array([0.7, 0.3], np.float32)]
SCALES = [np.array([0.3, 0.25], np.float32), np.array([0.2, 0.35], np.float32)]


def _mesh(n, jitter=0.0, seed=0, dtype=torch.float64):
    m = square_mesh(n)
    x = m.x_comp.to(dtype).clone()
    if jitter:
        g = torch.Generator().manual_seed(seed)
        d = (torch.rand(x.shape, generator=g, dtype=dtype) * 2 - 1) * jitter / (n - 1)
        d[m.boundary_nodes] = 0.0
        x = x + d
    return x, m.cells, m.boundary_nodes


def test_simpson_points_constant_matches_library_header():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'gadapt_fem.h')).read()
    assert f"#define GADAPT_FEM_SIMPSON_N {R.SIMPSON_N}" in hdr


def test_stiffness_rows_sum_to_zero_and_area_is_one():
    x, cells, bnd = _mesh(8, jitter=0.2)
    A, area = R.stiffness(x, cells, bnd)
    interior = (~bnd).nonzero().reshape(-1)
    assert A[interior].sum(1).abs().max().item() < 1e-12
    assert abs(area.sum().item() - 1.0) < 1e-12


def test_nodal_error_falls_as_h_squared():
    errs = []
    for n in (8, 16, 32):
        x, cells, bnd = _mesh(n)
        coeffs, _ = R.fem2d(x, cells, bnd, CENTERS, SCALES, torch.linspace(0, 1, 3, dtype=torch.float64))
        errs.append((coeffs - R.u_true(x.T, CENTERS, SCALES)).abs().max().item())
    hs = [1 / 7, 1 / 15, 1 / 31]
    rates = [np.log(errs[i] / errs[i + 1]) / np.log(hs[i] / hs[i + 1]) for i in range(2)]
    # measured: rates ~ 2 (second order nodal convergence of P1 on uniform meshes, with the Simpson load vector)
    assert all(r > 1.6 for r in rates), (errs, rates)


def test_gradcheck_fp64_jittered():
    x, cells, bnd = _mesh(6, jitter=0.3, seed=3)
    lat = torch.linspace(0.013, 0.987, 7, dtype=torch.float64)

    inner = (~bnd).nonzero().reshape(-1)
    # boxes widened by 1e-3: a box corner is a vertex whenever one vertex is extremal in x and y, and phim has a kink there
    boxes = [(lo - 1e-3, hi + 1e-3) for lo, hi in R.simpson_boxes(x, cells)]

    # interior coordinates only, Simpson boxes held: the reference detaches boundary values u_true(x_B) (difFEM_2d.py:172)
    # and the boxes (:298-309), so its gradient is the derivative with those fixed
    def f(xi):
        c, s = R.fem2d(x.index_put((inner,), xi), cells, bnd, CENTERS, SCALES, lat, boxes=boxes)
        return c, s
    assert torch.autograd.gradcheck(f, (x[inner].clone().requires_grad_(True),), eps=1e-7, atol=1e-5, rtol=1e-4)


def test_host_topology_band_and_incidence():
    pytest.importorskip('ctypes')
    from g_adaptivity_amd.fem import FemTopology
    from g_adaptivity_amd import _native_fem
    if not os.path.exists(_native_fem.LIB_PATH):
        pytest.fail("libgadapt_fem.so not built")
    meshes = [square_mesh(n) for n in (7, 12, 9)]
    cells = np.concatenate([m.cells.numpy() + off for m, off in zip(meshes, np.cumsum([0, 49, 144]))], 0)
    bnd = np.concatenate([m.boundary_nodes.numpy() for m in meshes])
    topo = FemTopology(cells, bnd, [49, 144, 81], [m.cells.shape[0] for m in meshes], 'cpu')
    h = topo.host
    for b, n in enumerate((7, 12, 9)):
        assert topo.band[b] == n - 2
        mc = cells[h['tri_mesh'] == b]
        ii = h['int_idx'][mc]
        band = 0
        for i in range(3):
            for j in range(3):
                ok = (ii[:, i] >= 0) & (ii[:, j] >= 0)
                if ok.any():
                    band = max(band, int(np.abs(ii[ok, i] - ii[ok, j]).max()))
        assert band == topo.band[b]
    seen = {}
    for v in range(cells.max() + 1):
        for e in h['nt_idx'][h['nt_ptr'][v]:h['nt_ptr'][v + 1]]:
            t, l = e >> 2, e & 3
            assert cells[t, l] == v
            seen[(t, l)] = seen.get((t, l), 0) + 1
    assert len(seen) == 3 * cells.shape[0] and set(seen.values()) == {1}


def test_pde_loss_on_1d_dataset_raises():
    ds = MeshDataset([11], 2)
    opt = hot_path_opt(mesh_dims=[11], hidden_dim=8, num_layers=2)
    opt['loss_type'] = 'pde_loss'
    with pytest.raises(NotImplementedError, match='1-D'):
        GNN(ds, opt)


def test_pde_loss_fields_only_when_asked():
    plain = MeshDataset([7, 7], 2, seed=0)
    asked = MeshDataset([7, 7], 2, seed=0, pde_loss_fields=True)
    assert not hasattr(plain.samples[0], 'u_true_fine_tensor') and not hasattr(plain, 'mapping_tensor_fine')
    u = asked.samples[0].u_true_fine_tensor
    assert u.shape == (101 * 101,) and torch.equal(asked.mapping_tensor_fine, torch.arange(101 * 101))
    q = torch.linspace(0, 1, 101).double()
    want = R.u_true(torch.stack([q[5].expand(1), q[17].expand(1)]), asked.samples[0].pde_params['centers'],
                    asked.samples[0].pde_params['scales'])
    assert abs(u[5 * 101 + 17].item() - want.item()) < 1e-6
