"""Golden data of the 2-D FEM tails on both band routes, recorded on the MI355X (tests/golden/fem2d_routes/fem2d_routes.npz).

    python tools/make_fem2d_golden.py [--out tests/golden/fem2d_routes/fem2d_routes.npz] [--force]

The fixture was recorded from the build of commit 6375237b1671b02cfd70689fe7b3a4508bcbda64, the parent of the commit that put
one batch descriptor and one launch plan behind the FEM C-ABI: tests/test_gpu_fem_routes_golden.py asserts that every later
build gives the same bits.  The kernels use no float atomics and every sum runs in a fixed order, so equality is exact.

One mixed batch of three meshes (tests/fem_meshes.py), the smallest that reaches every launch sequence on both routes:
    square_mesh(3)                                       one unknown, band 0, no pairs
    union_jack(5)                                        valences 4 and 8
    permuted(square_mesh(12), perm=far_swap(12, 78))     100 unknowns, band 78: the windowed ring (R = 82 rows) wraps, and its
                                                         6241 fp32 band entries still fit the resident-band route
Interior nodes jittered, two Gaussians per mesh, 9 lattice points per dimension.  Per route ('lds', 'window'):
    fem_poisson                                  coeffs, sol, d (sol.sum() + coeffs.sum()) / d x
    modular_loss_2d 'mse' and 'simpson'          loss, x_grads
    poisson_eval_errors, n_eval = 17             L1, L2
'lds' only: mesh_descent_2d, 3 epochs, keep_meshes -> x, loss_hist, mesh_hist, first_tangled, min_area.
'window' only: everything again with tri_slab = 32, which must equal tri_slab = 0 (asserted here and in the test).
The inputs (x, centers, scales) are stored beside the results and the test reads them from there.

The fixture has a directory of its own: other tests read every .npz directly under tests/golden as a fixture of theirs.
An existing fixture is not overwritten without --force: re-recording it from a build under test proves nothing.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if os.path.abspath(p) not in sys.path:
        sys.path.insert(0, os.path.abspath(p))

N_LAT, N_EVAL, EPOCHS, LR, BAND_WIDE = 9, 17, 3, 0.05, 78
ROUTES = ('lds', 'window')
DEFAULT_OUT = os.path.join(ROOT, 'tests', 'golden', 'fem2d_routes', 'fem2d_routes.npz')


def topology():
    """(x0 [N,2] unjittered, cells [T,3], boundary [N], node_counts, tri_counts) of the mixed batch, cells offset per mesh."""
    import fem_meshes as F
    from g_adaptivity_amd.mesh_graph import square_mesh
    m3, m12 = square_mesh(3), square_mesh(12)
    parts = [(m3.x_comp.clone(), torch.as_tensor(m3.cells), torch.as_tensor(m3.boundary_nodes)),
             F.union_jack(5),
             F.permuted(m12, m12.x_comp.clone(), perm=F.far_swap(12, BAND_WIDE))[:3]]
    assert F.band_of(parts[2][1], parts[2][2]) == BAND_WIDE
    xs, cs, bs, off = [], [], [], 0
    for x, cells, bnd in parts:
        xs.append(x.float())
        cs.append(cells.long() + off)
        bs.append(bnd.bool())
        off += x.shape[0]
    return torch.cat(xs), torch.cat(cs), torch.cat(bs), [p[0].shape[0] for p in parts], [p[1].shape[0] for p in parts]


def inputs():
    """What the fixture stores of the inputs: the jittered coordinates and the Gaussians, [3 meshes, 2 Gaussians, 2]."""
    x0, _, bnd, node_counts, _ = topology()
    g = torch.Generator().manual_seed(78)
    x, off = x0.clone(), 0
    for n in node_counts:                                              # a fifth of the mesh width, boundary nodes stay
        side = int(round(n ** 0.5))
        d = (torch.rand(n, 2, generator=g) * 2 - 1) * 0.2 / (side - 1)
        d[bnd[off:off + n]] = 0.0
        x[off:off + n] += d
        off += n
    rng = np.random.default_rng(78)
    return {'in_x': x.numpy(), 'in_centers': rng.uniform(0.2, 0.8, (3, 2, 2)).astype(np.float32),
            'in_scales': rng.uniform(0.15, 0.5, (3, 2, 2)).astype(np.float32)}


def compute(inp, dev, tri_slab=0):
    """Every recorded result from the stored inputs, as a dict of numpy arrays named '<route>_<what>'."""
    from g_adaptivity_amd import _native_fem, fem_poisson, poisson_eval_errors
    from g_adaptivity_amd.descent import mesh_descent_2d
    from g_adaptivity_amd.fem import _topology, modular_loss_2d
    _, cells, bnd, node_counts, tri_counts = topology()
    params = [{'centers': list(inp['in_centers'][b]), 'scales': list(inp['in_scales'][b])} for b in range(3)]
    x = torch.from_numpy(np.asarray(inp['in_x'])).to(dev)
    lat = torch.linspace(0, 1, N_LAT)
    quad = list(torch.meshgrid(lat, lat, indexing='ij'))
    topo = _topology(cells, bnd, node_counts, tri_counts, dev, 'lds')
    lib = _native_fem.lib()
    need = int(lib.gadapt_fem_factor_lds_bytes(int(topo.n_int[2]), int(topo.band[2])))
    assert int(topo.band[2]) == BAND_WIDE and int(topo.n_int[2]) == 100 and need <= int(lib.gadapt_fem_lds_budget()), need
    out = {}
    for route in ROUTES:
        kw = dict(tri_counts=tri_counts, band=route, tri_slab=tri_slab if route == 'window' else 0)
        xg = x.clone().requires_grad_(True)
        coeffs, sol = fem_poisson(xg, cells, bnd, node_counts, params, quad, **kw)
        (sol.sum() + coeffs.sum()).backward()
        out.update({f'{route}_coeffs': coeffs.detach(), f'{route}_sol': sol.detach(), f'{route}_grad': xg.grad})
        for red in ('mse', 'simpson'):
            loss, gx = modular_loss_2d(x, cells, bnd, node_counts, params, N_LAT, red, **kw)
            out.update({f'{route}_{red}_loss': loss, f'{route}_{red}_x_grads': gx})
        l1, l2 = poisson_eval_errors(x, node_counts, params, N_EVAL, cells=cells, boundary=bnd, **kw)
        out.update({f'{route}_L1': l1, f'{route}_L2': l2})
    res = mesh_descent_2d(x, cells, bnd, node_counts, params, EPOCHS, LR, keep_meshes=True, tri_counts=tri_counts)
    out.update({'lds_descent_x': res.x, 'lds_descent_loss_hist': res.loss_hist, 'lds_descent_mesh_hist': res.mesh_hist,
                'lds_descent_first_tangled': res.first_tangled, 'lds_descent_min_area': res.min_area})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=DEFAULT_OUT)
    ap.add_argument('--force', action='store_true', help='overwrite an existing fixture')
    args = ap.parse_args()
    if os.path.exists(args.out) and not args.force:
        sys.exit(f"{os.path.normpath(args.out)} exists; --force overwrites it (only from a build that is not under test)")
    assert torch.cuda.is_available(), "the fixture is recorded on the MI355X"
    dev = torch.device('cuda:0')
    inp = inputs()
    res = compute(inp, dev)
    slab = compute(inp, dev, tri_slab=32)
    for k, v in res.items():
        assert np.array_equal(v, slab[k], equal_nan=True), f"{k}: tri_slab = 32 differs from tri_slab = 0"
        assert np.isfinite(v).all(), k
    np.savez(args.out, **inp, **res)
    print(f"{len(res)} arrays, {os.path.getsize(args.out)} bytes -> {os.path.normpath(args.out)}")
    for k in sorted(res):
        print(f"  {k:28s} {res[k].shape!s:14s} |max| {np.abs(res[k]).max():.6g}")


if __name__ == '__main__':
    main()
