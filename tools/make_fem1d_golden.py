"""Golden data of the eight 1-D entry points of libgadapt_fem.so, recorded on the MI355X (tests/golden/fem1d_routes/fem1d_routes.npz).

    python tools/make_fem1d_golden.py [--out tests/golden/fem1d_routes/fem1d_routes.npz] [--force]

The fixture was recorded from the build of commit f2792f7ddd3a1b70de10fe168042cc2636142b08, the parent of the commit that put one
batch descriptor, one launch plan and one definition of each LDS layout behind the 1-D part of the FEM C-ABI:
tests/test_gpu_fem1d_routes_golden.py asserts that every later build gives the same bits.  The kernels use no float atomics and
every sum runs in a fixed order, so equality is exact; every case is computed twice here and the two runs must agree.

The cases are the smallest shapes at which host code can hand a kernel a wrong size.  load_quad_points = 5, eval_quad_points = 9,
two Gaussians per mesh and jittered interior nodes unless stated:
    poisson_mixed (3, 64, 65, 17)    the 3-node minimum, one full wave, a second wave with one live lane, small meshes in a 128-lane
                                     workgroup: fem_poisson_1d (coeffs, sol, flags, d (sol.sum() + coeffs.sum()) / d x),
                                     gradient_meshpoints_1D 'PDE_loss_direct_mse' and 'PDE_loss_direct_L2', poisson_eval_errors,
                                     mesh_descent_1d 3 epochs, lr 0.05, keep_meshes, 'internal' and 'all'
    poisson_cap (1024, 3)            the Poisson layout at exactly 65536 B: forward, gradient, eval errors, 1 epoch of descent
    poisson_default_quadrature (21,) the reference's defaults (101 load, 3 stiffness, 101 evaluation points): forward, gradient
    burgers_mixed (2, 65, 33)        3 steps, num_fine_mesh_points = 130 (the fine mesh decides the workgroup, 192 lanes, LDS
                                     11 * (65 + 130) rows): coeffs, sol, fine_sol, flags, d (sol.sum() + coeffs.sum()) / d x; and
                                     from a given u0 with explicit bc (no Gaussians, no fine mesh): the gradients in x and u0
    burgers_cap (1024,)              2 steps, num_fine_mesh_points = 465: 65516 B, the largest the forward takes; its gradient is
                                     the backward's 15 rows at 1024 nodes
    burgers_timestep_loss (17, 17)   gradient_meshpoints_1D 'burgers_timestep_loss_direct_mse', 2 steps, 40 fine points
    projection                       burgers_project on (2, 65) with k_proj = 7, get_Burgers_initial_coeffs on one 17-node mesh
    not_increasing (9, 9)            two interior nodes of the first mesh swapped, through fem_poisson_1d
    expand                           fn_expansion on 2 and on 65 nodes at 7 points including 0, 1 and a node's own coordinate
    spline                           sets of (4, 256, 5 not increasing) points - 256 is the last size of the one-wave launch - and
                                     of (257, 4), the first of the four-wave launch; deriv 0, 1, 2; queries shared and per set
The inputs are stored beside the results (keys 'in_*') and the test reads them from there.  An array of more than FULL_MAX
elements would be stored as the sha256 of its bytes beside its shape and dtype.

The fixture has a directory of its own: other tests read every .npz directly under tests/golden as a fixture of theirs.
An existing fixture is not overwritten without --force: re-recording it from a build under test proves nothing.
"""
import argparse
import hashlib
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
if os.path.abspath(ROOT) not in sys.path:
    sys.path.insert(0, os.path.abspath(ROOT))

DEFAULT_OUT = os.path.join(ROOT, 'tests', 'golden', 'fem1d_routes', 'fem1d_routes.npz')
FULL_MAX = 65536
OPT = {'load_quad_points': 5, 'eval_quad_points': 9, 'stiff_quad_points': 3, 'gauss_amplitude': 0.25, 'tau': 1 / 20.0, 'nu': 0.001}
EPOCHS, LR, K_PROJ = 3, 0.05, 7
COUNTS = {'poisson_mixed': (3, 64, 65, 17), 'poisson_cap': (1024, 3), 'poisson_default_quadrature': (21,),
          'burgers_mixed': (2, 65, 33), 'burgers_cap': (1024,), 'burgers_timestep_loss': (17, 17), 'projection': (2, 65),
          'projection_initial': (17,), 'not_increasing': (9, 9)}
SPLINE_SETS = {'a': (4, 256, 5), 'b': (257, 4)}                # 'a': one wave per set; 'b': four
SPLINE_OWN = {'a': (3, 0, 5), 'b': (6, 2)}                     # the sets' own query counts
DERIVS = (0, 1, 2)

FORWARD = ['coeffs', 'sol', 'flags', 'grad']
DESCENT = ['x', 'loss_hist', 'mesh_hist', 'first_tangled', 'min_area', 'sol']
NAMES = ([f'poisson_mixed_{w}' for w in FORWARD + ['mse_loss', 'mse_x_grads', 'L2_loss', 'L2_x_grads', 'err_L1', 'err_L2']] +
         [f'poisson_mixed_descent_{m}_{w}' for m in ('internal', 'all') for w in DESCENT] +
         [f'poisson_cap_{w}' for w in FORWARD + ['err_L1', 'err_L2']] + [f'poisson_cap_descent_internal_{w}' for w in DESCENT] +
         [f'poisson_default_quadrature_{w}' for w in FORWARD] +
         [f'burgers_mixed_{w}' for w in FORWARD + ['fine_sol', 'u0_grad_x', 'u0_grad_u0']] +
         [f'burgers_cap_{w}' for w in FORWARD + ['fine_sol']] +
         ['burgers_timestep_loss_loss', 'burgers_timestep_loss_x_grads', 'projection_u0', 'projection_initial_u0',
          'projection_initial_u0_fine'] +
         [f'not_increasing_{w}' for w in FORWARD] + ['expand_2', 'expand_65'] +
         [f'spline_{c}_{q}_d{d}_{w}' for c in SPLINE_SETS for q in ('shared', 'own') for d in DERIVS for w in ('values', 'status')])


def pack(a):
    a = np.ascontiguousarray(a)
    if a.size <= FULL_MAX:
        return a
    tag = f"{hashlib.sha256(a.tobytes()).hexdigest()} {a.shape} {a.dtype}"
    return np.frombuffer(tag.encode(), dtype=np.uint8).copy()


def _jittered(n, g):
    u = torch.linspace(0, 1, n)
    if n > 2:
        u = u + (torch.rand(n, generator=g) * 2 - 1) * 0.3 / (n - 1)
        u[0], u[-1] = 0.0, 1.0
    return u


def inputs():
    """What the fixture stores of the inputs, as float32 arrays named 'in_<case>_<what>'."""
    g = torch.Generator().manual_seed(1024)
    rng = np.random.default_rng(1024)
    inp = {}
    for case, counts in COUNTS.items():
        inp[f'in_{case}_x'] = torch.cat([_jittered(n, g) for n in counts]).numpy()
        inp[f'in_{case}_centers'] = rng.uniform(0.3, 0.7, (len(counts), 2)).astype(np.float32)
        inp[f'in_{case}_scales'] = rng.uniform(0.05, 0.2, (len(counts), 2)).astype(np.float32)
    x = inp['in_not_increasing_x']
    x[3], x[4] = x[4], x[3]
    n = sum(COUNTS['burgers_mixed'])
    inp['in_burgers_mixed_u0'] = rng.uniform(-0.2, 0.2, n).astype(np.float32)
    inp['in_burgers_mixed_bc'] = rng.uniform(-0.1, 0.1, (len(COUNTS['burgers_mixed']), 2)).astype(np.float32)
    for n in (2, 65):
        mesh = _jittered(n, g).numpy()
        inp[f'in_expand_{n}_x'] = mesh
        inp[f'in_expand_{n}_c'] = rng.uniform(-1, 1, n).astype(np.float32)
        inp[f'in_expand_{n}_pts'] = np.array([0.0, mesh[n // 3], 0.13, 0.5, 0.77, 0.999, 1.0], np.float32)
    for c, sets in SPLINE_SETS.items():
        xs = [_jittered(n, g).numpy().copy() for n in sets]
        if c == 'a':
            xs[2][2] = xs[2][1]                                 # not increasing: two equal abscissae
        inp[f'in_spline_{c}_x'] = np.concatenate(xs)
        inp[f'in_spline_{c}_y'] = rng.uniform(-1, 1, sum(sets)).astype(np.float32)
        inp[f'in_spline_{c}_q_own'] = rng.uniform(-0.05, 1.05, sum(SPLINE_OWN[c])).astype(np.float32)
    inp['in_spline_q_shared'] = np.linspace(-0.1, 1.1, 11).astype(np.float32)
    return inp


def compute(inp, dev):
    """Every recorded result from the stored inputs, as a dict of numpy arrays named as in NAMES."""
    from g_adaptivity_amd import cubic_spline_1d, poisson_eval_errors
    from g_adaptivity_amd.descent import mesh_descent_1d
    from g_adaptivity_amd.evaluation_burgers import burgers_project
    from g_adaptivity_amd.fem1d import (burgers_1d, fem_poisson_1d, fn_expansion, get_Burgers_initial_coeffs, gradient_meshpoints_1D,
                                        last_flags)
    t = lambda key: torch.from_numpy(np.asarray(inp[key])).to(dev)
    out = {}

    def params(case):
        c, s = inp[f'in_{case}_centers'], inp[f'in_{case}_scales']
        return [{'centers': list(c[b]), 'scales': list(s[b])} for b in range(c.shape[0])]

    def forward(case, fn, *more):
        """coeffs, sol, flags and d (sol.sum() + coeffs.sum()) / d x of one forward; fn(x) returns coeffs, sol and the rest."""
        xg = t(f'in_{case}_x').requires_grad_(True)
        coeffs, sol, *rest = fn(xg)
        flags = last_flags().clone()
        (sol.sum() + coeffs.sum()).backward()
        out.update({f'{case}_coeffs': coeffs.detach(), f'{case}_sol': sol.detach(), f'{case}_flags': flags, f'{case}_grad': xg.grad})
        for name, v in zip(more, rest):
            out[f'{case}_{name}'] = v.detach()

    def modular(case, gt, tag, opt):
        counts = COUNTS[case]
        data = types.SimpleNamespace(pde_params=params(case), batch=torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts)))
        loss, gx = gradient_meshpoints_1D(dict(opt, grad_type=gt), data, t(f'in_{case}_x'))
        out.update({f'{case}_{tag}loss': loss, f'{case}_{tag}x_grads': gx})

    def descent(case, mode, epochs):
        r = mesh_descent_1d(t(f'in_{case}_x'), COUNTS[case], params(case), OPT, epochs, LR, mesh_params=mode, keep_meshes=True)
        for w in DESCENT:
            out[f'{case}_descent_{mode}_{w}'] = getattr(r, w)

    for case, opt in (('poisson_mixed', OPT), ('poisson_cap', OPT), ('poisson_default_quadrature', {}), ('not_increasing', OPT)):
        forward(case, lambda x: fem_poisson_1d(x, COUNTS[case], params(case), opt))
    for case in ('poisson_mixed', 'poisson_cap'):
        l1, l2 = poisson_eval_errors(t(f'in_{case}_x'), COUNTS[case], params(case), OPT['eval_quad_points'], opt=OPT)
        out.update({f'{case}_err_L1': l1, f'{case}_err_L2': l2})
    modular('poisson_mixed', 'PDE_loss_direct_mse', 'mse_', OPT)
    modular('poisson_mixed', 'PDE_loss_direct_L2', 'L2_', OPT)
    descent('poisson_mixed', 'internal', EPOCHS)
    descent('poisson_mixed', 'all', EPOCHS)
    descent('poisson_cap', 'internal', 1)

    for case, steps, n_fine in (('burgers_mixed', 3, 130), ('burgers_cap', 2, 465)):
        o = dict(OPT, num_fine_mesh_points=n_fine)
        forward(case, lambda x: burgers_1d(x, COUNTS[case], params(case), o, steps), 'fine_sol')
    xg, u0 = t('in_burgers_mixed_x').requires_grad_(True), t('in_burgers_mixed_u0').requires_grad_(True)
    coeffs, sol, _ = burgers_1d(xg, COUNTS['burgers_mixed'], None, OPT, 3, u0=u0, bc=t('in_burgers_mixed_bc'), fine=False)
    (sol.sum() + coeffs.sum()).backward()
    out.update({'burgers_mixed_u0_grad_x': xg.grad, 'burgers_mixed_u0_grad_u0': u0.grad})
    modular('burgers_timestep_loss', 'burgers_timestep_loss_direct_mse', '', dict(OPT, num_time_steps=2, num_fine_mesh_points=40))

    out['projection_u0'] = burgers_project(t('in_projection_x'), COUNTS['projection'], params('projection'), OPT, k_proj=K_PROJ)
    a, b = get_Burgers_initial_coeffs(torch.linspace(0, 1, 40, device=dev), 40, t('in_projection_initial_x'), 17,
                                      params('projection_initial')[0], OPT['load_quad_points'], OPT)
    out.update({'projection_initial_u0': a, 'projection_initial_u0_fine': b})
    for n in (2, 65):
        out[f'expand_{n}'] = fn_expansion(t(f'in_expand_{n}_c'), t(f'in_expand_{n}_x'), t(f'in_expand_{n}_pts'))
    for c, sets in SPLINE_SETS.items():
        for q, key, q_counts in (('shared', 'in_spline_q_shared', None), ('own', f'in_spline_{c}_q_own', SPLINE_OWN[c])):
            for d in DERIVS:
                v, st = cubic_spline_1d(t(f'in_spline_{c}_x'), t(f'in_spline_{c}_y'), sets, t(key), q_counts=q_counts, deriv=d)
                out.update({f'spline_{c}_{q}_d{d}_values': v, f'spline_{c}_{q}_d{d}_status': st})
    torch.cuda.synchronize()
    return {k: pack(v.cpu().numpy()) for k, v in out.items()}


def computed(inp, dev):
    """compute() without the warning about the mesh that is not increasing, which the case is there to provoke."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return compute(inp, dev)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


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
    res, again = computed(inp, dev), computed(inp, dev)
    assert sorted(res) == sorted(NAMES), sorted(set(res) ^ set(NAMES))
    differ = [k for k in NAMES if not same_bits(res[k], again[k])]
    assert not differ, f"two runs of the same build differ in {differ}: these kernels are not bitwise repeatable"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez(args.out, **inp, **res)
    print(f"{len(res)} arrays, {os.path.getsize(args.out)} bytes -> {os.path.normpath(args.out)}")
    for k in NAMES:
        v = res[k]
        fin = np.isfinite(v).all() if v.dtype.kind == 'f' else True
        print(f"  {k:44s} {v.shape!s:12s} |max| {np.nanmax(np.abs(v.astype(np.float64))) if v.size else 0:.6g}{'' if fin else '  (not all finite)'}")


if __name__ == '__main__':
    main()
