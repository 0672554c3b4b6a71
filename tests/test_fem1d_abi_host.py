"""What the eight 1-D entry points of libgadapt_fem.so refuse, and in which order (include/gadapt_fem.h, 1-D part).  No GPU.

As tests/test_fem_abi_host.py does for the nine 2-D ones: each case starts from an argument list that would pass every check -
dummy non-null HOST addresses, so it is never called as it is - breaks one or two arguments and asserts the return code and the
text left in gadapt_fem_last_error().  Every call here fails a check that comes before the first launch, so nothing is
launched; a case with an optional pointer set to NULL carries a second fault that a LATER check refuses, which shows the NULL
was accepted on the way there.  The expectations are read off the checks of the code before the 1-D entry points got their
shared batch descriptor (fem_csrc/fem_host.h, Fem1dBatch), entry point by entry point.

HOISTED holds what gadapt_fem1d_descend refuses before its init launch since then: load_quad_points < 2 or stiff_quad_points < 1
with epochs > 0.  Before, these reached the init launch and were refused by the first epoch's gadapt_fem1d_poisson_forward
(whose name the text keeps), so they are not part of a comparison with that code: there they would launch on host addresses.

Two things have no later check to be paired with and are pinned where the kernels run instead (tests/test_gpu_fem1d_routes_golden.py):
fine_sol = NULL with n_fine <= 1 (without a fine mesh the LDS need cannot pass the budget) and a fine mesh of 465 nodes beside
1024 (the last size the LDS check accepts is the last check of that entry point); gadapt_fem1d_lds_bytes pins the size here."""
import ctypes as C
import os
import re

import pytest

from g_adaptivity_amd import _native_fem as nf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET, CAP = 65536, 1024
_buf = (C.c_double * 64)()                                    # 8-byte aligned
P = C.addressof(_buf)
VALID = {'n_meshes': 1, 'n_sets': 1, 'max_nodes': 8, 'amp': 0.25, 'tau': 0.05, 'taunu': 5e-5, 'k_load': 5, 'k_stiff': 3, 'k_proj': 9,
         'k_proj_fine': 90, 'n_steps': 1, 'n_fine': 0, 'n_pts': 9, 'n_queries': 5, 'deriv': 0, 'epochs': 1, 'lr': 0.1,
         'mesh_params': nf.DESCEND_INTERNAL, 'n_nodes': 8, 'stream': None}

PRE = 'gadapt_fem1d_'
BATCH = 'bad batch, pointers or point count'
QUAD = 'need load_quad_points >= 2 and stiff_quad_points >= 1'
NULL = 'null pointer'


def _nodes(n, lo):
    return f'{n} nodes per mesh; {lo}..{CAP} supported (one lane per node, state in LDS)'


def _names(entry):
    decl = re.search(r'\b' + entry + r'\s*\(([^;]*)\);', open(os.path.join(ROOT, 'include', 'gadapt_fem.h')).read()).group(1)
    return [re.search(r'(\w+)\s*$', p).group(1) for p in decl.split(',')]


def _call(entry, breaks):
    names = _names(entry)
    assert len(names) == len(nf.PROTOTYPES[entry][1]) and set(breaks) <= set(names), (entry, breaks)
    assert breaks, "an unbroken argument list would be launched on host addresses"
    lib = nf.lib()
    rc = getattr(lib, entry)(*[breaks[n] if n in breaks else VALID.get(n, P) for n in names])
    return rc, lib.gadapt_fem_last_error().decode()


def _common(who, lo, late, quad=True):
    """The checks the six FEM entry points share, in their order; `late` is a fault of `who`'s own later check."""
    w = PRE + who
    out = [({k: v}, -1, f'{w}: {BATCH}') for k, v in (('n_meshes', 0), ('node_off', None), ('x', None), ('pts', None), ('n_pts', -1))]
    out += [({'max_nodes': lo - 1}, -1, f'{w}: {_nodes(lo - 1, lo)}'), ({'max_nodes': CAP + 1}, -5, f'{w}: {_nodes(CAP + 1, lo)}'),
            ({'node_off': None, 'max_nodes': lo - 1}, -1, f'{w}: {BATCH}'),                       # the order
            (dict(late, max_nodes=CAP + 1), -5, f'{w}: {_nodes(CAP + 1, lo)}')]
    if quad:
        out += [({'k_load': 1}, -1, f'{w}: {QUAD}'), ({'k_stiff': 0}, -1, f'{w}: {QUAD}'),
                ({'k_load': 1, 'max_nodes': lo - 1}, -1, f'{w}: {_nodes(lo - 1, lo)}'), (dict(late, k_stiff=0), -1, f'{w}: {QUAD}')]
    return out


def _burgers_forward():
    w = PRE + 'burgers_forward'
    own = f'{w}: bad steps, pointers, projection or fine mesh'
    lds = lambda b: f'{w}: needs {b} B of LDS, the budget is {BUDGET} B'
    big = {'max_nodes': CAP, 'n_fine': CAP}                                                     # 11 * 2048 rows: 90112 B
    out = _common('burgers_forward', 2, {'hist': None})
    out += [({k: None}, -1, own) for k in ('hist', 'sol', 'flags')]
    out += [({'n_steps': 0}, -1, own), ({'n_fine': CAP + 1}, -1, own), ({'u0': None, 'k_proj': 1}, -1, own),
            ({'u0': None, 'gptr': None}, -1, own), ({'u0': None, 'gpar': None}, -1, own),
            ({'n_fine': 2, 'fine_sol': None}, -1, own), ({'n_fine': 2, 'gptr': None}, -1, own), ({'n_fine': 2, 'gpar': None}, -1, own),
            ({'n_fine': 2, 'k_proj_fine': 1}, -1, own), (dict(big, hist=None), -1, own),
            (big, -5, lds(90112)), ({'max_nodes': CAP, 'n_fine': 466}, -5, lds(65560)),
            # optional: u0 (projection instead), bc, and with u0 given the Gaussians and k_proj
            (dict(big, u0=None), -5, lds(90112)), (dict(big, bc=None), -5, lds(90112)), (dict(big, k_proj=1), -5, lds(90112))]
    return out


def _burgers_backward():
    w = PRE + 'burgers_backward'
    own = f'{w}: bad steps or pointers'
    out = _common('burgers_backward', 2, {'gx': None})
    out += [({'n_steps': 0}, -1, own), ({'hist': None}, -1, own), ({'gx': None}, -1, own)]
    out += [({k: None, 'n_steps': 0}, -1, own) for k in ('bc', 'g_sol', 'g_last', 'gu0')]          # optional
    out += [({'bc': None, 'g_sol': None, 'g_last': None, 'gu0': None, 'gx': None}, -1, own), ({'n_pts': 0, 'pts': None, 'gx': None}, -1, own)]
    return out


def _poisson(who, required, own, optional=()):
    w = PRE + who
    out = _common(who, 3, {required[-1]: None})
    out += [({k: None}, -1, f'{w}: {own}') for k in required]
    out += [({k: None, required[-1]: None}, -1, f'{w}: {own}') for k in optional]
    return out


def _eval_errors():
    own = 'null pointer or fewer than 2 evaluation points'
    w = PRE + 'poisson_eval_errors'
    return _poisson('poisson_eval_errors', ['gptr', 'gpar', 'err', 'flags'], own) + [
        ({'n_pts': 1}, -1, f'{w}: {own}'), ({'n_pts': 0, 'pts': None}, -1, f'{w}: {own}'), ({'n_pts': 1, 'k_load': 1}, -1, f'{w}: {QUAD}')]


def _expand():
    w = PRE + 'expand'
    return _common('expand', 2, {'sol': None}, quad=False) + [
        ({'c': None}, -1, f'{w}: {NULL}'), ({'sol': None}, -1, f'{w}: {NULL}'), ({'n_pts': 0, 'pts': None, 'c': None}, -1, f'{w}: {NULL}')]


def _spline():
    w = PRE + 'spline'
    bad, deriv = f'{w}: bad batch, pointers or query count', f'{w}: deriv is 0, 1 or 2'
    size = lambda n: f'{w}: {n} points per set; 4..{CAP} supported (the set lives in LDS)'
    out = [({k: None}, -1, bad) for k in ('set_off', 'x', 'y', 'q', 'out', 'status')]
    out += [({'n_sets': 0}, -1, bad), ({'n_queries': -1}, -1, bad), ({'q_off': None, 'n_queries': 0}, -1, bad),
            ({'deriv': 3}, -1, deriv), ({'deriv': -1}, -1, deriv), ({'max_nodes': 3}, -1, size(3)), ({'max_nodes': CAP + 1}, -5, size(CAP + 1)),
            ({'x': None, 'deriv': 3}, -1, bad), ({'deriv': 3, 'max_nodes': 3}, -1, deriv),                # the order
            ({'q_off': None, 'deriv': 3}, -1, deriv), ({'q_off': None, 'max_nodes': 3}, -1, size(3)),     # optional: shared queries
            ({'n_queries': 0, 'max_nodes': CAP + 1}, -5, size(CAP + 1))]                                   # with q_off, no shared count
    return out


def _descend():
    w = PRE + 'descend'
    bad, size = f'{w}: null pointer, bad size or unknown mesh_params', f'{w}: 3..GADAPT_FEM1D_MAX_NODES nodes per mesh (one lane per node)'
    required = ['node_off', 'x', 'gptr', 'gpar', 'pts', 'coeffs', 'sol', 'flags', 'loss', 'g_sol', 'gx', 'loss_hist', 'first_tangled',
                'min_area']
    out = [({k: None}, -1, bad) for k in required]
    out += [({k: v}, -1, bad) for k, v in (('n_meshes', 0), ('epochs', -1), ('n_nodes', 0), ('n_pts', 1), ('mesh_params', 2), ('mesh_params', -1))]
    out += [({'max_nodes': 2}, -1, size), ({'max_nodes': CAP + 1}, -5, size), ({'n_pts': 1, 'max_nodes': 2}, -1, bad),   # the order
            ({'mesh_hist': None, 'max_nodes': 2}, -1, size), ({'loss_hist': None, 'epochs': 0, 'max_nodes': CAP + 1}, -5, size),   # optional
            ({'mesh_params': nf.DESCEND_ALL, 'max_nodes': 2}, -1, size),
            # the quadrature is refused after the sizes, and not at all without an epoch
            ({'k_load': 1, 'max_nodes': 2}, -1, size), ({'k_stiff': 0, 'max_nodes': CAP + 1}, -5, size),
            ({'k_load': 1, 'k_stiff': 0, 'epochs': 0, 'max_nodes': 2}, -1, size)]
    return out


TABLE = {
    PRE + 'burgers_forward': _burgers_forward(),
    PRE + 'burgers_backward': _burgers_backward(),
    PRE + 'poisson_forward': _poisson('poisson_forward', ['gptr', 'gpar', 'coeffs', 'sol', 'flags'], NULL),
    PRE + 'poisson_eval_errors': _eval_errors(),
    PRE + 'poisson_backward': _poisson('poisson_backward', ['gptr', 'gpar', 'coeffs', 'gx'], NULL, optional=('g_coeffs', 'g_sol')),
    PRE + 'expand': _expand(),
    PRE + 'spline': _spline(),
    PRE + 'descend': _descend(),
}
_HOISTED_TEXT = f'{PRE}poisson_forward: {QUAD}'
HOISTED = [({'k_load': 1, 'epochs': 1}, -1, _HOISTED_TEXT), ({'k_stiff': 0, 'epochs': 1}, -1, _HOISTED_TEXT),
           ({'k_load': 1, 'epochs': 1, 'mesh_hist': None}, -1, _HOISTED_TEXT)]
CASES = [(entry, breaks, rc, text) for entry, rows in TABLE.items() for breaks, rc, text in rows]


def _id(entry, breaks):
    return f"{entry[len(PRE):]}-{'+'.join(f'{k}={v}' if isinstance(v, int) else k for k, v in breaks.items())}"


def test_the_eight_entry_points_are_covered():
    one_d = [n for n in nf.PROTOTYPES if n.startswith(PRE) and n != PRE + 'lds_bytes']
    assert sorted(one_d) == sorted(TABLE) and len(TABLE) == 8
    assert nf.lib().gadapt_fem_lds_budget() == BUDGET


@pytest.mark.parametrize('entry,breaks,rc,text', CASES, ids=[_id(e, b) for e, b, _, _ in CASES])
def test_refusal(entry, breaks, rc, text):
    got, msg = _call(entry, breaks)
    assert (got, msg[:len(text)]) == (rc, text), (entry, breaks, got, msg)


@pytest.mark.parametrize('breaks,rc,text', HOISTED, ids=[_id(PRE + 'descend', b) for b, _, _ in HOISTED])
def test_descent_refuses_the_quadrature_before_its_first_launch(breaks, rc, text):
    got, msg = _call(PRE + 'descend', breaks)
    assert (got, msg[:len(text)]) == (rc, text), (breaks, got, msg)


@pytest.mark.parametrize('max_nodes,n_fine,want', [
    (1024, 0, 65536), (1024, 465, 65536), (1024, 466, 65560), (1024, 1024, 90112),
    # max(4 * max(11 (max_nodes + n_fine), 15 max_nodes), 64 max_nodes), a fine mesh of fewer than 2 nodes being none
    (2, 0, 128), (21, 40, 2684), (65, 130, 8580), (21, 1, 1344)])
def test_lds_bytes(max_nodes, n_fine, want):
    assert nf.lib().gadapt_fem1d_lds_bytes(max_nodes, n_fine) == want
