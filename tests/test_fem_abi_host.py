"""What the nine 2-D entry points of libgadapt_fem.so refuse, and in which order (include/gadapt_fem.h).  No GPU.

Each case starts from an argument list that would pass every check - dummy non-null HOST addresses, so it is never called as
it is - breaks one or two arguments and asserts the return code and the text left in gadapt_fem_last_error().  Every call
here fails a check, and the checks come before the first launch, so nothing is launched; a case with an optional pointer
set to NULL carries a second fault that a LATER check refuses, which shows the NULL was accepted on the way there.  The
expectations are read off the checks of the code that first exported these nine symbols with ABI 4, entry point by entry
point, including where they differ: gadapt_fem_forward has no `nlat * nlat` range check, gadapt_fem_modular_forward reports
the shared arguments under gadapt_fem_forward's name, the windowed entry points refuse tri_slab before the ring."""
import ctypes as C
import os
import re

import pytest

from g_adaptivity_amd import _native_fem as nf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 65536
_buf = (C.c_double * 64)()                                    # 8-byte aligned
P = C.addressof(_buf)
_lat = (C.c_float * 4)(0.0, 0.5, 1.0, 0.0)
PL = C.addressof(_lat)
VALID = {'n_meshes': 1, 'n_nodes': 4, 'n_tris': 2, 'nlat': 3, 'max_lds_bytes': 1024, 'max_tris': 2, 'reduction': nf.LOSS_MSE,
         'tri_slab': 0, 'epochs': 1, 'lr': 0.1, 'stream': None, 'lat_x': PL, 'lat_y': PL}
HEAD = ['meta', 'cells', 'node_mesh', 'int_idx', 'int_node', 'nt_ptr', 'nt_idx', 'gptr', 'gpar', 'x']

NULL = 'null pointer or bad size'
LAT = 'evaluation lattice: need lat_x, lat_y and nlat >= 2'
BAND = 'band factor: LDS bytes outside'
MASK = 'evaluation: triangle bin mask exceeds the LDS budget'
RING = "windowed band: the ring's LDS bytes are outside"
SLAB_MASK = "windowed evaluation: tri_slab's bin mask exceeds the LDS budget"


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


def _shared(who, required, sizes, lds_msg, tail):
    """The checks an entry point shares with the others, in their order; `tail` is a later fault of the same entry point."""
    out = [({p: None}, -1, f'{who}: {NULL}') for p in HEAD + required]
    out += [({s: 0}, -1, f'{who}: {NULL}') for s in sizes]
    out += [({'lat_x': None}, -1, LAT), ({'lat_y': None}, -1, LAT), ({'nlat': 1}, -1, LAT)]
    out += [({'max_lds_bytes': 0}, -5, lds_msg), ({'max_lds_bytes': BUDGET + 1}, -5, lds_msg)]
    out += [({'meta': None, 'nlat': 1}, -1, f'{who}: {NULL}'), ({'nlat': 1, 'max_lds_bytes': 0}, -1, LAT)]   # the order
    out += [(dict(tail[0], meta=None), -1, f'{who}: {NULL}')]
    return out


def _loss(who, next_who):
    """The loss arguments of a modular forward: before the shared ones."""
    bad, simpson, rows = f'{who}: null output or unknown reduction', f'{who}: the Simpson rule needs an odd nlat >= 3', \
        f"{who}: the lattice's row sums exceed the LDS budget"
    return [({'loss': None}, -1, bad), ({'g_sol': None}, -1, bad), ({'reduction': 2}, -1, bad), ({'n_meshes': 0}, -1, bad),
            ({'reduction': nf.LOSS_SIMPSON, 'nlat': 4}, -1, simpson), ({'reduction': nf.LOSS_SIMPSON, 'nlat': 1}, -1, simpson),
            ({'nlat': 16385}, -5, rows), ({'nlat': 16385, 'reduction': nf.LOSS_SIMPSON}, -5, rows),
            ({'reduction': 2, 'meta': None}, -1, bad), ({'reduction': nf.LOSS_SIMPSON, 'nlat': 4, 'meta': None}, -1, simpson),
            ({'nlat': 16385, 'meta': None}, -5, rows), ({'reduction': nf.LOSS_SIMPSON, 'meta': None}, -1, f'{next_who}: {NULL}')]


SIZES = ['n_meshes', 'n_nodes', 'n_tris', 'max_tris']


def _lds_forward(who, sizes=SIZES, big_nlat=46341):
    """gadapt_fem_forward's checks (under `who`): lfac and sol come last, and nlat has no upper limit."""
    late = ({'sol': None}, -1, f'{who}: {NULL}')
    return _shared(who, ['rhs', 'coeffs'], sizes, BAND, late) + [
        ({'max_tris': 2049}, -5, MASK), ({'max_lds_bytes': 0, 'max_tris': 2049}, -5, BAND),
        ({'lfac': None}, -1, f'{who}: {NULL}'), late, ({'lfac': None, 'max_lds_bytes': 0}, -5, BAND),
        ({'sol': None, 'max_tris': 2049}, -5, MASK), ({'nlat': big_nlat, 'sol': None}, -1, f'{who}: {NULL}')]


def _window_forward(who, outputs, sizes=SIZES, nlat_range=True):
    """The windowed forward entry points: workspace, outputs and sizes at once, the lattice, nlat's range, tri_slab, the ring."""
    slab, rng = f'{who}: tri_slab must be 0 or a positive multiple of 32', f'{who}: nlat * nlat exceeds the int range'
    late = ({'tri_slab': 31}, -1, slab)
    ranged = [({'nlat': 46341}, -1, rng), ({'nlat': 46341, 'tri_slab': 31}, -1, rng), ({'lat_x': None, 'nlat': 46341}, -1, LAT)]
    return _shared(who, ['rhs', 'coeffs', 'work'] + outputs, sizes, RING, late) + (ranged if nlat_range else []) + [
        ({'work': P + 4}, -1, f'{who}: {NULL}'), ({'work': P + 4, 'max_lds_bytes': 0}, -1, f'{who}: {NULL}'),
        late, ({'tri_slab': -32}, -1, slab), ({'tri_slab': 31, 'max_lds_bytes': 0}, -1, slab),
        ({'tri_slab': 32 * 65}, -5, SLAB_MASK), ({'tri_slab': 32 * 65, 'max_lds_bytes': 0}, -5, RING)]


def _backward(who, factor, lds_msg):
    """The backward entry points: tri_mesh is required, g_coeffs and g_sol are not, nlat has no upper limit."""
    late = ({'max_lds_bytes': 0}, -5, lds_msg)
    out = _shared(who, ['tri_mesh', 'coeffs', factor, 'gc', 'mu', 'tgrad', 'gx'], ['n_meshes', 'n_nodes', 'n_tris'], lds_msg, late)
    out += [({'g_coeffs': None, 'max_lds_bytes': 0}, -5, lds_msg), ({'g_sol': None, 'max_lds_bytes': 0}, -5, lds_msg),
            ({'g_coeffs': None, 'g_sol': None, 'nlat': 46341, 'max_lds_bytes': BUDGET + 1}, -5, lds_msg)]
    if factor == 'work':
        out += [({'work': P + 4}, -1, f'{who}: {NULL}'), ({'work': P + 4, 'max_lds_bytes': 0}, -1, f'{who}: {NULL}')]
    return out


def _descend():
    who = 'gadapt_fem_descend'
    simpson, lds = f'{who}: the Simpson rule needs an odd nlat >= 3', f'{who}: band factor or triangle bin mask outside the LDS budget'
    required = HEAD + ['tri_mesh', 'lat_x', 'lat_y', 'rhs', 'coeffs', 'lfac', 'sol', 'loss', 'g_sol', 'gc', 'mu', 'tgrad', 'gx',
                       'loss_hist', 'first_tangled', 'min_area', 'sign']
    out = [({p: None}, -1, f'{who}: {NULL}') for p in required]
    out += [({s: 0}, -1, f'{who}: {NULL}') for s in SIZES]
    out += [({'epochs': -1}, -1, f'{who}: {NULL}'), ({'epochs': -1, 'nlat': 4}, -1, f'{who}: {NULL}'),
            ({'nlat': 1}, -1, simpson), ({'nlat': 4}, -1, simpson), ({'nlat': 4, 'max_lds_bytes': 0}, -1, simpson),
            ({'max_lds_bytes': 0}, -5, lds), ({'max_lds_bytes': BUDGET + 1}, -5, lds), ({'max_tris': 2049}, -5, lds),
            ({'x_ref': None, 'max_lds_bytes': 0}, -5, lds), ({'mesh_hist': None, 'max_lds_bytes': 0}, -5, lds),
            ({'loss_hist': None, 'epochs': 0, 'max_lds_bytes': 0}, -5, lds), ({'nlat': 46341, 'max_lds_bytes': 0}, -5, lds)]
    return out


def _eval_errors():
    who = 'gadapt_fem_eval_errors'
    rng = f'{who}: nlat * nlat exceeds the int range'
    late = ({'nlat': 46341}, -1, rng)
    return _shared(who, ['rhs', 'coeffs'], SIZES, BAND, late) + [
        ({'max_tris': 2049}, -5, MASK), ({'partials': None}, -1, f'{who}: {NULL}'), ({'err': None}, -1, f'{who}: {NULL}'),
        ({'partials': None, 'max_lds_bytes': 0}, -5, BAND), ({'partials': None, 'nlat': 46341}, -1, f'{who}: {NULL}'),
        late, ({'lfac': None, 'nlat': 46341}, -1, rng), ({'max_tris': 2049, 'nlat': 46341}, -5, MASK)]


F, FW = 'gadapt_fem_forward', 'gadapt_fem_forward_window'
M, MW = 'gadapt_fem_modular_forward', 'gadapt_fem_modular_forward_window'
TABLE = {
    F: _lds_forward(F),
    'gadapt_fem_eval_errors': _eval_errors(),
    M: _loss(M, F) + _lds_forward(F, SIZES[1:], 16384),                                    # the shared arguments: under gadapt_fem_forward's name
    'gadapt_fem_backward': _backward('gadapt_fem_backward', 'lfac', BAND),
    FW: _window_forward(FW, ['sol']),
    'gadapt_fem_eval_errors_window': _window_forward('gadapt_fem_eval_errors_window', ['partials', 'err']),
    MW: _loss(MW, MW) + _window_forward(MW, ['sol'], SIZES[1:], nlat_range=False),   # its row-sum check refuses such an nlat first
    'gadapt_fem_backward_window': _backward('gadapt_fem_backward_window', 'work', RING),
    'gadapt_fem_descend': _descend(),
}
CASES = [(entry, breaks, rc, text) for entry, rows in TABLE.items() for breaks, rc, text in rows]


def test_the_nine_entry_points_are_covered():
    two_d = [n for n in nf.PROTOTYPES if re.fullmatch(r'gadapt_fem_(forward|eval_errors|modular_forward|backward)(_window)?|gadapt_fem_descend', n)]
    assert sorted(two_d) == sorted(TABLE) and len(TABLE) == 9
    assert nf.lib().gadapt_fem_lds_budget() == BUDGET


@pytest.mark.parametrize('entry,breaks,rc,text', CASES,
                         ids=[f"{e[11:]}-{'+'.join(f'{k}={v}' if isinstance(v, int) and k != 'work' else k for k, v in b.items())}"
                              for e, b, _, _ in CASES])
def test_refusal(entry, breaks, rc, text):
    got, msg = _call(entry, breaks)
    assert (got, msg[:len(text)]) == (rc, text), (entry, breaks, got, msg)
