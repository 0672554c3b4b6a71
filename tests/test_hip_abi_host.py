"""What the message-passing entry points of libgadapt_hip.so refuse, and in which order (include/gadapt_hip.h).  No GPU.

Each case starts from an argument list that would pass every check - a gadapt_graph whose pointer fields are dummy non-null
HOST addresses, so it is never called as it is - breaks one or two arguments and asserts the return code and the text left
in gadapt_last_error().  Every call here fails a check before anything is launched; a case with an optional pointer set to
NULL carries a second fault that a LATER check refuses, which shows the NULL was accepted on the way there.  A break named
'g.<field>' changes that field of the graph, 'g' itself passes NULL for it.  Refusals that can only be reached after a launch
(the narrow backward's source-side checks, the loss partial count) are not here.  The expectations are read off the checks of
ABI 9 as first released, entry point by entry point, including their quirks: gadapt_block_backward sizes the slab (and refuses
the hidden size there) before it looks for the source CSR, which it does inside its layer loop; gadapt_block_forward_loss
checks x_comp and the loss arguments before the graph."""
import ctypes as C
import os
import re

import pytest

from g_adaptivity_amd import _native as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_buf = (C.c_double * 2048)()
P = C.addressof(_buf)
BAD = -1

GRAPH = 'bad graph'
META = 'graph without tile metadata (gadapt_tile_meta_host)'
GIB = 'n_nodes*C*4 must stay below 4 GiB (32-bit row offsets)'
HIDDEN = 'hidden_dim must be one of 4, 8, 16, 32, 64, 128'
G_COLS = 'compact upstream gradient: 1..4 columns'
# a row-major batch the wide forward takes with eight-wave workgroups: 64 steps of 256 nodes (gadapt_narrow_route = 1,
# gadapt_forward_computes_coeffs = 1 at hidden 64, enough workgroups for the in-kernel coefficients)
GRAPH_VALID = dict(n_nodes=16384, n_edges=65536, wide_deg_t=5, wide_deg_s=5, wide_big_deg_t=0, wide_half_deg_t=0)
GRAPH_POINTERS = ['rowptr_t', 'col_t', 'rowptr_s', 'col_s', 'perm_s', 'tpos_s', 'ell_t', 'ell_s']


def _graph(breaks):
    g = nv.GadaptGraph()
    for k, v in GRAPH_VALID.items():
        setattr(g, k, v)
    for i, k in enumerate(GRAPH_POINTERS):
        setattr(g, k, P + 64 * (i + 1))
    for k in range(3):
        g.meta_t[k], g.meta_s[k] = P + 1024 + 64 * k, P + 2048 + 64 * k
    for k, v in breaks.items():
        m = re.fullmatch(r'g\.(meta_[ts])\[(\d)\]', k)
        if m:
            getattr(g, m.group(1))[int(m.group(2))] = v
        else:
            assert hasattr(g, k[2:]), k
            setattr(g, k[2:], v)
    return g


VALID = {'n_layers': 3, 'c': 64, 'x0_cols': 4, 'a_stride': 0, 'p0_stride': 0, 'residual_only': 0, 'accumulate': 0, 'stream': None,
         'dim': 2, 'd': 2, 'l1': 0, 'g_top_cols': 2, 'want_d_scale': 0, 'n_rows': 4, 'n_loss_partials': 8, 'loss_count': 100,
         'lr': 1e-3, 'beta1': 0.9, 'beta2': 0.999, 'eps': 1e-8, 'weight_decay': 0.0, 'grad_scale': 1.0, 'want_source': 0,
         'n_nodes': 1024, 'halo': 32}
# what the compact and narrow backward take NULL for (they refuse a pointer there)
NO_GRADS = {'d_x0': None, 'd_layer_params': None}
VALID_OF = {'gadapt_block_backward': {'d_x0': None}, 'gadapt_block_backward_narrow': NO_GRADS, 'gadapt_block_backward_narrow_packed': NO_GRADS}


def _names(entry):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'gadapt_hip.h')).read(), flags=re.S)
    decl = re.search(r'\b' + entry + r'\s*\(([^;{]*)\);', text).group(1)
    return [re.search(r'(\w+)\s*$', p).group(1) for p in decl.split(',')]


def _call(entry, breaks):
    names = _names(entry)
    args_of = {k: v for k, v in breaks.items() if not k.startswith('g.')}
    assert len(names) == len(nv.PROTOTYPES[entry][1]) and set(args_of) <= set(names), (entry, breaks)
    assert breaks, "an unbroken argument list would be launched on host addresses"
    graph = _graph({k: v for k, v in breaks.items() if k.startswith('g.')})
    valid = dict(VALID, **VALID_OF.get(entry, {}))
    args = []
    for i, n in enumerate(names):
        if n in args_of:
            args.append(args_of[n])
        elif n == 'g':
            args.append(C.byref(graph))
        else:
            args.append(valid.get(n, P + 4096 + 16 * i))             # every pointer argument its own address: none aliases another
    lib = nv.lib()
    rc = getattr(lib, entry)(*args)
    return rc, lib.gadapt_last_error().decode()


def _check_graph(later):
    """check_graph's refusals in their order; `later` is a fault of the same entry point that a later check refuses."""
    out = [({'g': None}, GRAPH), ({'g.n_nodes': 0}, GRAPH), ({'g.n_edges': -1}, GRAPH), ({'g.rowptr_t': None}, GRAPH), ({'g.col_t': None}, GRAPH)]
    out += [({f'g.meta_{s}[{k}]': None}, META) for s in 'ts' for k in range(3)]
    out += [({'g.n_nodes': 1 << 24}, GIB), ({'g.n_nodes': 0, 'g.meta_t[0]': None}, GRAPH), ({'g.meta_s[2]': None, 'g.n_nodes': 1 << 24}, META)]
    out += [(dict(later, **{'g.col_t': None}), GRAPH), (dict(later, **{'g.n_nodes': 1 << 24}), GIB)]
    return out


def _nulls(names, msg):
    return [({n: None}, msg) for n in names]


def _layer_forward():
    nul = 'layer_forward: null or aliased pointer'
    return _check_graph({'x_in': None}) + _nulls(['x_in', 'x_out', 'a', 'p0', 'layer_params'], nul) + [
        ({'x_in': P, 'x_out': P}, nul), ({'c': 12}, HIDDEN), ({'c': 0}, HIDDEN), ({'x_in': None, 'c': 12}, nul), ({'alpha_out': None, 'c': 12}, HIDDEN)]


def _layer_backward():
    nul, csr, alias = 'layer_backward: null pointer', 'layer_backward: source CSR missing', 'layer_backward: g_out aliases an input'
    return _check_graph({'slab': None}) + _nulls(['x_in', 'g_in', 'alpha', 'a', 'p0', 'layer_params', 'edge_ws', 'dxd_ws', 'slab'], nul) + [
        ({'g.tpos_s': None}, csr), ({'g.rowptr_s': None}, csr), ({'g.col_s': None}, csr), ({'g.tpos_s': None, 'g_out': None}, csr),
        ({'g_out': P, 'g_in': P}, alias), ({'g_out': P, 'dxd_ws': P}, alias), ({'c': 12}, HIDDEN),
        ({'slab': None, 'g.tpos_s': None}, nul), ({'g.tpos_s': None, 'g_out': P, 'g_in': P}, csr), ({'g_out': P, 'g_in': P, 'c': 12}, alias),
        ({'g_out': None, 'g.rowptr_s': None, 'g.col_s': None, 'c': 12}, HIDDEN), ({'sums_out': None, 'c': 12}, HIDDEN)]


def _block_forward(narrow):
    bad, compact = 'block_forward: bad argument', 'block_forward: compact x0 needs 4 columns, >= 2 layers, hidden >= 8'
    out = _check_graph({'x_all': None}) + _nulls(['x_all', 'a', 'p0', 'layer_params'], bad) + [
        ({'n_layers': 0}, bad), ({'x0_cols': 3}, compact), ({'n_layers': 1}, compact), ({'c': 4}, compact),
        ({'x_all': None, 'x0_cols': 3}, bad), ({'n_layers': 0, 'c': 4}, bad)]
    if narrow:
        nar = 'block_forward (narrow): compact x0, head rows, hidden 64 on a graph the wide forward takes (gadapt_narrow_route)'
        out += [({'x0_cols': 0}, nar), ({'x_top4': None}, nar), ({'c': 32}, nar), ({'c': 128}, nar), ({'g.ell_t': None}, nar),
                ({'g.wide_deg_t': 0}, nar), ({'g.wide_deg_t': 0, 'g.wide_big_deg_t': 8}, nar),
                ({'x0_cols': 3, 'x_top4': None}, compact), ({'n_layers': 1, 'c': 32}, compact), ({'alpha_all': None, 'x_top4': None}, nar)]
    else:
        out += [({'c': 12}, HIDDEN), ({'x0_cols': 0, 'c': 12}, HIDDEN), ({'x0_cols': 0, 'x_top4': None, 'c': 12}, HIDDEN),
                ({'x0_cols': 3, 'c': 12}, compact), ({'alpha_all': None, 'c': 12}, HIDDEN)]
    return out


def _block_forward_loss(narrow):
    cols = 'block_forward_loss: 1..4 coordinates, coordinates + extras <= 4 columns'
    head = 'block_forward_loss: head rows; with a target: seed, partials, 1 <= d <= 4'
    given = 'block_forward_loss: param given, but this graph / hidden size does not compute the coefficients in its layer-0 launch'
    bad, compact = 'block_forward: bad argument', 'block_forward: compact x0 needs 4 columns, >= 2 layers, hidden >= 8'
    out = [({'x_comp': None}, cols), ({'dim': 0}, cols), ({'dim': 5}, cols), ({'dim': 3}, cols), ({'dim': 4, 'uu_tensor': None}, cols),
           ({'x_top4': None}, head), ({'seed': None}, head), ({'loss_partials': None}, head), ({'d': 0}, head), ({'d': 5}, head),
           ({'g': None}, GRAPH), ({'g.n_nodes': 0}, GRAPH),
           ({'x_comp': None, 'g': None}, cols), ({'x_comp': None, 'x_top4': None}, cols), ({'d': 5, 'g': None}, head),   # x_comp and the loss: before the graph
           ({'c': 32}, given), ({'c': 12}, given), ({'g.wide_half_deg_t': 3}, given), ({'g.ell_t': None}, given), ({'g': None, 'c': 32}, GRAPH),
           ({'g.rowptr_t': None}, GRAPH), ({'g.rowptr_t': None, 'c': 32}, given),            # the rest of the graph: block_forward's check, after param
           ({'g.meta_t[1]': None}, META), ({'g.n_nodes': 1 << 24, 'c': 128, 'param': None}, GIB),
           ({'x_all': None}, bad), ({'a': None}, bad), ({'p0': None}, bad), ({'layer_params': None}, bad), ({'n_layers': 0}, bad),
           ({'n_layers': 1}, compact), ({'c': 4, 'param': None}, compact), ({'x_all': None, 'n_layers': 1}, bad),
           ({'dim': 3, 'f_tensor': None, 'x_all': None}, bad), ({'f_tensor': None, 'uu_tensor': None, 'dim': 4, 'x_all': None}, bad),
           ({'target': None, 'seed': None, 'loss_partials': None, 'd': 0, 'x_all': None}, bad), ({'alpha_all': None, 'x_all': None}, bad)]
    if narrow:
        nar = 'block_forward (narrow): compact x0, head rows, hidden 64 on a graph the wide forward takes (gadapt_narrow_route)'
        small = 'block_forward_loss (narrow): param given without the coefficient buffers'
        out += [({'c': 32, 'param': None}, nar), ({'g.ell_t': None, 'param': None}, nar), ({'g.wide_deg_t': 0, 'param': None}, nar),
                ({'g.n_nodes': 16128, 'a': None}, small), ({'g.n_nodes': 1024, 'p0': None}, small), ({'g.n_nodes': 1024, 'a': None, 'n_layers': 1}, small),
                ({'g.n_nodes': 1024, 'a': None, 'param': None}, bad)]            # (64 workgroups and more, or no param: block_forward's check)
    else:
        out += [({'c': 12, 'param': None}, HIDDEN), ({'c': 12, 'param': None, 'target': None}, HIDDEN)]
    return out


def _tail():
    bad, rows = 'step_tail: bad argument', 'step_tail: slab without row count / scratch'
    loss = 'step_tail: loss partials need a count, a destination and the slab launch they ride in'
    return _nulls(['param', 'grad', 'state', 'exp_avg', 'exp_avg_sq', 'a_out', 'p0_out'], bad) + [
        ({'c': 12}, bad), ({'slab': None, 'exp_avg': None, 'exp_avg_sq': None}, bad),
        ({'n_rows': 0}, rows), ({'scratch': None}, rows), ({'n_loss_partials': 0}, loss), ({'loss_out': None}, loss), ({'loss_count': 0}, loss),
        ({'slab': None}, loss), ({'param': None, 'n_rows': 0}, bad), ({'n_rows': 0, 'loss_out': None}, rows),
        ({'exp_avg': None, 'exp_avg_sq': None, 'state': None, 'a_out': None, 'n_rows': 0}, rows),       # gradient only: no state, no moments
        ({'a_out': None, 'p0_out': None, 'n_rows': 0}, rows), ({'loss_partials': None, 'n_loss_partials': 0, 'loss_out': None, 'n_rows': 0}, rows),
        ({'slab': None, 'n_rows': 0, 'scratch': None, 'param': None}, bad)]


def _tail_narrow():
    who = 'step_tail_narrow: '
    hid, slab, bad, loss = who + 'hidden 64 only (gadapt_narrow_route)', who + 'the packed slab, its row count and the scratch', who + 'bad argument', \
        who + 'loss partials need a count and a destination'
    return [({'c': 32}, hid), ({'c': 128}, hid), ({'slab': None}, slab), ({'n_rows': 0}, slab), ({'scratch': None}, slab)] + \
        _nulls(['param', 'grad', 'state', 'exp_avg', 'exp_avg_sq', 'a_out', 'p0_out'], bad) + [
        ({'n_loss_partials': 0}, loss), ({'loss_out': None}, loss), ({'loss_count': 0}, loss),
        ({'c': 32, 'slab': None}, hid), ({'slab': None, 'param': None}, slab), ({'param': None, 'loss_out': None}, bad),
        ({'exp_avg': None, 'exp_avg_sq': None, 'state': None, 'a_out': None, 'loss_out': None}, loss), ({'a_out': None, 'p0_out': None, 'loss_count': 0}, loss)]


def _block_backward():
    bad = 'block_backward: bad argument'
    compact = 'block_backward: compact x0 needs 4 columns, >= 2 layers, hidden >= 8, no d_x0'
    csr = 'block_backward: source CSR missing'
    req = ['x_all', 'alpha_all', 'g_top', 'a', 'p0', 'layer_params', 'g_ws', 'dxd_ws', 'edge_ws', 'slab']
    return _check_graph({'slab': None}) + _nulls(req, bad) + [
        ({'n_layers': 0}, bad), ({'x0_cols': 3}, compact), ({'n_layers': 1}, compact), ({'c': 4}, compact), ({'d_x0': P}, compact),
        ({'c': 12}, HIDDEN), ({'x0_cols': 0, 'c': 12}, HIDDEN), ({'x0_cols': 0, 'd_x0': P, 'c': 12}, HIDDEN),
        ({'g.tpos_s': None}, csr), ({'g.rowptr_s': None}, csr), ({'g.col_s': None}, csr),
        ({'g_top_cols': 5}, G_COLS), ({'g_top_cols': -1}, G_COLS),
        ({'slab': None, 'x0_cols': 3}, bad), ({'x0_cols': 3, 'c': 12}, compact),
        ({'c': 12, 'g.tpos_s': None}, HIDDEN),                                     # the slab is sized before the layer loop looks for the source CSR
        ({'g.tpos_s': None, 'g_top_cols': 5}, csr),
        ({'x0_cols': 0, 'n_layers': 1, 'g.rowptr_s': None, 'g.col_s': None, 'g_top_cols': 5}, G_COLS),   # nothing to pass on: no source CSR needed
        ({'x0_cols': 0, 'n_layers': 1, 'g.tpos_s': None, 'g_top_cols': 5}, csr),
        ({'d_layer_params': None, 'g_top_cols': 5}, G_COLS)]


def _block_backward_narrow(packed):
    bad = 'block_backward (narrow): bad argument'
    nar = 'block_backward (narrow): compact x0, compact top gradient, no d_x0, fixed steps and temperature, hidden 64 on a graph the wide forward takes'
    one = 'block_backward (narrow, packed slab): one shared conv (a_stride = p0_stride = 0)'
    tgt = 'narrow target pass: hidden 64, ELL graph, 0..4 g columns'
    req = ['x_all', 'alpha_all', 'g_top', 'a', 'p0', 'layer_params', 'g_ws', 'dxd_ws', 'edge_ws', 'slab']
    out = _check_graph({'slab': None}) + _nulls(req, bad) + [
        ({'n_layers': 1}, bad), ({'n_layers': 0}, bad), ({'x0_cols': 0}, nar), ({'g_top_cols': 0}, nar), ({'g_top_cols': 5}, nar), ({'d_x0': P}, nar),
        ({'d_layer_params': P}, nar), ({'c': 32}, nar), ({'c': 128}, nar), ({'g.ell_t': None}, nar), ({'g.wide_deg_t': 0}, nar),
        ({'slab': None, 'x0_cols': 0}, bad), ({'g.tpos_s': None}, tgt), ({'g.tpos_s': None, 'g.ell_s': None}, tgt),
        ({'g.tpos_s': None, 'g.n_edges': 16384 * 40}, tgt), ({'c': 32, 'g.tpos_s': None}, nar)]
    if packed:
        out += [({'a_stride': 4096}, one), ({'p0_stride': 64}, one), ({'a_stride': 4096, 'c': 32}, nar), ({'a_stride': 4096, 'g.tpos_s': None}, one)]
    else:
        out += [({'a_stride': 4096, 'p0_stride': 64, 'g.tpos_s': None}, tgt)]
    return out


def _reduce():
    bad = 'slab_reduce: bad argument'
    return _nulls(['slab', 'scratch', 'd_a', 'd_p0'], bad) + [({'n_rows': 0}, bad), ({'c': 12}, bad)]


def _reduce_coeffs():
    bad, lp = 'slab_reduce_coeffs_backward: bad argument', 'slab_reduce_coeffs_backward: layer-parameter partials without a destination'
    return _nulls(['slab', 'scratch', 'wq', 'bq', 'wk', 'd_wq', 'd_bq', 'd_wk', 'd_bk'], bad) + [
        ({'n_rows': 0}, bad), ({'c': 12}, bad), ({'n_layers': 0}, lp), ({'d_layer_params': None}, lp), ({'slab': None, 'n_layers': 0}, bad)]


ROWS = 'slab_rows: bad node count'
REGISTER = 'narrow_block_register: a graph with its ELL copy, halo 0 (forget), 32 or 64'
TABLE = {
    'gadapt_layer_forward': _layer_forward(),
    'gadapt_layer_backward': _layer_backward(),
    'gadapt_block_forward': _block_forward(False),
    'gadapt_block_forward_narrow': _block_forward(True),
    'gadapt_block_forward_loss': _block_forward_loss(False),
    'gadapt_block_forward_loss_narrow': _block_forward_loss(True),
    'gadapt_block_backward': _block_backward(),
    'gadapt_block_backward_narrow': _block_backward_narrow(False),
    'gadapt_block_backward_narrow_packed': _block_backward_narrow(True),
    'gadapt_step_tail': _tail(),
    'gadapt_step_tail_narrow': _tail_narrow(),
    'gadapt_slab_reduce': _reduce(),
    'gadapt_slab_reduce_coeffs_backward': _reduce_coeffs(),
    'gadapt_backward_slab_rows': [({'n_nodes': 0}, ROWS), ({'n_nodes': -5}, ROWS), ({'c': 12}, HIDDEN), ({'n_nodes': 0, 'c': 12}, ROWS)],
    'gadapt_backward_slab_floats': [({'n_nodes': 0}, ROWS), ({'c': 12}, HIDDEN), ({'n_nodes': 0, 'c': 12}, ROWS)],
    'gadapt_narrow_slab_floats': [({'n_nodes': 0}, ROWS), ({'n_nodes': -1}, ROWS)],
    'gadapt_narrow_block_register': [({'g': None}, REGISTER), ({'g.rowptr_t': None}, REGISTER), ({'g.ell_t': None}, REGISTER), ({'g.n_nodes': 0}, REGISTER),
                                     ({'halo': 16}, REGISTER), ({'halo': -32}, REGISTER), ({'halo': 128}, REGISTER)],
}
CASES = [(entry, breaks, text) for entry, rows in TABLE.items() for breaks, text in rows]


def _id(entry, breaks):
    return f"{entry[7:]}-" + '+'.join(k if (v is None or v == P) else f'{k}={v}' for k, v in breaks.items())


def test_the_entry_points_are_covered():
    assert len(TABLE) == 17 and set(TABLE) <= set(nv.PROTOTYPES)
    assert len({_id(e, b) for e, b, _ in CASES}) == len(CASES)
    assert nv.lib().gadapt_abi_version() == 9
    valid = _graph({})                                                             # the unbroken graph is what the cases say it is
    assert nv.lib().gadapt_narrow_route(C.byref(valid), 64) == 1 and nv.lib().gadapt_forward_computes_coeffs(C.byref(valid), 64) == 1
    assert nv.lib().gadapt_narrow_route(C.byref(valid), 32) == 0 and nv.lib().gadapt_narrow_block_halo(C.byref(valid), 64) == 0


@pytest.mark.parametrize('entry,breaks,text', CASES, ids=[_id(e, b) for e, b, _ in CASES])
def test_refusal(entry, breaks, text):
    got, msg = _call(entry, breaks)
    assert (got, msg[:len(text)]) == (BAD, text), (entry, breaks, got, msg)
