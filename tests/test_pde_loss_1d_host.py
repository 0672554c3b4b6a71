"""1-D pde_loss, the host side: the dataset fields, the opt-in key, the refusals that stay, the fused tail's two symbols of
libgadapt_fem.so (header, prototypes, LDS formula, refusals before any launch) and `fem1d.Pde1dBatch`'s Gaussian staging.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from g_adaptivity_amd import GNN, MeshDataset, collate, hot_path_opt
from g_adaptivity_amd import _native_fem as nf
from g_adaptivity_amd import fem1d
from g_adaptivity_amd.functional import l1_loss, mse_loss
from g_adaptivity_amd.optim import FlatAdam
from g_adaptivity_amd.training import GraphedTrainStep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'gadapt_fem.h')).read()
ENTRY, BYTES = 'gadapt_fem_poisson1d_loss', 'gadapt_fem_poisson1d_loss_lds_bytes'
BUDGET, CAP = 65536, 1024

_buf = (C.c_double * 64)()                                    # dummy non-null HOST address, 8-byte aligned: never dereferenced
P = C.addressof(_buf)
VALID = {'n_meshes': 1, 'max_nodes': 8, 'k_load': 5, 'k_stiff': 3, 'n_pts': 9, 'loss_kind': nf.FEM1D_LOSS_L1, 'stream': None}


# ------------------------------------------------------------------------------------------------ the dataset fields
def _gauss64(q, params):
    u = torch.zeros_like(q)
    for c, s in zip(params['centers'], params['scales']):
        u += torch.exp(-((q - float(c[0])) / float(s[0])) ** 2)
    return u


@pytest.mark.parametrize('P_', [101, 33])
def test_1d_dataset_fields(P_):
    plain = MeshDataset([15], 3, seed=2)
    asked = MeshDataset([15], 3, seed=2, pde_loss_fields=True, eval_quad_points=P_)
    assert not hasattr(plain.samples[0], 'u_true_fine_tensor') and not hasattr(plain, 'mapping_tensor_fine')
    assert torch.equal(asked.mapping_tensor_fine, torch.arange(P_))
    q = torch.linspace(0, 1, P_).double()
    for a, b in zip(asked.samples, plain.samples):
        u = a.u_true_fine_tensor
        assert u.shape == (P_,) and u.dtype == torch.float32
        assert torch.equal(u, _gauss64(q, a.pde_params).float())              # computed in fp64, stored as fp32
        assert torch.equal(a.x_phys, b.x_phys) and torch.equal(a.uu_tensor, b.uu_tensor)     # the samples are unchanged otherwise
    batch = collate(asked.samples)
    assert batch.u_true_fine_tensor.shape == (3 * P_,)
    assert torch.equal(batch.u_true_fine_tensor, torch.cat([s.u_true_fine_tensor for s in asked.samples]))


# ------------------------------------------------------------------------------------------------ the key
def test_hot_path_opt_lists_the_key_and_the_split_tail():
    o = hot_path_opt()
    assert o['pde_loss_1d'] is False and o['fem1d_tail'] == 'split'
    assert hot_path_opt(pde_loss_1d=True, fem1d_tail='fused')['fem1d_tail'] == 'fused'


def _opt(**kw):
    return hot_path_opt(mesh_dims=[15], hidden_dim=8, num_layers=2, loss_type='pde_loss', **kw)


def test_model_is_built_with_the_key_and_refused_without_it():
    ds = MeshDataset([15], 2, pde_loss_fields=True)
    with pytest.raises(NotImplementedError, match='1-D'):
        GNN(ds, _opt())
    with pytest.raises(NotImplementedError, match='1-D'):
        GNN(ds, _opt(pde_loss_1d=False))
    model = GNN(ds, _opt(pde_loss_1d=True))
    assert model.dim == 1 and model.quad_points.shape == (101,)
    with pytest.raises(NotImplementedError, match='2-D Poisson only'):        # Burgers stays out of scope, key or not
        GNN(ds, _opt(pde_loss_1d=True, pde_type='Burgers'))
    with pytest.raises(ValueError, match='fem1d_tail'):
        GNN(ds, _opt(pde_loss_1d=True, fem1d_tail='both'))


def test_tail_check_follows_the_key():
    from g_adaptivity_amd import fem

    class Model:
        dim = 1
    Model.opt = _opt()
    with pytest.raises(NotImplementedError, match='1-D'):
        fem._check_tail(Model())
    Model.opt = _opt(pde_loss_1d=True)
    assert fem._check_tail(Model()) == ('lds', 'lane')


def test_step_refusals_at_construction():
    ds = MeshDataset([15], 2, pde_loss_fields=True)
    model = GNN(ds, _opt(pde_loss_1d=True, fem1d_tail='fused')).train()
    optim = FlatAdam(model.parameters(), capturable=True)
    with pytest.raises(ValueError, match="'fused'.*l1_loss or mse_loss"):      # a foreign loss_fn with the fused tail
        GraphedTrainStep(model, optim, loss_fn=torch.nn.functional.l1_loss)
    without = GNN(MeshDataset([15], 2), hot_path_opt(mesh_dims=[15], hidden_dim=8, num_layers=2)).train()
    without.opt['loss_type'] = 'pde_loss'                                      # (the constructor refuses such a model itself)
    with pytest.raises(NotImplementedError, match='1-D'):
        GraphedTrainStep(without, FlatAdam(without.parameters(), capturable=True))
    model.opt['fem1d_tail'] = 'both'
    with pytest.raises(ValueError, match='fem1d_tail'):
        GraphedTrainStep(model, optim, loss_fn=l1_loss)
    assert mse_loss is not l1_loss


# ------------------------------------------------------------------------------------------------ the two symbols
def _decl(entry):
    return re.search(r'\b' + entry + r'\s*\(([^;]*)\);', HEADER).group(1)


def _names(entry):
    return [re.search(r'(\w+)\s*$', p).group(1) for p in _decl(entry).split(',')]


def test_header_names_equal_prototypes_and_abi_is_4():
    declared = set(re.findall(r'\b(gadapt_fem\w*)\s*\(', HEADER))
    assert declared == set(nf.PROTOTYPES) and {ENTRY, BYTES} <= declared
    lib = nf.lib()
    assert hasattr(lib, ENTRY) and hasattr(lib, BYTES)
    assert len(_names(ENTRY)) == len(nf.PROTOTYPES[ENTRY][1]) == 20 and len(_names(BYTES)) == len(nf.PROTOTYPES[BYTES][1]) == 2
    assert nf.PROTOTYPES[BYTES][0] is C.c_int64 and nf.PROTOTYPES[ENTRY][0] is C.c_int
    # the Poisson forward's leading arguments, then the target and the loss
    assert _names(ENTRY)[:10] == _names('gadapt_fem1d_poisson_forward')[:10]
    assert _names(ENTRY)[10:] == ['target', 'loss_kind', 'coeffs', 'sol', 'gx', 'flags', 'partials', 'loss', 'ticket', 'stream']
    assert lib.gadapt_fem_abi_version() == 4 and nf.ABI_VERSION == 4 and re.search(r'#define GADAPT_FEM_ABI 4\b', HEADER)
    assert re.search(r'#define GADAPT_FEM1D_LOSS_L1\s+0\b', HEADER) and re.search(r'#define GADAPT_FEM1D_LOSS_MSE\s+1\b', HEADER)
    assert (nf.FEM1D_LOSS_L1, nf.FEM1D_LOSS_MSE) == (0, 1)


@pytest.mark.parametrize('n,p', [(3, 2), (15, 101), (65, 64), (1017, 101), (1018, 101), (1024, 1), (1024, 0)])
def test_lds_bytes_is_the_layout_formula(n, p):
    lib = nf.lib()
    poisson = 64 * n                                                           # 12 fp32 rows and two fp64 rows per node
    assert lib.gadapt_fem_poisson1d_loss_lds_bytes(n, p) == poisson + 4 * p
    assert lib.gadapt_fem1d_lds_bytes(n, 0) == max(poisson, 60 * n)             # the Poisson layout is what the seed row follows


def _call(breaks):
    assert breaks, "an unbroken argument list would be launched on host addresses"
    names = _names(ENTRY)
    assert set(breaks) <= set(names)
    lib = nf.lib()
    rc = getattr(lib, ENTRY)(*[breaks[n] if n in breaks else VALID.get(n, P) for n in names])
    return rc, lib.gadapt_fem_last_error().decode()


def test_node_cap_with_the_seed_row():
    """1017 nodes at 101 points pass the LDS check and 1018 do not; every call here carries a fault, so nothing is launched."""
    lds = lambda b: f'{ENTRY}: needs {b} B of LDS, the budget is {BUDGET} B'
    assert _call({'max_nodes': 1018, 'n_pts': 101}) == (-5, lds(64 * 1018 + 404))                 # GADAPT_FEM_E_LDS
    assert _call({'max_nodes': 1024, 'n_pts': 1}) == (-5, lds(65540))
    assert _call({'max_nodes': 1017, 'n_pts': 113}) == (-5, lds(64 * 1017 + 452))                 # one point past what 1017 nodes leave
    # 1017 at 101 points is within the budget: with a fault of its own, that fault is what is refused, and it comes before the budget
    own = f'{ENTRY}: null pointer, no evaluation points or unknown loss_kind'
    assert _call({'max_nodes': 1017, 'n_pts': 101, 'gx': None}) == (-1, own)
    assert _call({'max_nodes': 1018, 'n_pts': 101, 'gx': None}) == (-1, own)
    assert nf.lib().gadapt_fem_poisson1d_loss_lds_bytes(1017, 101) <= BUDGET < nf.lib().gadapt_fem_poisson1d_loss_lds_bytes(1018, 101)


def test_entry_point_refuses_before_any_launch():
    batch = f'{ENTRY}: bad batch, pointers or point count'
    own = f'{ENTRY}: null pointer, no evaluation points or unknown loss_kind'
    quad = f'{ENTRY}: need load_quad_points >= 2 and stiff_quad_points >= 1'
    nodes = lambda n: f'{ENTRY}: {n} nodes per mesh; 3..{CAP} supported (one lane per node, state in LDS)'
    for k, v in (('n_meshes', 0), ('n_meshes', -2), ('node_off', None), ('x', None), ('pts', None), ('n_pts', -1)):
        assert _call({k: v}) == (-1, batch), (k, v)
    assert _call({'max_nodes': 2}) == (-1, nodes(2))
    assert _call({'max_nodes': CAP + 1}) == (-5, nodes(CAP + 1))
    assert _call({'k_load': 1}) == (-1, quad) and _call({'k_stiff': 0}) == (-1, quad)
    for k in ('gptr', 'gpar', 'target', 'coeffs', 'sol', 'gx', 'flags', 'partials', 'loss', 'ticket'):
        assert _call({k: None}) == (-1, own), k
    assert _call({'loss_kind': 2}) == (-1, own) and _call({'loss_kind': -1}) == (-1, own)
    assert _call({'n_pts': 0, 'pts': None}) == (-1, own)                       # no evaluation points: nothing to take a loss over
    # the order: batch, node range, quadrature, its own, the budget
    assert _call({'x': None, 'max_nodes': 2}) == (-1, batch)
    assert _call({'k_load': 1, 'max_nodes': 2}) == (-1, nodes(2))
    assert _call({'gx': None, 'k_stiff': 0}) == (-1, quad)
    assert _call({'gx': None, 'max_nodes': 1024}) == (-1, own)


# ------------------------------------------------------------------------------------------------ Pde1dBatch
def _gauss(k, seed):
    rng = np.random.default_rng(seed)
    return {'centers': [rng.uniform(0, 1, 1).astype('f') for _ in range(k)], 'scales': [rng.uniform(0.1, 0.5, 1).astype('f') for _ in range(k)]}


def test_pde1d_batch_packs_what_a_call_packs():
    pts = torch.linspace(0, 1, 33)
    pb = fem1d.Pde1dBatch([3, 15, 65], pts, cap=3 * 8)
    assert (pb.n_meshes, pb.n_nodes, pb.nmax, pb.cap, pb.counts) == (3, 83, 65, 24, [3, 15, 65])
    assert pb.node_off.tolist() == [0, 3, 18, 83] and pb.node_off.dtype == torch.int32
    assert torch.equal(pb.pts, pts) and (pb.k_load, pb.k_stiff) == (101, 3)
    assert pb.gptr.shape == (4,) and pb.gptr.dtype == torch.int32 and pb.gpar.shape == (24, 2) and pb.gpar.dtype == torch.float32
    assert pb.host_gptr.shape == pb.gptr.shape and pb.host_gpar.shape == pb.gpar.shape
    assert pb.interior.tolist() == [1] + list(range(4, 17)) + list(range(19, 82))
    assert pb.watch is False and pb.fused is None
    ptr0, par0 = pb.gptr.data_ptr(), pb.gpar.data_ptr()
    for counts, seed in (((1, 3, 2), 0), ((3, 1, 1), 1), ((2, 2, 2), 2)):        # mixed counts; a second batch with fewer rows
        params = [_gauss(k, 10 * seed + i) for i, k in enumerate(counts)]
        pb.set_params(params)
        ptr, rows = fem1d._gaussian_rows(params)
        g = rows.shape[0]
        want = np.array([[p['centers'][j][0], p['scales'][j][0]] for p in params for j in range(len(p['centers']))], 'f')
        assert np.array_equal(rows, want) and ptr.tolist() == np.cumsum((0,) + counts).tolist()
        assert torch.equal(pb.host_gptr, torch.from_numpy(ptr)) and torch.equal(pb.host_gpar[:g], torch.from_numpy(rows))
        assert torch.equal(pb.gptr, pb.host_gptr) and torch.equal(pb.gpar[:g], pb.host_gpar[:g])
        assert (pb.gptr.data_ptr(), pb.gpar.data_ptr()) == (ptr0, par0)          # the same tensors
        assert pb.head(torch.zeros(83))[:3] == (3, 65, pb.node_off.data_ptr()) and pb.head(torch.zeros(83))[4:] == (ptr0, par0)
    assert pb.gptr.tolist() == [0, 2, 4, 6]


def test_pde1d_batch_refusals():
    pts = torch.linspace(0, 1, 9)
    pb = fem1d.Pde1dBatch([5, 5], pts, cap=4)
    pb.set_params([_gauss(2, 0), _gauss(2, 1)])
    before = (pb.host_gptr.clone(), pb.host_gpar.clone(), pb.gpar.clone())
    with pytest.raises(ValueError, match=r'\b5 Gaussians.*room for 4\b'):
        pb.set_params([_gauss(2, 2), _gauss(3, 3)])
    assert all(torch.equal(a, b) for a, b in zip(before, (pb.host_gptr, pb.host_gpar, pb.gpar)))   # raised before any copy
    with pytest.raises(ValueError, match='3 meshes'):
        pb.set_params([_gauss(1, 0)] * 3)
    with pytest.raises(ValueError, match='at least 3 nodes'):
        fem1d.Pde1dBatch([5, 2], pts, cap=4)
    with pytest.raises(NotImplementedError, match='1025 nodes'):
        fem1d.Pde1dBatch([1025], pts, cap=4)
    with pytest.raises(ValueError, match='room for 0'):
        fem1d.Pde1dBatch([5], pts, cap=0)
    with pytest.raises(ValueError, match='x_phys'):
        pb.solve(torch.zeros(9))
    with pytest.raises(fem1d.NativeError, match='no CPU fallback'):            # nothing but the GPU solves
        pb.solve(torch.zeros(10))


def test_pde1d_batch_from_data_reads_the_model():
    ds = MeshDataset([15], 3, seed=1, pde_loss_fields=True, eval_quad_points=33, num_gauss=3)
    model = GNN(ds, _opt(pde_loss_1d=True, eval_quad_points=33, load_quad_points=41))
    batch = collate(ds.samples)
    pb = fem1d.Pde1dBatch.from_data(model, batch, max_gauss=4)
    assert (pb.B, pb.counts, pb.cap, pb.k_load, pb.k_stiff) == (3, [15, 15, 15], 12, 41, 3)
    assert torch.equal(pb.pts, torch.linspace(0, 1, 33)) and pb.gptr.tolist() == [0, 3, 6, 9]
    with pytest.raises(ValueError, match='9 Gaussians in the batch, room for 6'):
        fem1d.Pde1dBatch.from_data(model, batch, max_gauss=2)


def test_fused_tail_refuses_on_the_host():
    params = [_gauss(1, 0)]
    with pytest.raises(fem1d.NativeError, match='no CPU fallback'):
        fem1d.poisson_loss_1d(torch.linspace(0, 1, 5), [5], params, torch.zeros(101), {})
    with pytest.raises(ValueError, match=r'x must be \[N\]'):
        fem1d.poisson_loss_1d(torch.zeros(5, 1), [5], params, torch.zeros(101), {})
    assert set(fem1d.LOSS_KINDS) == {'l1', 'mse'}
