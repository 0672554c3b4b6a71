"""The Burgers evaluation tables on the MI355X (g_adaptivity_amd.evaluation_burgers) against gradient_meshpoints_1D (the
one-step table: the same kernel, bit for bit) and against the CPU restatement of the rollout
(tests/burgers_eval_restatement.py) on a small config.

Rollout bound (the project's rule, floor as tests/test_gpu_fem1d.py's forwards): rel(gpu, fp64) <= max(1e-5, 1.5 * noise),
noise = rel(fp32 restatement, fp64 restatement) of the same sample.  Measured figures: docs/measurements.md."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import burgers_eval_restatement as BE  # noqa: E402

from g_adaptivity_amd import (GNN, MeshData, MeshDataset, calculate_error_reduction, collate, evaluate_model_fine_burgers,  # noqa: E402
                              evaluate_model_fine_burgers_time_step, gradient_meshpoints_1D, hot_path_opt)
from g_adaptivity_amd import evaluation_burgers as eb  # noqa: E402
from g_adaptivity_amd.inference import GraphedForward  # noqa: E402
from g_adaptivity_amd.mmpde5 import CAP, CONVERGED  # noqa: E402
from g_adaptivity_amd.spline import SPLINE_NOT_INCREASING, SPLINE_OK  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_dispatch]

N = 11
OPT = {'mesh_dims': [N], 'num_fine_mesh_points': 20, 'eval_quad_points': 41, 'load_quad_points': 41, 'tau': 1 / 20.0, 'nu': 1e-3,
       'gauss_amplitude': 0.25, 'mon_reg': 0.1, 'mon_power': 0.2, 'num_time_steps': 1, 'num_eval_time_steps': 4,
       'grad_type': 'burgers_timestep_loss_direct_mse'}
FIXED = dict(tol=0, max_steps=200)
FLOOR = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'burgers_eval', 'rollout_converged.npz')


def make_ds():
    return MeshDataset([N], 3, seed=2, num_gauss=1, burgers=True, target='mmpde5', target_params={'mon_power': 0.2, 'mon_reg': 0.1})


def make_model(ds, dev, seed=0):
    torch.manual_seed(seed)
    return GNN(ds, hot_path_opt(mesh_dims=[N], conv_type='GRAND', hidden_dim=8, gnn_inc_feat_f=False, device=str(dev))).to(dev).eval()


def col(df, name):
    return np.asarray(df[name], dtype=np.float64)


def rel(a, b):
    return abs(a - b) / abs(b)


def run(model, ds, dev, batch_size=1, mmpde5=FIXED, expect_warnings=None):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        out = evaluate_model_fine_burgers_time_step(model, ds, dict(OPT, device=str(dev)), batch_size=batch_size, mmpde5=mmpde5)
    torch.cuda.synchronize()
    got = [w for w in rec if issubclass(w.category, RuntimeWarning)]
    if expect_warnings is not None:
        assert len(got) == expect_warnings, [str(w.message) for w in got]
    return out


@pytest.fixture(scope='module')
def base(gpu_device):
    """The fixed-step rollout at batch_size=1, computed once: (dataset, model, df, df_time)."""
    ds = make_ds()
    model = make_model(ds, gpu_device)
    df, dt = run(model, ds, gpu_device, expect_warnings=1)          # CAP on every relaxation: ONE warning for the call
    return ds, model, df, dt


def test_one_step_table(gpu_device):
    ds = make_ds()
    model = make_model(ds, gpu_device)
    opt = dict(OPT, device=str(gpu_device))
    df, dt = evaluate_model_fine_burgers(model, ds, opt, batch_size=1)
    assert list(df.keys()) == ['L2_grid', 'L2_MA', 'L2_MLmodel', 'L2_reduction_MA', 'L2_reduction_MLmodel']
    assert list(dt.keys()) == ['MA_time', 'MLmodel_time']
    for i, s in enumerate(ds.samples):
        d = collate([s]).to(gpu_device)
        with torch.no_grad():
            x_ml = model(d).reshape(-1).clone()
        for name, mesh in (('L2_grid', s.x_comp.to(gpu_device)), ('L2_MA', s.x_phys.to(gpu_device)), ('L2_MLmodel', x_ml)):
            loss, _ = gradient_meshpoints_1D(opt, MeshData(pde_params=s.pde_params), mesh.reshape(-1))
            print(f"one-step {name}[{i}] = {col(df, name)[i]:.9e}, gradient_meshpoints_1D {float(loss):.9e}")
            assert col(df, name)[i] == float(loss)                   # the same kernel: bit for bit
        g = col(df, 'L2_grid')[i]
        assert col(df, 'L2_reduction_MA')[i] == calculate_error_reduction(g, col(df, 'L2_MA')[i])
        assert col(df, 'L2_reduction_MLmodel')[i] == calculate_error_reduction(g, col(df, 'L2_MLmodel')[i])
    assert (col(dt, 'MA_time') > 0).all() and (col(dt, 'MLmodel_time') > 0).all()
    # stored on the samples: another checkpoint pays for the model's meshes only
    calls = []
    keep = eb.burgers_1d
    eb.burgers_1d = lambda x, counts, *a, **k: (calls.append(len(counts)), keep(x, counts, *a, **k))[1]
    try:
        df2, _ = evaluate_model_fine_burgers(make_model(ds, gpu_device, seed=1), ds, opt, batch_size=3)
    finally:
        eb.burgers_1d = keep
    assert calls == [3]
    assert np.array_equal(col(df2, 'L2_grid'), col(df, 'L2_grid')) and np.array_equal(col(df2, 'L2_MA'), col(df, 'L2_MA'))


def _model_fn(model, sample, dev):
    def fn(u, x):
        d = collate([sample]).to(dev)
        if u is not None:
            d.uu_tensor = u.float().to(dev).reshape(d.uu_tensor.shape)
            d.x_phys = x.float().to(dev).reshape(d.x_phys.shape)
        with torch.no_grad():
            return model(d).reshape(-1).cpu().clone()
    return fn


def test_rollout_fixed_steps_against_restatement(gpu_device, base):
    ds, model, df, dt = base
    assert list(df.keys()) == ['L2_grid', 'L2_MA', 'L2_MLmodel', 'L2_reduction_MA', 'L2_reduction_MLmodel']
    assert list(dt.keys()) == ['MA_time', 'MA_mesh_time', 'MLmodel_time', 'ML_mesh_time']
    for i, s in enumerate(ds.samples):
        fn = _model_fn(model, s, gpu_device)
        r64 = BE.rollout(s.pde_params, s.x_phys, OPT, N, torch.float64, FIXED, fn)
        r32 = BE.rollout(s.pde_params, s.x_phys, OPT, N, torch.float32, FIXED, fn)
        assert r64['steps'] == [200] * 3
        e = s.eval_rollout_burgers
        assert e['mmpde5_status'].tolist() == [CAP] * 3 and e['mmpde5_steps'].tolist() == [200] * 3
        for name in ('L2_grid', 'L2_MA', 'L2_MLmodel'):
            got, err, noise = col(df, name)[i], rel(col(df, name)[i], r64[name]), rel(r32[name], r64[name])
            print(f"rollout fixed {name}[{i}]: gpu {got:.6e} fp64 {r64[name]:.6e} err {err:.3e} noise {noise:.3e}")
            assert err <= max(FLOOR, 1.5 * noise), (name, i, err, noise)
        g = col(df, 'L2_grid')[i]
        assert col(df, 'L2_reduction_MA')[i] == calculate_error_reduction(g, col(df, 'L2_MA')[i])
        assert col(df, 'L2_reduction_MLmodel')[i] == calculate_error_reduction(g, col(df, 'L2_MLmodel')[i])
    t = {k: col(dt, k) for k in dt.keys()}
    assert (t['MA_time'] >= t['MA_mesh_time']).all() and (t['MA_mesh_time'] > 0).all()
    assert (t['MLmodel_time'] >= t['ML_mesh_time']).all() and (t['ML_mesh_time'] > 0).all()


def test_rollout_to_convergence_against_fixture(gpu_device):
    g = np.load(GOLDEN)
    ds = MeshDataset([N], 1, seed=5, num_gauss=1, burgers=True)
    s = ds.samples[0]
    assert np.array_equal(np.asarray(s.pde_params['centers'][0], np.float32), g['center'])
    assert np.array_equal(np.asarray(s.pde_params['scales'][0], np.float32), g['scale'])
    s.x_phys = torch.from_numpy(g['x_ma0'])
    model = make_model(ds, gpu_device)
    df, _ = run(model, ds, gpu_device, mmpde5=None, expect_warnings=0)
    e = s.eval_rollout_burgers
    assert e['mmpde5_status'].tolist() == [CONVERGED] * 3
    # the stopping step follows the rounding of the last increments.  The spread of this case: the largest difference between
    # the fixture's fp32 and fp64 restatements over its three relaxations (6, 17, 13 -> 17 steps of ~1000-1800).  Measured on
    # the MI355X: 0, 11, 16 steps from the fp64 counts (docs/measurements.md; relaxation by relaxation the third, 16 against
    # 13, would not fit: the GPU's fp32 arithmetic is not the fp32 restatement's either, 3 steps apart there).
    spread = int(np.abs(g['steps_f32'] - g['steps_f64']).max())
    print(f"rollout converged: steps gpu {e['mmpde5_steps'].tolist()} fp64 {g['steps_f64'].tolist()} fp32 {g['steps_f32'].tolist()}")
    assert (np.abs(e['mmpde5_steps'].numpy() - g['steps_f64']) <= spread).all()
    for name in ('L2_grid', 'L2_MA'):
        r64, r32 = float(g[name + '_f64']), float(g[name + '_f32'])
        err, noise = rel(col(df, name)[0], r64), rel(r32, r64)
        print(f"rollout converged {name}: gpu {col(df, name)[0]:.6e} fp64 {r64:.6e} err {err:.3e} noise {noise:.3e}")
        assert err <= max(FLOOR, 1.5 * noise), (name, err, noise)


def test_a_row_does_not_depend_on_its_batch(gpu_device, base):
    _, _, df1, _ = base
    ds = make_ds()
    df3, _ = run(make_model(ds, gpu_device), ds, gpu_device, batch_size=3, expect_warnings=1)
    assert np.array_equal(col(df1, 'L2_grid'), col(df3, 'L2_grid')) and np.array_equal(col(df1, 'L2_MA'), col(df3, 'L2_MA'))
    print("rollout batch 1 vs 3 L2_MLmodel:", col(df1, 'L2_MLmodel'), col(df3, 'L2_MLmodel'))
    # one model under two batch sizes: the relative tolerance of tests/test_gpu_callers.py
    assert np.allclose(col(df1, 'L2_MLmodel'), col(df3, 'L2_MLmodel'), rtol=1e-5, atol=0)


def test_second_checkpoint_reuses_the_reference_rollouts(gpu_device, base, monkeypatch):
    ds, _, df, dt = base
    calls = {'burgers': [], 'mmpde5': 0}
    keep_b, keep_m = eb.burgers_1d, eb.mmpde5_batch
    monkeypatch.setattr(eb, 'burgers_1d', lambda x, counts, *a, **k: (calls['burgers'].append(len(counts)), keep_b(x, counts, *a, **k))[1])
    monkeypatch.setattr(eb, 'mmpde5_batch', lambda *a, **k: (calls.__setitem__('mmpde5', calls['mmpde5'] + 1), keep_m(*a, **k))[1])
    df2, dt2 = run(make_model(ds, gpu_device, seed=1), ds, gpu_device, batch_size=3, expect_warnings=0)
    assert calls['mmpde5'] == 0 and calls['burgers'] == [3] * 3     # the model's meshes only: one call per outer step
    for name in ('L2_grid', 'L2_MA'):
        assert np.array_equal(col(df2, name), col(df, name))
    assert np.array_equal(col(dt2, 'MA_time'), col(dt, 'MA_time'))
    assert not np.array_equal(col(df2, 'L2_MLmodel'), col(df, 'L2_MLmodel'))


class Tangler:
    """The model, with two interior nodes of one sample swapped from its second call on."""

    def __init__(self, model, which):
        self.model, self.which, self.calls = model, which, 0

    def __call__(self, data):
        x = self.model(data).clone()
        self.calls += 1
        if self.which is not None and self.calls >= 2:
            v = x.view(-1, N)
            v[self.which, 4], v[self.which, 5] = v[self.which, 5].clone(), v[self.which, 4].clone()
        return x


def test_tangled_mesh_gives_a_nan_row_and_one_warning(gpu_device, base):
    ds, model, _, _ = base
    clean, _ = run(Tangler(model, None), ds, gpu_device, batch_size=3, expect_warnings=0)
    df, _ = run(Tangler(model, 1), ds, gpu_device, batch_size=3, expect_warnings=1)
    torch.cuda.synchronize()
    assert np.isnan(col(df, 'L2_MLmodel')[1]) and np.isnan(col(df, 'L2_reduction_MLmodel')[1])
    assert [s.eval_rollout_burgers['ML_status'] for s in ds.samples] == [SPLINE_OK, SPLINE_NOT_INCREASING, SPLINE_OK]
    for i in (0, 2):
        assert col(df, 'L2_MLmodel')[i] == col(clean, 'L2_MLmodel')[i]
    assert np.array_equal(col(df, 'L2_grid'), col(clean, 'L2_grid')) and np.array_equal(col(df, 'L2_MA'), col(clean, 'L2_MA'))


def test_graphed_forward_gives_the_same_tables(gpu_device, base):
    ds, model, df, _ = base
    graphed = GraphedForward(model, collate([ds.samples[0]]).to(gpu_device))
    df2, _ = run(graphed, ds, gpu_device, batch_size=1, expect_warnings=0)
    for name in df.keys():
        assert np.array_equal(col(df2, name), col(df, name)), name
    one, _ = evaluate_model_fine_burgers(model, ds, dict(OPT, device=str(gpu_device)))
    two, _ = evaluate_model_fine_burgers(graphed, ds, dict(OPT, device=str(gpu_device)))
    for name in one.keys():
        assert np.array_equal(col(one, name), col(two, name)), name
