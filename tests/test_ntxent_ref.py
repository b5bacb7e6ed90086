"""tests/ntxent_ref.py against torch's fp64 autograd, the properties of the seeded inputs that tests/test_gpu_ntxent.py relies
on, and the host-side wiring of the NT-Xent feature (refusals before any device is touched, factories, state-dict keys)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ntxent_ref as nr                  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('T', [0.07, 0.5])
@pytest.mark.parametrize('b', [1, 2, 5, 33])
def test_spec_matches_torch_autograd(b, T):
    rng = np.random.RandomState(b)
    z = rng.randn(2 * b, 16) * rng.uniform(0.5, 2.0, size=(2 * b, 1))           # not unit-norm
    zt = torch.from_numpy(z).requires_grad_(True)
    loss = nr.torch_chain(zt, 1.0 / T)
    loss.backward()
    ref = nr.ntxent(z, 1.0 / T)
    assert abs(ref['loss'] - float(loss.detach())) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    g = zt.grad.numpy()
    assert np.abs(ref['dz'] - g).max() <= 1e-12 * max(1.0, np.abs(g).max())
    assert np.allclose(nr.ntxent(z, 1.0 / T, g=-3.5)['dz'], -3.5 * ref['dz'], rtol=1e-14, atol=0)


def test_n2_edge():
    ref = nr.ntxent(np.array([[1.0, 2.0], [0.5, -1.0]]), 4.0)
    assert ref['loss'] == 0.0 and np.all(ref['dz'] == 0.0) and np.all(ref['rank'] == 0) and np.all(ref['lse'] == ref['sp'])


@pytest.mark.parametrize('b,D', nr.EXACT_CASES)
def test_rank_is_the_sort_based_count_ties_included(b, D):
    z = nr.exact_inputs(b, D)
    ref = nr.ntxent(z, nr.EXACT_INV_T)
    assert np.array_equal(ref['rank'], nr.rank_by_sort(ref['s'], 2 * b))


@pytest.mark.parametrize('b,D', nr.EXACT_CASES)
def test_exact_inputs_preconditions(b, D):
    z = nr.exact_inputs(b, D)
    N = 2 * b
    assert z.dtype == np.float32 and np.array_equal(z * 8, np.round(z * 8)) and np.abs(z).max() <= 1.0
    s64 = nr.ntxent(z, nr.EXACT_INV_T)['s']
    s32 = (z @ z.T) * np.float32(nr.EXACT_INV_T)                  # fp32 arithmetic, numpy's own order
    assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), s64)
    zr = z[:, ::-1].copy()                                        # ... and in the reverse order of summation
    assert np.array_equal(((zr @ zr.T) * np.float32(nr.EXACT_INV_T)).astype(np.float64), s64)
    pos = nr.pos_index(N)
    off = ~np.eye(N, dtype=bool)
    neg = off.copy()
    neg[np.arange(N), pos] = False
    if b >= 2:                                                    # (b = 1 has no negatives at all)
        assert (neg & (s64 == s64[np.arange(N), pos][:, None])).any()           # an exact tie with the positive
        assert (off & (s64 == np.diag(s64)[:, None])).any()                     # and one with the diagonal
    if D >= 8:                                                    # (D = 1: |s| <= 16 whatever the entries in [-1, 1])
        assert np.abs(np.where(off, s64, 0)).max() > 88.0 or b == 1
        assert np.abs(s64).max() > 88.0
    # P != P^T: the backward pass cannot get away with one of the two terms (b = 2 is two pairs of equal rows: symmetric)
    if b >= 4:
        P = nr.ntxent(z, nr.EXACT_INV_T)['P']
        assert np.abs(P - P.T).max() > 1e-3


def test_cases_name_their_paths():
    assert len(nr.EXACT_CASES) == len(nr.EXACT_PATHS)
    for (b, D), path in zip(nr.EXACT_CASES, nr.EXACT_PATHS):
        assert nr.ntxent_path(2 * b, D)[0] == path
    assert {nr.ntxent_path(2 * b, D)[0] for b, D in nr.FLOAT_CASES} == {'fast'}
    assert nr.ntxent_path(64, 128, aligned=False)[0] == 'generic'
    # more than one split, one split, and splits capped by the tiles per wave
    assert nr.ntxent_path(66, 128) == ('fast', 4, 1) and nr.ntxent_path(512, 128) == ('fast', 4, 4)
    assert nr.ntxent_path(66, 130) == ('generic', 1, 3) and nr.ntxent_path(8192, 128) == ('fast', 4, 1)


def test_path_rule_is_the_librarys(pkg):
    import ctypes as C
    lib = pkg._hip.lib
    for N, D, aligned in [(2, 8, 1), (66, 128, 1), (66, 128, 0), (66, 130, 1), (8, 1, 1), (512, 128, 1), (2048, 64, 1), (8192, 128, 1),
                          (65536, 4, 1), (200, 124, 1)]:
        w, s = C.c_int32(), C.c_int32()
        rc = lib.gca_ntxent_path(N, D, aligned, C.addressof(w), C.addressof(s))
        assert (['generic', 'fast'][rc], w.value, s.value) == nr.ntxent_path(N, D, bool(aligned)), (N, D, aligned)
        assert lib.gca_ntxent_ws_bytes(N, D) > 0
    for N, D in [(3, 8), (0, 8), (65538, 4), (4, 0), (65536, 32768)]:
        assert lib.gca_ntxent_path(N, D, 1, None, None) == -1 and lib.gca_ntxent_ws_bytes(N, D) == -1


def test_hard_float_inputs_have_the_promised_properties():
    z = nr.float_inputs(33, 128, hard=True).astype(np.float64)
    n = np.linalg.norm(z, axis=1)
    assert n.max() / n.min() > 3.0 and np.array_equal(z[0], z[33])
    ref = nr.ntxent(z, 2.0)
    assert np.abs(ref['P'] - ref['P'].T).max() > 1e-3 and ref['lse'].max() - ref['lse'].min() > 1.0
    assert np.abs(ref['s']).max() < 8.5                          # the logit scale of unit rows at T = 0.125
    assert np.abs(np.linalg.norm(nr.float_inputs(5, 32), axis=1) - 1).max() < 1e-6


def test_ops_refuse_bad_arguments_before_touching_a_device(pkg):
    ops = pkg.engine.ops
    z = torch.zeros(4, 8)
    for bad in (torch.zeros(3, 8), torch.zeros(0, 8), torch.zeros(4, 0), torch.zeros(8), torch.zeros(4, 8, dtype=torch.float64),
                torch.zeros(65538, 1)):
        with pytest.raises(ValueError, match='ntxent_fwd'):
            ops.ntxent_fwd(bad, 2.0)
        with pytest.raises(ValueError, match='ntxent_bwd'):
            ops.ntxent_bwd(bad, torch.zeros(bad.shape[0]), 2.0)
    for inv_T in (0.0, -1.0, float('inf'), float('nan'), 1e39):
        with pytest.raises(ValueError, match='1 / T'):
            ops.ntxent_fwd(z, inv_T)
        with pytest.raises(ValueError, match='1 / T'):
            ops.ntxent_bwd(z, torch.zeros(4), inv_T)
    with pytest.raises(ValueError, match='lse'):
        ops.ntxent_bwd(z, torch.zeros(5), 2.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.ntxent_fwd(z, 2.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.ntxent_bwd(z, torch.zeros(4), 2.0)


def test_factories(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    NTXent = importlib.import_module(pkg.__name__ + '.lib.memory.ntxent').NTXent
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'simclr', 32, 16, 8)
    c = pkg.create_contrast(cfg, 100)
    assert isinstance(c, NTXent) and c.T == 0.07 and c.rank is None and len(c.state_dict()) == 0
    with pytest.raises(ValueError):
        NTXent(0.0)
    cfg_bank = parity.make_cfg(pkg, 'R2P1D10T', 'bank', 32, 16, 8)
    with pytest.raises(NotImplementedError, match='mem not suported: bank'):
        pkg.create_contrast(cfg_bank, 100)
    with pytest.raises(NotImplementedError, match='mem not suported: nope'):
        pkg.create_contrast(parity.make_cfg(pkg, 'R2P1D10T', 'nope', 32, 16, 8), 100)
    assert pkg.create_contrast(parity.make_cfg(pkg, 'R2P1D10T', 'simsiam', 32, 16, 8), 100) is None


def test_simclr_wrapper_has_the_moco_state_dict(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    build = importlib.import_module(pkg.__name__ + '.lib.modeling.build')
    gw = importlib.import_module(pkg.__name__ + '.lib.modeling.graph_wrappers')
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'simclr', 32, 16, 8)
    cfg.CONTRAST.NCE_T = 0.2
    model, ema = build.create_visual_model(cfg)
    assert ema is None and isinstance(model.model, gw.SimCLR) and isinstance(model.model, gw.ContrastWrapper) and model.model.T == 0.2
    moco, moco_ema = build.create_visual_model(parity.make_cfg(pkg, 'R2P1D10T', 'moco', 32, 16, 8))
    assert moco_ema is not None and type(moco.model) is gw.ContrastWrapper
    assert list(model.state_dict()) == list(moco.state_dict())
    assert all(k.startswith(('model.encoder.', 'model.proj_head.')) for k in model.state_dict())


def test_trainer_is_exported_and_shares_the_two_view_step(pkg):
    tr = importlib.import_module(pkg.__name__ + '.engine.trainer')
    assert pkg.SimCLRTrainer is tr.SimCLRTrainer
    assert issubclass(tr.SimCLRTrainer, tr._TwoViewTrainer) and issubclass(tr.SimSiamTrainer, tr._TwoViewTrainer)
    for name in ('train_step', 'state_dict', 'load_state_dict', '_fwd_bwd', '_update'):
        assert getattr(tr.SimCLRTrainer, name) is getattr(tr.SimSiamTrainer, name) is getattr(tr._TwoViewTrainer, name)


def test_abi_and_build_lists_name_the_kernel(pkg):
    sig = pkg._hip.SIGNATURES
    assert len(sig['gca_ntxent_fwd'][1]) == 10 and len(sig['gca_ntxent_bwd'][1]) == 10 and len(sig['gca_ntxent_ws_bytes'][1]) == 2
    entry = importlib.import_module('__graft_entry__')
    assert 'ntxent' in entry.SOURCES
    sh = open(os.path.join(ROOT, 'build_hip.sh')).read()
    assert ' ntxent ' in sh and 'ntxent.o' in sh
