"""tests/swav_ref.py against torch's fp64 autograd of a literal transcription of the published loop, the properties of the codes
(rows sum to 1, columns converge to N / K, the scaling-vector form and the shift change nothing), the wrong variants that the
GPU bar must tell apart, the preconditions of the seeded inputs that tests/test_gpu_swav.py relies on, and the host-side wiring
of the SwAV feature (refusals before any device is touched, factories, state-dict keys, trainer, ABI)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swav_ref as sr                    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = sr.BAR                             # the GPU tests' bar, of each array's max-abs against fp64
SHAPES = [(2, 1, 2), (3, 5, 7), (8, 16, 24), (33, 20, 65), (64, 32, 130)]
PARAMS = [(0.05, 0.1, 3), (0.025, 0.1, 3), (0.3, 0.5, 1), (0.05, 0.07, 7)]


def nrel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def autograd(z1, z2, C, eps, T, iters, **variant):
    t1, t2, tc = (torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_(True) for a in (z1, z2, C))
    loss, l12, l21 = sr.torch_chain(t1, t2, tc, eps, T, iters, **variant)
    loss.backward()
    return dict(loss=float(loss.detach()), l12=float(l12.detach()), l21=float(l21.detach()), dz1=t1.grad.numpy(),
                dz2=t2.grad.numpy(), dC=tc.grad.numpy())


# ----------------------------------------------------------------------------- the specification
@pytest.mark.parametrize('eps,T,iters', PARAMS)
@pytest.mark.parametrize('N,D,K', SHAPES)
def test_spec_matches_torch_autograd_of_the_literal_loop(N, D, K, eps, T, iters):
    z1, z2, C = sr.unit_inputs(N, D, K, seed=1)
    want = autograd(z1, z2, C, eps, T, iters)
    ref = sr.grads(z1, z2, C, eps, T, iters)
    for k in ('loss', 'l12', 'l21'):
        assert abs(ref[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])), k
    for k in ('dz1', 'dz2', 'dC'):
        assert np.abs(ref[k] - want[k]).max() <= 1e-12 * max(1.0, np.abs(want[k]).max()), k
    scaled = sr.grads(z1, z2, C, eps, T, iters, g=-3.5)
    for k in ('dz1', 'dz2', 'dC'):
        assert nrel(scaled[k], -3.5 * ref[k]) <= 1e-14
    assert abs(ref['loss'] - 0.5 * (ref['l12'] + ref['l21'])) <= 1e-15 * abs(ref['loss'])


@pytest.mark.parametrize('N,D,K', SHAPES)
def test_codes_are_positive_and_rows_sum_to_one(N, D, K):
    z1, _, C = sr.unit_inputs(N, D, K, seed=2)
    S = z1.astype(np.float64) @ C.astype(np.float64).T
    for eps, iters in ((0.05, 3), (0.025, 1), (1.0, 16)):
        q = sr.sinkhorn(S, eps, iters)
        assert q.shape == (N, K) and (q > 0).all()
        assert np.abs(q.sum(axis=1) - 1.0).max() <= 1e-12


# Sinkhorn converges linearly at a rate that the spread of the scores sets: the contraction factor of one round is
# tanh(delta / 4)^2 with delta the largest log cross-ratio of exp(S / eps), at most 2 (max S - min S) / eps (Franklin & Lorenz
# 1989).  Unit rows in D = 5 spread the scores over 30 eps and 50 rounds then leave 3e-4; at the feature widths the model has
# (D >= 32: a spread of at most 24 eps here, 16 eps at the workload's D = 128) they reach N / K far inside 1e-6.
@pytest.mark.parametrize('N,D,K', [(64, 32, 130), (33, 130, 65), (64, 128, 128), (65, 128, 3000)])
def test_codes_columns_converge_to_the_uniform_marginal(N, D, K):
    z1, _, C = sr.unit_inputs(N, D, K, seed=2)
    S = z1.astype(np.float64) @ C.astype(np.float64).T
    assert (S.max() - S.min()) / 0.05 <= 24.0
    q = sr.sinkhorn(S, 0.05, 50)
    assert np.abs(q.sum(axis=0) * K / N - 1.0).max() <= 1e-6
    assert np.abs(q.sum(axis=1) - 1.0).max() <= 1e-12


@pytest.mark.parametrize('eps,iters', [(0.05, 3), (0.025, 3), (0.5, 16)])
@pytest.mark.parametrize('N,D,K', SHAPES)
def test_scaling_vectors_and_shift_change_nothing(N, D, K, eps, iters):
    _, z2, C = sr.unit_inputs(N, D, K, seed=3)
    S = z2.astype(np.float64) @ C.astype(np.float64).T
    q = sr.sinkhorn(S, eps, iters)
    for shift in (None, 1.0, 0.0, -0.37):
        assert np.abs(sr.sinkhorn_scaled(S, eps, iters, shift) - q).max() <= 1e-12 * q.max(), shift
    assert np.abs(sr.sinkhorn(S - 0.61, eps, iters) - q).max() <= 1e-12 * q.max()


def test_rows_normalize_spec():
    rng = np.random.RandomState(4)
    C = rng.randn(7, 5) * rng.uniform(0.1, 30.0, size=(7, 1))
    C[3] = 0.0
    out = sr.rows_normalize(C)
    assert np.array_equal(out[3], np.zeros(5))
    keep = [0, 1, 2, 4, 5, 6]
    assert np.abs(np.sqrt((out[keep] ** 2).sum(1)) - 1.0).max() <= 1e-15
    assert np.allclose(out[keep] * np.sqrt((C[keep] ** 2).sum(1, keepdims=True)), C[keep], rtol=1e-15, atol=0)


def test_spec_refuses_and_defaults():
    assert sr.DEFAULTS == dict(K=3000, eps=0.05, T=0.1, iters=3)
    z1, z2, C = sr.unit_inputs(4, 3, 5)
    for kw in (dict(eps=0.02), dict(eps=1.5), dict(eps=float('nan')), dict(T=0.0), dict(T=-1.0), dict(T=float('inf')),
               dict(T=float('nan')), dict(iters=0), dict(iters=17), dict(iters=2.5)):
        with pytest.raises(ValueError):
            sr.loss_parts(z1, z2, C, **kw)
    with pytest.raises(ValueError):
        sr.loss_parts(z1[:1], z2[:1], C)
    with pytest.raises(ValueError):
        sr.loss_parts(z1, z2, C[:1])
    with pytest.raises(ValueError):
        sr.loss_parts(z1, z2[:, :2], C)
    with pytest.raises(ValueError):
        sr.loss_parts(z1, z2, C[:, :2])
    sr.loss_parts(z1, z2, C, eps=np.float32(0.025), T=1e-3, iters=16)           # the edges are inside


def test_one_route_and_the_cases_straddle_its_tile_edge():
    assert sr.ROUTES == ('tiled',)
    for case in sr.KERNEL_CASES + sr.ADVERSARIAL_CASES + [(2, 1, 2), (8192, 8192, 65536)]:
        assert sr.route(*case) == 'tiled'
    for bad in [(1, 8, 8), (8193, 8, 8), (8, 0, 8), (8, 8193, 8), (8, 8, 1), (8, 8, 65537)]:
        with pytest.raises(ValueError):
            sr.route(*bad)
    for axis in range(3):                                                        # below, at and above a tile on every axis
        sizes = {c[axis] for c in sr.KERNEL_CASES}
        assert any(s < sr.TILE for s in sizes) and any(s % sr.TILE == 0 for s in sizes) and any(s > sr.TILE and s % sr.TILE for s in sizes)
    splits = {c: sr.dz_splits(*c) for c in sr.KERNEL_CASES}                       # one slab and several, the cap of 32 included
    assert splits[(2, 1, 2)] == 1 and splits[(4096, 16, 64)] == 1 and splits[(33, 130, 65)] == 1
    assert splits[(65, 128, 3000)] == 12 and splits[(256, 128, 1000)] == 4 and splits[(4, 16, 16384)] == 32
    assert sr.dz_splits(64, 128, 256) == 1 and sr.dz_splits(64, 128, 257) == 2 and sr.dz_splits(8192, 8192, 65536) == 1
    for must in [(2, 1, 2), (3, 5, 7), (33, 130, 65), (64, 128, 128), (65, 128, 3000), (256, 128, 1000), (4096, 16, 64), (4, 16, 16384)]:
        assert must in sr.KERNEL_CASES


# ----------------------------------------------------------------------------- what the GPU bar must tell apart
@pytest.mark.parametrize('N,D,K', [(33, 130, 65), (64, 128, 128), (65, 128, 3000)])
def test_wrong_variants_miss_by_100_bars(N, D, K):
    z1, z2, C = sr.unit_inputs(N, D, K)
    eps, T, iters = sr.DEFAULTS['eps'], sr.DEFAULTS['T'], sr.DEFAULTS['iters']
    ref = sr.grads(z1, z2, C, eps, T, iters)
    keys = ('loss', 'dz1', 'dz2', 'dC')
    right = autograd(z1, z2, C, eps, T, iters)
    assert max(nrel(right[k], ref[k]) for k in keys) <= 1e-12
    variants = dict(unswapped=dict(swapped=False), row_softmax=dict(codes='softmax'), no_temperature=dict(use_T=False),
                    codes_with_gradient=dict(detach=False))
    for name, kw in variants.items():
        got = autograd(z1, z2, C, eps, T, iters, **kw)
        miss = max(nrel(got[k], ref[k]) for k in keys)
        assert miss > 100 * BAR, (name, miss)
    one_view = ref['dS1'].T @ z1.astype(np.float64)                               # a dC that forgets view 2
    assert nrel(one_view, ref['dC']) > 100 * BAR


# ----------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize('N,D,K', sr.KERNEL_CASES)
def test_unit_inputs_meet_their_preconditions(N, D, K):
    z1, z2, C = sr.unit_inputs(N, D, K)
    for a, shape in ((z1, (N, D)), (z2, (N, D)), (C, (K, D))):
        assert a.dtype == np.float32 and a.shape == shape and a.flags['C_CONTIGUOUS']
        assert np.abs(np.sqrt((a.astype(np.float64) ** 2).sum(1)) - 1.0).max() <= 2e-7
    assert not np.array_equal(z1, z2)
    eps = float(np.float32(sr.ADVERSARIAL_EPS))
    for z in (z1, z2):
        S = z.astype(np.float64) @ C.astype(np.float64).T
        assert (S.max() - S.min()) / eps <= 80.0 and S.max() <= 1.0 + 2e-7
    # the reference is no cancellation residue: the loss and every gradient keep the size of their terms
    ref = sr.grads(z1, z2, C)
    T = sr.DEFAULTS['T']
    assert ref['loss'] >= 0.5 and min(ref['l12'], ref['l21']) >= 0.5
    for k in ('dz1', 'dz2', 'dC'):
        assert np.abs(ref[k]).max() >= 1e-3 / (2.0 * N * T), k
    again = sr.unit_inputs(N, D, K)
    assert all(np.array_equal(a, b) for a, b in zip((z1, z2, C), again))
    assert D == 1 or not np.array_equal(sr.unit_inputs(N, D, K, seed=1)[0], z1)


@pytest.mark.parametrize('N,D,K', sr.ADVERSARIAL_CASES)
def test_adversarial_inputs(N, D, K):
    eps = float(np.float32(sr.ADVERSARIAL_EPS))
    for make, lo, hi in ((sr.equal_scores_inputs, -1.0, -1.0), (sr.one_hot_scores_inputs, -1.0, 1.0)):
        z1, z2, C = make(N, D, K)
        S = z1.astype(np.float64) @ C.astype(np.float64).T
        assert S.min() == lo and S.max() == hi and (S.max() - S.min()) / eps <= 80.0
        assert np.exp((lo - 1.0) / eps) > float(np.finfo(np.float32).tiny)        # the smallest P stays a normal fp32 number
        ref = sr.grads(z1, z2, C, eps, 0.1, 3)
        assert np.abs(ref['codes'] * K - 1.0).max() <= 1e-9                       # uniform codes, whatever the column sums were
        assert np.isfinite(ref['loss']) and all(np.isfinite(ref[k]).all() for k in ('dz1', 'dz2', 'dC'))
    z1, z2, C = sr.equal_scores_inputs(N, D, K)
    assert abs(sr.loss_parts(z1, z2, C, eps, 0.1, 3)['loss'] - np.log(K)) <= 1e-12 * np.log(K)


# ----------------------------------------------------------------------------- host-side wiring (no device)
def test_ops_refuse_before_any_device_is_touched(pkg):
    ops = pkg.engine.ops
    z, C = torch.zeros(4, 8), torch.zeros(6, 8)
    dS, dC = torch.zeros(2, 4, 6), torch.zeros(6, 8)
    for a, b, c in ((torch.zeros(1, 8), torch.zeros(1, 8), C), (z, torch.zeros(4, 9), C), (z, z, torch.zeros(6, 9)),
                    (z, z, torch.zeros(1, 8)), (z.double(), z.double(), C), (z, z, C.double()), (z[0], z[0], C),
                    (torch.zeros(8193, 2), torch.zeros(8193, 2), torch.zeros(6, 2)), (torch.zeros(4, 8193), torch.zeros(4, 8193), torch.zeros(6, 8193))):
        with pytest.raises(ValueError, match='swav_fwd'):
            ops.swav_fwd(a, b, c, 0.05, 0.1, 3)
    for kw, name in ((dict(eps=0.02), 'eps'), (dict(eps=1.01), 'eps'), (dict(eps=float('nan')), 'eps'), (dict(T=0.0), 'T'),
                     (dict(T=-0.1), 'T'), (dict(T=float('inf')), 'T'), (dict(T=float('nan')), 'T'), (dict(T=1e-39), 'T'),
                     (dict(iters=0), 'iters'), (dict(iters=17), 'iters'), (dict(iters=1.5), 'iters')):
        args = dict(eps=0.05, T=0.1, iters=3)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            ops.swav_fwd(z, z, C, **args)
    for gs in (float('inf'), float('nan'), 1e39):
        with pytest.raises(ValueError, match='gscale_host'):
            ops.swav_bwd(z, z, C, dS, dC, False, gscale_host=gs)
    with pytest.raises(ValueError, match='dS'):
        ops.swav_bwd(z, z, C, torch.zeros(2, 4, 5), dC, False)
    with pytest.raises(ValueError, match='dC'):
        ops.swav_bwd(z, z, C, dS, torch.zeros(8, 6), False)
    with pytest.raises(ValueError, match='rows_normalize_'):
        ops.rows_normalize_(torch.zeros(8))
    with pytest.raises(ValueError, match='rows_normalize_'):
        ops.rows_normalize_(torch.zeros(8, 6).t())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.swav_fwd(z, z, C, 0.05, 0.1, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.swav_bwd(z, z, C, dS, dC, False)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.rows_normalize_(C)


def test_factories(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    SwAVLoss = importlib.import_module(pkg.__name__ + '.lib.memory.swav').SwAVLoss
    Cc = pkg.get_defaults().CONTRAST
    assert (Cc.SWAV_K, Cc.SWAV_EPS, Cc.SWAV_T, Cc.SWAV_ITERS) == (3000, 0.05, 0.1, 3)
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'swav', 32, 16, 8)
    c = pkg.create_contrast(cfg, 100)
    assert isinstance(c, SwAVLoss) and (c.eps, c.T, c.iters) == (0.05, 0.1, 3)
    assert len(c.state_dict()) == 0 and c.l12 is None and c.l21 is None
    d = SwAVLoss()
    assert (d.eps, d.T, d.iters) == (0.05, 0.1, 3)
    cfg.CONTRAST.SWAV_EPS, cfg.CONTRAST.SWAV_T, cfg.CONTRAST.SWAV_ITERS = 0.03, 0.2, 5
    c = pkg.create_contrast(cfg, 100)
    assert (c.eps, c.T, c.iters) == (0.03, 0.2, 5)
    for bad in (dict(eps=0.01), dict(eps=2.0), dict(T=0.0), dict(T=float('nan')), dict(iters=0), dict(iters=17)):
        with pytest.raises(ValueError):
            SwAVLoss(**bad)
    for key, v in (('SWAV_EPS', 0.001), ('SWAV_T', -1.0), ('SWAV_ITERS', 40)):
        bad = parity.make_cfg(pkg, 'R2P1D10T', 'swav', 32, 16, 8)
        setattr(bad.CONTRAST, key, v)
        with pytest.raises(ValueError):
            pkg.create_contrast(bad, 100)
    z = torch.zeros(4, 8)
    for a, b, cc in ((z, torch.zeros(4, 9), torch.zeros(6, 8)), (z, z, torch.zeros(6, 9)), (z[0], z[0], torch.zeros(6, 8))):
        with pytest.raises(ValueError, match='two'):
            SwAVLoss()(a, b, cc)
    with pytest.raises(NotImplementedError, match='mem not suported: nope'):
        pkg.create_contrast(parity.make_cfg(pkg, 'R2P1D10T', 'nope', 32, 16, 8), 100)


def test_wrapper_state_dict_and_prototypes(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    build = importlib.import_module(pkg.__name__ + '.lib.modeling.build')
    gw = importlib.import_module(pkg.__name__ + '.lib.modeling.graph_wrappers')
    layers = importlib.import_module(pkg.__name__ + '.engine.layers')
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'swav', 32, 16, 8)
    cfg.CONTRAST.SWAV_K, cfg.CONTRAST.SWAV_T = 24, 0.2
    torch.manual_seed(5)
    model, ema = build.create_visual_model(cfg)
    inner = model.model
    assert ema is None and isinstance(inner, gw.SwAV) and isinstance(inner, gw.ContrastWrapper)
    assert (inner.eps, inner.T, inner.iters) == (0.05, 0.2, 3)
    w = inner.prototypes.weight
    assert isinstance(w, torch.nn.Parameter) and tuple(w.shape) == (24, 32) and w.requires_grad
    assert not isinstance(inner.prototypes, layers._PackedWeight)
    assert float((w.detach().norm(dim=1) - 1.0).abs().max()) <= 1e-6
    assert float(w.detach().abs().max()) <= 1.0 and float(w.detach().std()) > 0.05
    keys = list(model.state_dict())
    assert all(k.startswith(('model.encoder.', 'model.proj_head.', 'model.prototypes.')) for k in keys)
    assert [k for k in keys if k.startswith('model.prototypes.')] == ['model.prototypes.weight']
    # the encoder and head keys are those of the SimCLR / MoCo model, whose loaders must go on reading this checkpoint
    simclr, _ = build.create_visual_model(parity.make_cfg(pkg, 'R2P1D10T', 'simclr', 32, 16, 8))
    assert list(simclr.state_dict()) == [k for k in keys if k != 'model.prototypes.weight']
    # the defaults reach the model when the config does not set the keys
    d = gw.GraphWrapper(inner.encoder, 32, 'mlp', 'swav').model
    assert tuple(d.prototypes.weight.shape) == (3000, 32) and (d.eps, d.T, d.iters) == (0.05, 0.1, 3)
    for bad in (dict(K=1), dict(K=65537), dict(K=2.5), dict(eps=0.01), dict(T=0.0), dict(iters=0)):
        with pytest.raises(ValueError):
            gw.SwAV(inner.encoder, 32, **bad)
    for key, v in (('SWAV_K', 1), ('SWAV_EPS', 3.0), ('SWAV_T', float('nan')), ('SWAV_ITERS', 17)):
        bad = parity.make_cfg(pkg, 'R2P1D10T', 'swav', 32, 16, 8)
        setattr(bad.CONTRAST, key, v)
        with pytest.raises(ValueError):
            build.create_visual_model(bad)
    # the oracle of the GPU test has the same keys
    import swav_model as sm
    assert list(sm.oracle_swav('R2P1D10T', 8, 32, 24).state_dict()) == keys


def test_trainer_is_exported_and_shares_the_two_view_step(pkg):
    tr = importlib.import_module(pkg.__name__ + '.engine.trainer')
    assert pkg.SwAVTrainer is tr.SwAVTrainer and issubclass(tr.SwAVTrainer, tr._TwoViewTrainer)
    for name in ('train_step', 'state_dict', 'load_state_dict', '_fwd_bwd', '_update'):
        assert getattr(tr.SwAVTrainer, name) is getattr(tr.SimSiamTrainer, name) is getattr(tr._TwoViewTrainer, name)


def test_abi_and_build_lists_name_the_kernel(pkg):
    sig = pkg._hip.SIGNATURES
    assert len(sig['gca_swav_fwd'][1]) == 14 and len(sig['gca_swav_bwd'][1]) == 15 and len(sig['gca_swav_dz_splits'][1]) == 3
    assert len(sig['gca_swav_ws_bytes'][1]) == 3 and len(sig['gca_rows_normalize'][1]) == 4
    lib = pkg._hip.lib
    for N, D, K in sr.KERNEL_CASES + [(64, 128, 3000), (64, 128, 256), (64, 128, 257), (8192, 8192, 65536), (2, 8192, 65536)]:
        assert lib.gca_swav_ws_bytes(N, D, K) == sr.ws_bytes(N, D, K) > 0
        assert lib.gca_swav_dz_splits(N, D, K) == sr.dz_splits(N, D, K)
    assert lib.gca_swav_dz_splits(1, 8, 8) == -1
    for N, D, K in [(1, 8, 8), (0, 8, 8), (8193, 4, 8), (4, 0, 8), (4, 8193, 8), (4, 8, 1), (4, 8, 65537), (-2, 8, 8)]:
        assert lib.gca_swav_ws_bytes(N, D, K) == -1
    entry = importlib.import_module('__graft_entry__')
    assert 'swav' in entry.SOURCES
    sh = open(os.path.join(ROOT, 'build_hip.sh')).read()
    assert ' swav ' in sh and 'swav.o' in sh
    hdr = open(os.path.join(ROOT, 'include', 'gca_hip.h')).read()
    for name in ('gca_swav_fwd', 'gca_swav_bwd', 'gca_swav_ws_bytes', 'gca_swav_dz_splits', 'gca_rows_normalize'):
        assert name in hdr
    src = open(os.path.join(ROOT, pkg.__name__, 'csrc', 'swav.hip')).read()
    assert '#include "mma_tile.h"' in src and 'chunk_mma(' in src and '__builtin_amdgcn_mfma' not in src
    assert 'atomic' not in src.lower().replace('no atomics', '') and 'cooperative' not in src.lower()
