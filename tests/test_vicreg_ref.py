"""tests/vicreg_ref.py against torch's fp64 autograd of the published loss, the properties of the seeded inputs that
tests/test_gpu_vicreg.py relies on (exact inputs: the same bits in fp32 under two summation orders and in fp64; float inputs:
hinges on both sides of 1 with a margin, one constant and one nearly collapsed column, an fp32 torch chain within a third of
the GPU bar of fp64; every wrong variant misses by 100x the bar somewhere), and the host-side wiring of the VICReg feature
(refusals before any device is touched, factories, state-dict keys, trainer, ABI)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vicreg_ref as vr                  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5                               # the GPU tests' bar: Barlow's rule, of each tensor's max-abs against fp64


def nrel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def autograd(z1, z2, coeffs, eps=1e-4, dtype=torch.float64):
    t1 = torch.from_numpy(np.asarray(z1)).to(dtype).requires_grad_(True)
    t2 = torch.from_numpy(np.asarray(z2)).to(dtype).requires_grad_(True)
    loss, inv, varl, covl = vr.torch_chain(t1, t2, *coeffs, eps)
    loss.backward()
    return [float(v.detach()) for v in (loss, inv, varl, covl)], t1.grad.numpy(), t2.grad.numpy()


_REF = {}


def float_ref(N, D, coeffs):
    """The fp64 specification on the float inputs, computed once per case and left unchanged."""
    key = (N, D, coeffs)
    if key not in _REF:
        z1, z2 = vr.float_inputs(N, D)
        _REF[key] = (z1, z2, vr.vicreg(z1, z2, *coeffs))
    return _REF[key]


# ----------------------------------------------------------------------------- the specification
@pytest.mark.parametrize('coeffs', [(25.0, 25.0, 1.0), (1.0, 0.0, 4.0), (0.0, 16.0, 1.0)])
@pytest.mark.parametrize('N,D', [(2, 3), (7, 5), (5, 33), (64, 40), (32, 256)])
def test_spec_matches_torch_autograd(N, D, coeffs):
    rng = np.random.RandomState(N + D)
    z1 = rng.randn(N, D) * rng.uniform(0.3, 2.0, size=(1, D)) + rng.uniform(-1, 1, size=(1, D))
    z2 = z1 + 0.3 * rng.randn(N, D)
    (loss, inv, varl, covl), g1, g2 = autograd(z1, z2, coeffs)
    ref = vr.vicreg(z1, z2, *coeffs)
    for k, want in (('loss', loss), ('inv', inv), ('varl', varl), ('covl', covl)):
        assert abs(ref[k] - want) <= 1e-12 * max(1.0, abs(want)), k
    assert np.abs(ref['dz1'] - g1).max() <= 1e-12 * max(1.0, np.abs(g1).max())
    assert np.abs(ref['dz2'] - g2).max() <= 1e-12 * max(1.0, np.abs(g2).max())
    scaled = vr.vicreg(z1, z2, *coeffs, g=-3.5)
    assert np.allclose(scaled['dz1'], -3.5 * ref['dz1'], rtol=1e-14, atol=0)
    # the saved state is what its names say
    assert np.allclose(ref['stats'][0], z1.mean(0), rtol=0, atol=1e-13)
    assert np.allclose(ref['stats'][3], np.sqrt(z2.var(0, ddof=1) + 1e-4), rtol=0, atol=1e-13)
    assert np.allclose(ref['covm'][0], np.cov(z1.T).reshape(D, D), rtol=0, atol=1e-12)
    assert np.allclose(ref['covm'][1], np.cov(z2.T).reshape(D, D), rtol=0, atol=1e-12)
    assert np.array_equal(ref['covm'], ref['covm'].transpose(0, 2, 1))


def test_spec_refuses_and_defaults():
    z = np.zeros((4, 3))
    assert vr.DEFAULTS == dict(sim=25.0, std=25.0, cov=1.0, eps=1e-4)
    for kw in (dict(sim=-1.0), dict(std=float('nan')), dict(cov=float('inf')), dict(eps=-1e-4)):
        with pytest.raises(ValueError):
            vr.vicreg(z, z, **kw)
    with pytest.raises(ValueError):
        vr.vicreg(np.zeros((1, 3)), np.zeros((1, 3)))
    with pytest.raises(ValueError):
        vr.vicreg(z, np.zeros((4, 2)))
    # eps = 0 and a constant column: 0 / 0, as the torch chain gives -- documented, not special-cased
    z1 = np.random.RandomState(0).randn(4, 3)
    z1[:, 1] = 2.0
    assert np.isnan(vr.vicreg(z1, z1 + 1.0, eps=0.0)['dz1'][:, 1]).all()
    _, g1, _ = autograd(z1, z1 + 1.0, (25.0, 25.0, 1.0), eps=0.0)
    assert np.isnan(g1[:, 1]).all()


# ----------------------------------------------------------------------------- exact inputs
@pytest.mark.parametrize('N,D', vr.EXACT_CASES)
def test_exact_inputs_preconditions(N, D):
    z1, z2 = vr.exact_inputs(N, D)
    k = (N - 1).bit_length() - 1
    assert N == 2 ** k + 1 and z1.dtype == z2.dtype == np.float32 and z1.shape == z2.shape == (N, D)
    for z in (z1, z2):
        assert np.all((z == 0.5).sum(axis=0) == 2 ** (k - 1)) and np.all((z == -0.5).sum(axis=0) == 2 ** (k - 1))
        assert np.all((z == 0.0).sum(axis=0) == 1)
    assert not np.array_equal(z1, z2) and np.array_equal(z1[:, 1::2], z2[:, 1::2])
    sim, std, cov = vr.EXACT_COEFFS
    assert sim == 0.0
    r64 = vr.vicreg(z1, z2, sim, std, cov, eps=0.0)
    assert np.all(r64['stats'][[0, 2]] == 0.0) and np.all(r64['stats'][[1, 3]] == 0.5)        # the hinge is active everywhere
    assert r64['varl'] == 0.5 and r64['inv'] > 0
    assert np.array_equal(r64['covm'] * 2 ** (k + 2), np.round(r64['covm'] * 2 ** (k + 2)))  # every Cov[i,j] is m / 2^(k+2)
    assert np.all(np.diagonal(r64['covm'], axis1=1, axis2=2) == 0.25)
    if D >= 32:
        assert r64['covl'] > 0
    assert np.abs(r64['dz1']).max() > 0 and np.abs(r64['dz2']).max() > 0
    # fp32, in two different orders of summation, gives the fp64 bits: the GPU test may demand bit equality
    for reverse in (False, True):
        r32 = vr.vicreg(z1, z2, np.float32(sim), np.float32(std), np.float32(cov), eps=np.float32(0), dtype=np.float32,
                        reverse=reverse)
        for key in ('stats', 'covm', 'dz1', 'dz2'):
            assert r32[key].dtype == np.float32 and np.array_equal(r32[key].astype(np.float64), r64[key]), (key, reverse)
        for key in ('loss', 'varl', 'covl'):
            assert isinstance(r32[key], np.float32) and float(r32[key]) == float(r64[key]), (key, reverse)
        # inv = S / (N D) with N odd is not dyadic: S is exact, and each precision holds the correctly rounded quotient
        assert r32['inv'] == np.float32(r64['inv']) and r64['inv'] * N * D == np.round(r64['inv'] * N * D)
    # with sim = 16 the loss and the gradient pick that quotient up: fp32 is then only close (the GPU test uses the float bar)
    s64 = vr.vicreg(z1, z2, 16.0, std, cov, eps=0.0)
    s32 = vr.vicreg(z1, z2, np.float32(16), np.float32(std), np.float32(cov), eps=np.float32(0), dtype=np.float32)
    assert abs(float(s32['loss']) - s64['loss']) <= BAR / 3 * s64['loss'] and nrel(s32['dz1'], s64['dz1']) <= BAR / 3


# ----------------------------------------------------------------------------- float inputs
@pytest.mark.parametrize('N,D', vr.FLOAT_CASES)
def test_float_inputs_preconditions(N, D):
    z1, z2 = vr.float_inputs(N, D)
    assert N >= 5 and z1.dtype == z2.dtype == np.float32
    eps = vr.DEFAULTS['eps']
    for coeffs in vr.FLOAT_COEFFS:
        _, _, ref = float_ref(N, D, coeffs)
        sd = ref['stats'][[1, 3]]
        sd32 = vr.vicreg(z1, z2, *coeffs, dtype=np.float32)['stats'][[1, 3]]
        assert np.abs(sd - 1.0).min() > 1e-3 and np.array_equal(sd < 1, sd32 < 1)      # fp32 and fp64 take the same hinge branch
        assert (sd < 1).any()
        if D >= 2:
            assert (sd > 1).any()
        if D >= 3:                       # the constant column: sd = sqrt(eps), and a hinge gradient of xc / sd = 0
            assert np.all(z1[:, -1] == z1[0, -1]) and np.all(z2[:, -1] == z2[0, -1])
            assert np.allclose(sd[:, -1], np.sqrt(eps), rtol=1e-12, atol=0)
            only_hinge = vr.vicreg(z1, z2, 0.0, 25.0, 0.0)
            assert np.all(only_hinge['dz1'][:, -1] == 0.0) and np.all(only_hinge['dz2'][:, -1] == 0.0)
            assert np.abs(only_hinge['dz1'][:, :-1]).max() > 0
        assert abs(sd[0, 0] - np.sqrt(0.02 ** 2 + eps)) < 1e-6                          # the nearly collapsed column
        assert np.abs(ref['stats'][[0, 2]]).max() > (2.0 if D >= 32 else 0.0)           # means of a few units
        # the tolerance rule: the unfused fp32 torch chain, autograd gradient included, on these very inputs is within a third
        # of the bar of the fp64 specification
        (l32, i32, v32, c32), g1, g2 = autograd(z1, z2, coeffs, dtype=torch.float32)
        e = dict(loss=abs(l32 - ref['loss']) / abs(ref['loss']), inv=abs(i32 - ref['inv']) / ref['inv'],
                 varl=abs(v32 - ref['varl']) / ref['varl'], dz1=nrel(g1, ref['dz1']), dz2=nrel(g2, ref['dz2']))
        if D > 1:
            e['covl'] = abs(c32 - ref['covl']) / ref['covl']
        print('MEASURED vicreg fp32 torch chain N=%d D=%d coeffs=%s: %s' % (N, D, coeffs, ' '.join('%s %.2e' % kv for kv in e.items())))
        assert max(e.values()) <= BAR / 3, e


@pytest.mark.parametrize('mistake', vr.MISTAKES)
def test_mistakes_that_must_show(mistake):
    """Each wrong variant moves the loss or a gradient by at least 100x the GPU bar on at least one float case."""
    worst = {}
    for coeffs in vr.FLOAT_COEFFS:
        for N, D in vr.FLOAT_CASES:
            z1, z2, ref = float_ref(N, D, coeffs)
            bad = vr.vicreg(z1, z2, *coeffs, mistake=mistake)
            worst[(N, D, coeffs)] = max(abs(bad['loss'] - ref['loss']) / abs(ref['loss']), nrel(bad['dz1'], ref['dz1']),
                                        nrel(bad['dz2'], ref['dz2']))
    print('MEASURED vicreg mistake %s: worst miss %.2e, smallest %.2e' % (mistake, max(worst.values()), min(worst.values())))
    assert max(worst.values()) >= 100 * BAR, (mistake, worst)


# ----------------------------------------------------------------------------- host-side wiring
def test_ops_refuse_bad_arguments_before_touching_a_device(pkg):
    ops = pkg.engine.ops
    z = torch.zeros(4, 8)
    saved = (torch.zeros(4, 8), torch.zeros(2, 8, 8))
    for bad in (torch.zeros(1, 8), torch.zeros(0, 8), torch.zeros(4, 0), torch.zeros(8), torch.zeros(4, 8, dtype=torch.float64),
                torch.zeros(65537, 1), torch.zeros(2, 8193)):
        with pytest.raises(ValueError, match='vicreg_fwd'):
            ops.vicreg_fwd(bad, bad, 25.0, 25.0, 1.0)
        with pytest.raises(ValueError, match='vicreg_bwd'):
            ops.vicreg_bwd(bad, bad, *saved, 25.0, 25.0, 1.0)
    with pytest.raises(ValueError, match='vicreg_fwd'):
        ops.vicreg_fwd(z, torch.zeros(4, 9), 25.0, 25.0, 1.0)
    for pos, name in enumerate(('sim', 'std', 'cov')):
        for v in (-1.0, float('inf'), float('nan'), 1e39):
            coeffs = [25.0, 25.0, 1.0]
            coeffs[pos] = v
            with pytest.raises(ValueError, match=name):
                ops.vicreg_fwd(z, z, *coeffs)
            with pytest.raises(ValueError, match=name):
                ops.vicreg_bwd(z, z, *saved, *coeffs)
    for eps in (-1e-5, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='eps'):
            ops.vicreg_fwd(z, z, 25.0, 25.0, 1.0, eps)
    for gs in (float('inf'), float('nan'), 1e39):
        with pytest.raises(ValueError, match='gscale_host'):
            ops.vicreg_bwd(z, z, *saved, 25.0, 25.0, 1.0, gscale_host=gs)
    with pytest.raises(ValueError, match='covm'):
        ops.vicreg_bwd(z, z, torch.zeros(4, 8), torch.zeros(8, 8), 25.0, 25.0, 1.0)
    with pytest.raises(ValueError, match='stats'):
        ops.vicreg_bwd(z, z, torch.zeros(3, 8), torch.zeros(2, 8, 8), 25.0, 25.0, 1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.vicreg_fwd(z, z, 25.0, 25.0, 1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.vicreg_bwd(z, z, *saved, 25.0, 25.0, 1.0)


def test_factories(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    VICRegLoss = importlib.import_module(pkg.__name__ + '.lib.memory.vicreg').VICRegLoss
    C = pkg.get_defaults().CONTRAST
    assert (C.VIC_SIM, C.VIC_STD, C.VIC_COV) == (25.0, 25.0, 1.0)
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'vicreg', 32, 16, 8)
    c = pkg.create_contrast(cfg, 100)
    assert isinstance(c, VICRegLoss) and (c.sim_coeff, c.std_coeff, c.cov_coeff, c.eps) == (25.0, 25.0, 1.0, 1e-4)
    assert len(c.state_dict()) == 0 and c.inv is None and c.var is None and c.cov is None
    d = VICRegLoss()
    assert (d.sim_coeff, d.std_coeff, d.cov_coeff, d.eps) == (25.0, 25.0, 1.0, 1e-4)
    cfg.CONTRAST.VIC_SIM, cfg.CONTRAST.VIC_STD, cfg.CONTRAST.VIC_COV = 10.0, 5.0, 0.04
    c = pkg.create_contrast(cfg, 100)
    assert (c.sim_coeff, c.std_coeff, c.cov_coeff) == (10.0, 5.0, 0.04)
    for bad in (dict(sim_coeff=-1.0), dict(std_coeff=float('nan')), dict(cov_coeff=float('inf')), dict(eps=-1.0)):
        with pytest.raises(ValueError):
            VICRegLoss(**bad)
    with pytest.raises(ValueError, match='two'):
        VICRegLoss()(torch.zeros(4, 8), torch.zeros(4, 9))
    with pytest.raises(NotImplementedError, match='mem not suported: nope'):
        pkg.create_contrast(parity.make_cfg(pkg, 'R2P1D10T', 'nope', 32, 16, 8), 100)


def test_wrapper_state_dict_and_projector(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    build = importlib.import_module(pkg.__name__ + '.lib.modeling.build')
    gw = importlib.import_module(pkg.__name__ + '.lib.modeling.graph_wrappers')
    ph = importlib.import_module(pkg.__name__ + '.lib.modeling.project_head')
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'vicreg', 32, 16, 8)
    cfg.CONTRAST.VIC_COV = 0.5
    model, ema = build.create_visual_model(cfg)
    inner = model.model
    assert ema is None and isinstance(inner, gw.VICReg)
    assert (inner.sim_coeff, inner.std_coeff, inner.cov_coeff, inner.eps) == (25.0, 25.0, 0.5, 1e-4)
    assert type(inner.projection) is ph.BarlowProjector and inner.projection.l3.bias is None
    keys = list(model.state_dict())
    assert all(k.startswith(('model.encoder.', 'model.projection.')) for k in keys)
    # the same keys as the Barlow Twins model, whose state dict this feature must not change
    barlow, _ = build.create_visual_model(parity.make_cfg(pkg, 'R2P1D10T', 'barlow', 32, 16, 8))
    assert isinstance(barlow.model, gw.BarlowTwins) and list(barlow.state_dict()) == keys
    with pytest.raises(ValueError):
        gw.VICReg(inner.encoder, 32, sim_coeff=-1.0)
    # the oracle of the GPU test has the same keys
    import vicreg_model as vm
    assert list(vm.oracle_vicreg('R2P1D10T', 8, 32).state_dict()) == keys


def test_trainer_is_exported_and_shares_the_two_view_step(pkg):
    tr = importlib.import_module(pkg.__name__ + '.engine.trainer')
    assert pkg.VICRegTrainer is tr.VICRegTrainer and issubclass(tr.VICRegTrainer, tr._TwoViewTrainer)
    for name in ('train_step', 'state_dict', 'load_state_dict', '_fwd_bwd', '_update'):
        assert getattr(tr.VICRegTrainer, name) is getattr(tr.SimSiamTrainer, name) is getattr(tr._TwoViewTrainer, name)


def test_abi_and_build_lists_name_the_kernel(pkg):
    sig = pkg._hip.SIGNATURES
    assert len(sig['gca_vicreg_fwd'][1]) == 13 and len(sig['gca_vicreg_bwd'][1]) == 15 and len(sig['gca_vicreg_ws_bytes'][1]) == 2
    lib = pkg._hip.lib
    for N, D in [(2, 1), (5, 33), (256, 2048), (65536, 2047), (32, 8192), (65536, 8192)]:
        assert lib.gca_vicreg_ws_bytes(N, D) > 0
    for N, D in [(1, 8), (0, 8), (65537, 4), (4, 0), (4, 8193), (-2, 8)]:
        assert lib.gca_vicreg_ws_bytes(N, D) == -1
    entry = importlib.import_module('__graft_entry__')
    assert 'vicreg' in entry.SOURCES
    sh = open(os.path.join(ROOT, 'build_hip.sh')).read()
    assert ' vicreg ' in sh and 'vicreg.o' in sh
    hdr = open(os.path.join(ROOT, 'include', 'gca_hip.h')).read()
    assert 'gca_vicreg_fwd' in hdr and 'gca_vicreg_bwd' in hdr and 'gca_vicreg_ws_bytes' in hdr
    # the tile helpers live in one header that both loss files include
    csrc = os.path.join(ROOT, pkg.__name__, 'csrc')
    for name in ('barlow.hip', 'vicreg.hip'):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "mma_tile.h"' in src and 'chunk_mma(' in src and '__builtin_amdgcn_mfma' not in src
