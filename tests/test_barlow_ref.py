"""tests/barlow_ref.py against torch's fp64 autograd, the properties of the seeded inputs that tests/test_gpu_barlow.py relies
on (exact inputs: the same bits in fp32 under two summation orders and in fp64; float inputs: spread scales, non-zero means,
correlated views, an fp32 torch chain within 3e-6 of fp64; the wrong variants miss by 1e-3 or more), and the host-side wiring
of the Barlow Twins feature (refusals before any device is touched, factories, state-dict keys, trainer, ABI)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import barlow_ref as br                  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def nrel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def autograd64(z1, z2, lambd, eps=1e-5, dtype=torch.float64):
    t1 = torch.from_numpy(np.asarray(z1)).to(dtype).requires_grad_(True)
    t2 = torch.from_numpy(np.asarray(z2)).to(dtype).requires_grad_(True)
    loss = br.torch_chain(t1, t2, lambd, eps)
    loss.backward()
    return float(loss.detach()), t1.grad.numpy(), t2.grad.numpy()


_REF = {}


def float_ref(N, D, lambd):
    """The fp64 specification on the float inputs, computed once per case and left unchanged."""
    key = (N, D, lambd)
    if key not in _REF:
        z1, z2 = br.float_inputs(N, D)
        _REF[key] = (z1, z2, br.barlow(z1, z2, lambd))
    return _REF[key]


# ----------------------------------------------------------------------------- the specification
@pytest.mark.parametrize('lambd', [0.0051, 1.0])
@pytest.mark.parametrize('N,D', [(2, 3), (5, 33), (64, 40), (32, 256)])
def test_spec_matches_torch_autograd(N, D, lambd):
    rng = np.random.RandomState(N + D)
    z1 = rng.randn(N, D) * rng.uniform(0.5, 2.0, size=(1, D)) + rng.uniform(-1, 1, size=(1, D))
    z2 = z1 + 0.3 * rng.randn(N, D)
    loss, g1, g2 = autograd64(z1, z2, lambd)
    ref = br.barlow(z1, z2, lambd)
    assert abs(ref['loss'] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert np.abs(ref['dz1'] - g1).max() <= 1e-12 * max(1.0, np.abs(g1).max())
    assert np.abs(ref['dz2'] - g2).max() <= 1e-12 * max(1.0, np.abs(g2).max())
    assert abs(ref['on'] + lambd * ref['off'] - ref['loss']) <= 1e-15 * max(1.0, abs(loss))
    scaled = br.barlow(z1, z2, lambd, g=-3.5)
    assert np.allclose(scaled['dz1'], -3.5 * ref['dz1'], rtol=1e-14, atol=0)
    # the saved state is what its names say
    a = (z1 - z1.mean(0)) / np.sqrt(z1.var(0) + 1e-5)
    b = (z2 - z2.mean(0)) / np.sqrt(z2.var(0) + 1e-5)
    assert np.allclose(ref['C'], a.T @ b / N, rtol=0, atol=1e-13)
    assert np.allclose(ref['stats'][0], z1.mean(0), rtol=0, atol=1e-13) and np.allclose(ref['stats'][3], 1 / np.sqrt(z2.var(0) + 1e-5))


# ----------------------------------------------------------------------------- exact inputs
@pytest.mark.parametrize('N,D', br.EXACT_CASES)
def test_exact_inputs_preconditions(N, D):
    z1, z2 = br.exact_inputs(N, D)
    assert N & (N - 1) == 0 and z1.dtype == z2.dtype == np.float32 and z1.shape == z2.shape == (N, D)
    for z in (z1, z2):
        assert np.array_equal(np.abs(z), np.ones_like(z)) and np.all(z.sum(axis=0) == 0)      # +-1, equal counts
    assert not np.array_equal(z1, z2)
    r64 = br.barlow(z1, z2, br.EXACT_LAMBDA, eps=0.0)
    assert np.all(r64['stats'][[0, 2]] == 0.0) and np.all(r64['stats'][[1, 3]] == 1.0)
    assert np.array_equal(r64['C'] * N, np.round(r64['C'] * N))                               # every C[i,j] is k / N
    if D > 1:
        assert r64['off'] > 0
    assert r64['on'] > 0
    if N > 2:                            # (at N = 2 every standardised entry is +-1 whatever z is: the gradient is zero)
        assert np.abs(r64['dz1']).max() > 0 and np.abs(r64['dz2']).max() > 0
    else:
        assert np.abs(r64['dz1']).max() == 0 and np.abs(r64['dz2']).max() == 0
    # fp32, in two different orders of summation, gives the fp64 bits: the GPU test may demand bit equality
    for reverse in (False, True):
        r32 = br.barlow(z1, z2, np.float32(br.EXACT_LAMBDA), eps=np.float32(0), dtype=np.float32, reverse=reverse)
        for k in ('stats', 'C', 'rsum', 'dz1', 'dz2'):
            assert r32[k].dtype == np.float32 and np.array_equal(r32[k].astype(np.float64), r64[k]), (k, reverse)
        for k in ('on', 'off', 'loss'):
            assert isinstance(r32[k], np.float32) and float(r32[k]) == float(r64[k]), (k, reverse)


# ----------------------------------------------------------------------------- float inputs
@pytest.mark.parametrize('N,D', br.FLOAT_CASES)
def test_float_inputs_preconditions(N, D):
    z1, z2 = br.float_inputs(N, D)
    assert N >= 5 and z1.dtype == z2.dtype == np.float32
    if D >= 32:
        sd = z1.astype(np.float64).std(axis=0)
        assert 15.0 < sd.max() / sd.min() < 60.0                   # column scales spread over about 20x
        assert np.abs(z1.astype(np.float64).mean(axis=0)).max() > 2.0              # means of a few units
    for lambd in br.FLOAT_LAMBDAS:
        _, _, ref = float_ref(N, D, lambd)
        diag = np.diag(ref['C'])
        assert np.median(diag) > 0.75 and (N < 33 or diag.min() > 0.5)             # view 2 is a noisy copy of view 1
        if D > 1 and N >= 33:
            offd = ref['C'][~np.eye(D, dtype=bool)]
            assert np.sqrt((offd ** 2).mean()) < 0.25
        # the unfused fp32 torch chain on these very inputs is within 3e-6 of fp64
        l32, g1, g2 = autograd64(z1, z2, lambd, dtype=torch.float32)
        e = (abs(l32 - ref['loss']) / abs(ref['loss']), nrel(g1, ref['dz1']), nrel(g2, ref['dz2']))
        print('MEASURED barlow fp32 torch chain N=%d D=%d lambda=%g: loss %.2e dz1 %.2e dz2 %.2e' % ((N, D, lambd) + e))
        assert max(e) <= 3e-6, e


@pytest.mark.parametrize('mistake', br.MISTAKES)
def test_mistakes_that_must_show(mistake):
    """Each wrong variant misses fp64 by at least 1e-3 on the float inputs: 100x the GPU bar."""
    worst = {}
    for N, D in br.FLOAT_CASES:
        if D == 1 and mistake in ('g_transposed',):
            continue                                               # (a 1 x 1 matrix is its own transpose)
        lambd = 0.0051                                             # (lambda = 1 makes 'lambda_on_diag' the right formula)
        z1, z2, ref = float_ref(N, D, lambd)
        bad = br.barlow(z1, z2, lambd, mistake=mistake)
        miss = max(abs(bad['loss'] - ref['loss']) / abs(ref['loss']), nrel(bad['dz1'], ref['dz1']), nrel(bad['dz2'], ref['dz2']))
        worst[(N, D)] = miss
        assert miss >= 1e-3, (mistake, N, D, miss)
    assert len(worst) >= len(br.FLOAT_CASES) - 1


# ----------------------------------------------------------------------------- host-side wiring
def test_ops_refuse_bad_arguments_before_touching_a_device(pkg):
    ops = pkg.engine.ops
    z = torch.zeros(4, 8)

    def saved(N, D):
        return torch.zeros(4, D), torch.zeros(D, D), torch.zeros(2, D)

    for bad in (torch.zeros(1, 8), torch.zeros(0, 8), torch.zeros(4, 0), torch.zeros(8), torch.zeros(4, 8, dtype=torch.float64),
                torch.zeros(65537, 1), torch.zeros(2, 8193)):
        with pytest.raises(ValueError, match='barlow_fwd'):
            ops.barlow_fwd(bad, bad, 0.005)
        with pytest.raises(ValueError, match='barlow_bwd'):
            ops.barlow_bwd(bad, bad, *saved(4, 8), 0.005)
    with pytest.raises(ValueError, match='barlow_fwd'):
        ops.barlow_fwd(z, torch.zeros(4, 9), 0.005)
    for lam in (-1.0, float('inf'), float('nan'), 1e39):
        with pytest.raises(ValueError, match='lambda'):
            ops.barlow_fwd(z, z, lam)
        with pytest.raises(ValueError, match='lambda'):
            ops.barlow_bwd(z, z, *saved(4, 8), lam)
    for eps in (-1e-5, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='eps'):
            ops.barlow_fwd(z, z, 0.005, eps)
    for gs in (float('inf'), float('nan'), 1e39):
        with pytest.raises(ValueError, match='gscale_host'):
            ops.barlow_bwd(z, z, *saved(4, 8), 0.005, gscale_host=gs)
    with pytest.raises(ValueError, match='cmat'):
        ops.barlow_bwd(z, z, torch.zeros(4, 8), torch.zeros(8, 7), torch.zeros(2, 8), 0.005)
    with pytest.raises(ValueError, match='stats'):
        ops.barlow_bwd(z, z, torch.zeros(3, 8), torch.zeros(8, 8), torch.zeros(2, 8), 0.005)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.barlow_fwd(z, z, 0.005)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.barlow_bwd(z, z, *saved(4, 8), 0.005)


def test_factories(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    BarlowTwinsLoss = importlib.import_module(pkg.__name__ + '.lib.memory.barlow').BarlowTwinsLoss
    assert pkg.get_defaults().CONTRAST.BT_LAMBDA == 0.0051
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'barlow', 32, 16, 8)
    c = pkg.create_contrast(cfg, 100)
    assert isinstance(c, BarlowTwinsLoss) and c.lambd == 0.0051 and c.eps == 1e-5 and len(c.state_dict()) == 0
    assert c.on_diag is None and c.off_diag is None
    cfg.CONTRAST.BT_LAMBDA = 0.02
    assert pkg.create_contrast(cfg, 100).lambd == 0.02
    for bad in (dict(lambd=-1.0), dict(lambd=float('nan')), dict(eps=-1.0)):
        with pytest.raises(ValueError):
            BarlowTwinsLoss(**bad)
    with pytest.raises(NotImplementedError, match='mem not suported: bank'):
        pkg.create_contrast(parity.make_cfg(pkg, 'R2P1D10T', 'bank', 32, 16, 8), 100)
    with pytest.raises(NotImplementedError, match='mem not suported: nope'):
        pkg.create_contrast(parity.make_cfg(pkg, 'R2P1D10T', 'nope', 32, 16, 8), 100)
    assert pkg.create_contrast(parity.make_cfg(pkg, 'R2P1D10T', 'simsiam', 32, 16, 8), 100) is None


def test_wrapper_state_dict_and_projector(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    build = importlib.import_module(pkg.__name__ + '.lib.modeling.build')
    gw = importlib.import_module(pkg.__name__ + '.lib.modeling.graph_wrappers')
    ph = importlib.import_module(pkg.__name__ + '.lib.modeling.project_head')
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'barlow', 32, 16, 8)
    cfg.CONTRAST.BT_LAMBDA = 0.01
    model, ema = build.create_visual_model(cfg)
    assert ema is None and isinstance(model.model, gw.BarlowTwins) and model.model.lambd == 0.01
    proj = model.model.projection
    assert isinstance(proj, ph.BarlowProjector) and proj.l3.bias is None and tuple(proj.l3.weight.shape) == (32, 32)
    keys = list(model.state_dict())
    assert all(k.startswith(('model.encoder.', 'model.projection.')) for k in keys)
    assert [k for k in keys if k.startswith('model.projection.l3')] == ['model.projection.l3.weight']
    simsiam, _ = build.create_visual_model(parity.make_cfg(pkg, 'R2P1D10T', 'simsiam', 32, 16, 8))
    enc = [k for k in keys if k.startswith('model.encoder.')]
    assert enc == [k for k in simsiam.state_dict() if k.startswith('model.encoder.')] and len(enc) > 100
    assert [k for k in keys if k.startswith('model.projection.l1')] == [k for k in simsiam.state_dict() if k.startswith('model.projection.l1')]
    # the oracle of the GPU test has the same keys
    import barlow_model as bm
    assert list(bm.oracle_barlow('R2P1D10T', 8, 32).state_dict()) == keys


def test_trainer_is_exported_and_shares_the_two_view_step(pkg):
    tr = importlib.import_module(pkg.__name__ + '.engine.trainer')
    assert pkg.BarlowTwinsTrainer is tr.BarlowTwinsTrainer and issubclass(tr.BarlowTwinsTrainer, tr._TwoViewTrainer)
    for name in ('train_step', 'state_dict', 'load_state_dict', '_fwd_bwd', '_update'):
        assert getattr(tr.BarlowTwinsTrainer, name) is getattr(tr.SimSiamTrainer, name) is getattr(tr._TwoViewTrainer, name)


def test_abi_and_build_lists_name_the_kernel(pkg):
    sig = pkg._hip.SIGNATURES
    assert len(sig['gca_barlow_fwd'][1]) == 12 and len(sig['gca_barlow_bwd'][1]) == 14 and len(sig['gca_barlow_ws_bytes'][1]) == 2
    lib = pkg._hip.lib
    for N, D in [(2, 1), (5, 33), (256, 2048), (65536, 2047), (32, 8192), (65536, 8192)]:
        assert lib.gca_barlow_ws_bytes(N, D) > 0
    for N, D in [(1, 8), (0, 8), (65537, 4), (4, 0), (4, 8193), (-2, 8)]:
        assert lib.gca_barlow_ws_bytes(N, D) == -1
    entry = importlib.import_module('__graft_entry__')
    assert 'barlow' in entry.SOURCES
    sh = open(os.path.join(ROOT, 'build_hip.sh')).read()
    assert ' barlow ' in sh and 'barlow.o' in sh
    hdr = open(os.path.join(ROOT, 'include', 'gca_hip.h')).read()
    assert 'gca_barlow_fwd' in hdr and 'gca_barlow_bwd' in hdr and 'gca_barlow_ws_bytes' in hdr
