"""tests/dino_ref.py against torch's fp64 autograd of the literal loss, the properties of its outputs (teacher rows sum to 1, rows
of dS to 0, the centre moves after it is used), the wrong variants that the GPU bar must tell apart, the preconditions of the
seeded inputs that tests/test_gpu_dino.py relies on, and the host-side wiring of the DINO feature (refusals before any device
is touched, schedules, factories, state-dict keys, trainer, ABI)."""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dino_ref as dr                    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = dr.BAR                             # the GPU tests' bar, of each array's max-abs against fp64
SHAPES = [(3, 5, 7), (33, 130, 65), (65, 128, 3000), (4, 16, 16384)]
PARAMS = [(0.1, 0.04, 0.9), (0.1, 0.07, 0.9), (0.5, 0.02, 0.0)]
OTHERS = ('moco', 'simsiam', 'simclr', 'barlow', 'vicreg', 'swav')


def nrel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def autograd(inputs, Ts, Tt, cm, **variant):
    t = [torch.from_numpy(np.asarray(a, dtype=np.float64)) for a in inputs]
    for a in t[:3]:
        a.requires_grad_(True)
    loss, l12, l21, ent, new_c = dr.torch_chain(*t, Ts, Tt, cm, **variant)
    loss.backward()
    return dict(loss=float(loss.detach()), l12=float(l12.detach()), l21=float(l21.detach()), ent=float(ent), dz1=t[0].grad.numpy(),
                dz2=t[1].grad.numpy(), dC=t[2].grad.numpy(), center=new_c.numpy())


# ----------------------------------------------------------------------------- the specification
@pytest.mark.parametrize('Ts,Tt,cm', PARAMS)
@pytest.mark.parametrize('N,D,K', SHAPES)
def test_spec_matches_torch_autograd_of_the_literal_loss(N, D, K, Ts, Tt, cm):
    inputs = dr.unit_inputs(N, D, K, seed=1)
    want = autograd(inputs, Ts, Tt, cm)
    ref = dr.forward(*inputs, Ts, Tt, cm)
    for k in ('loss', 'l12', 'l21', 'ent'):
        assert abs(ref[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])), k
    for k in ('dz1', 'dz2', 'dC', 'center'):
        assert np.abs(ref[k] - want[k]).max() <= 1e-12 * max(1.0, np.abs(want[k]).max()), k
    scaled = dr.forward(*inputs, Ts, Tt, cm, g=-3.5)
    for k in ('dz1', 'dz2', 'dC'):
        assert nrel(scaled[k], -3.5 * ref[k]) <= 1e-14
    assert abs(ref['loss'] - 0.5 * (ref['l12'] + ref['l21'])) <= 1e-15 * abs(ref['loss'])


@pytest.mark.parametrize('N,D,K', SHAPES)
def test_teacher_rows_sum_to_one_and_gradient_rows_to_zero(N, D, K):
    ref = dr.forward(*dr.unit_inputs(N, D, K, seed=2))
    p = ref['probs']
    assert p.shape == (2, N, K) and (p >= 0).all() and np.abs(p.sum(axis=2) - 1.0).max() <= 1e-12
    for k in ('dS1', 'dS2'):
        assert np.abs(ref[k].sum(axis=1)).max() <= 1e-14 * np.abs(ref[k]).max() * K
    assert 0.0 <= ref['ent'] <= math.log(K) * (1 + 1e-12)


def test_centre_moves_after_the_loss_used_it_and_in_view_order():
    N, D, K = 33, 20, 65
    inputs = dr.unit_inputs(N, D, K, seed=3)
    zt1, zt2, Ct, c = (np.asarray(a, dtype=np.float64) for a in inputs[3:])
    ref = dr.forward(*inputs, cm=0.9)
    mean = np.concatenate([zt1 @ Ct.T, zt2 @ Ct.T]).mean(axis=0)               # the 2 N teacher rows, view 1 first
    assert np.abs(ref['center'] - (0.9 * c + 0.1 * mean)).max() <= 1e-15
    assert np.abs(ref['center'] - c).max() > 1e-3                               # it moves ...
    moved = dr.forward(*inputs[:6], ref['center'])                              # ... and the loss had used the old one
    assert abs(moved['loss'] - ref['loss']) > 100 * BAR * ref['loss']
    assert np.abs(dr.forward(*inputs, cm=0.0)['center'] - mean).max() <= 1e-15  # cm = 0: the batch mean itself
    # the student never sees the centre: a constant added to it changes nothing (softmax is shift-invariant per row)
    shifted = dr.forward(*inputs[:6], c + 0.37)
    assert abs(shifted['loss'] - ref['loss']) <= 1e-12 * ref['loss']


def test_spec_refuses_and_defaults():
    assert dr.DEFAULTS == dict(K=4096, Ts=0.1, Tt=0.04, cm=0.9)
    inputs = dr.unit_inputs(4, 3, 5)
    for kw in (dict(Ts=0.0), dict(Ts=-1.0), dict(Ts=float('inf')), dict(Ts=float('nan')), dict(Tt=0.0), dict(Tt=float('nan')),
               dict(cm=1.0), dict(cm=-0.1), dict(cm=float('nan'))):
        with pytest.raises(ValueError):
            dr.forward(*inputs, **kw)
    zs1, zs2, Cs, zt1, zt2, Ct, c = inputs
    for bad in ((zs1[:1], zs2[:1], Cs, zt1[:1], zt2[:1], Ct, c), (zs1, zs2, Cs[:1], zt1, zt2, Ct[:1], c[:1]),
                (zs1, zs2[:, :2], Cs, zt1, zt2, Ct, c), (zs1, zs2, Cs, zt1, zt2, Ct[:4], c), (zs1, zs2, Cs, zt1, zt2, Ct, c[:4])):
        with pytest.raises(ValueError):
            dr.forward(*bad)
    dr.forward(*inputs, Ts=1e-3, Tt=1e-3, cm=0.0)                               # the edges are inside
    for bad in [(1, 8, 8), (8193, 8, 8), (8, 0, 8), (8, 8193, 8), (8, 8, 1), (8, 8, 65537)]:
        with pytest.raises(ValueError):
            dr.ws_bytes(*bad)
    assert dr.ws_bytes(64, 128, 4096) == (2 * 64 * 4096 + 256) * 4


def test_the_cases_straddle_every_edge():
    for must in [(2, 1, 2), (3, 5, 7), (33, 130, 65), (64, 128, 128), (65, 128, 3000), (256, 128, 1000), (4096, 16, 64),
                 (4, 16, 16384), (2, 8, 65536)]:
        assert must in dr.KERNEL_CASES
    for axis in range(3):                                                        # below, at and above a tile on every axis
        sizes = {c[axis] for c in dr.KERNEL_CASES}
        assert any(s < dr.TILE for s in sizes) and any(s % dr.TILE == 0 for s in sizes) and any(s > dr.TILE and s % dr.TILE for s in sizes)
    ks = {c[2] for c in dr.KERNEL_CASES}                                         # below, at a multiple of and off the row stride
    assert any(k < dr.ROW_STRIDE for k in ks) and any(k % dr.ROW_STRIDE == 0 for k in ks) and any(k > dr.ROW_STRIDE and k % dr.ROW_STRIDE for k in ks)
    assert min(ks) == 2 and max(ks) == 65536
    assert dr.TEMPERATURES == [(0.1, 0.07), (0.5, 0.02)] and dr.TEMPERATURE_CASES == [(33, 130, 65), (65, 128, 3000)]


# ----------------------------------------------------------------------------- what the GPU bar must tell apart
@pytest.mark.parametrize('N,D,K', SHAPES)
def test_wrong_variants_miss_by_100_bars(N, D, K):
    inputs = dr.unit_inputs(N, D, K)
    assert np.abs(inputs[6]).max() > 0.01                                        # a zero centre would hide two of them
    Ts, Tt, cm = dr.DEFAULTS['Ts'], dr.DEFAULTS['Tt'], dr.DEFAULTS['cm']
    ref = dr.forward(*inputs, Ts, Tt, cm)
    keys = ('loss', 'dz1', 'dz2', 'dC', 'center')
    right = autograd(inputs, Ts, Tt, cm)
    assert max(nrel(right[k], ref[k]) for k in keys) <= 1e-12
    variants = dict(no_centring=dict(centring='none'), centre_on_student=dict(centring='student'),
                    centre_updated_first=dict(center_first=True), temperatures_swapped=dict(swap_temperatures=True),
                    same_view_pairs=dict(cross=False), missing_half=dict(half=False))
    for name, kw in variants.items():
        got = autograd(inputs, Ts, Tt, cm, **kw)
        miss = max(nrel(got[k], ref[k]) for k in keys)
        assert miss > 100 * BAR, (name, miss)


# ----------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize('N,D,K', dr.KERNEL_CASES)
def test_unit_inputs_meet_their_preconditions(N, D, K):
    inputs = dr.unit_inputs(N, D, K)
    zs1, zs2, Cs, zt1, zt2, Ct, c = inputs
    for a, shape in ((zs1, (N, D)), (zs2, (N, D)), (Cs, (K, D)), (zt1, (N, D)), (zt2, (N, D)), (Ct, (K, D))):
        assert a.dtype == np.float32 and a.shape == shape and a.flags['C_CONTIGUOUS']
        assert np.abs(np.sqrt((a.astype(np.float64) ** 2).sum(1)) - 1.0).max() <= 2e-7
    assert c.dtype == np.float32 and c.shape == (K,) and 0.01 < np.abs(c).max() < 1.0
    assert not np.array_equal(zs1, zs2) and (D == 1 or not np.array_equal(zs1, zt1))
    # the largest exponent argument the kernels meet: (max - min of St - c) / Tt at the smallest Tt of the cases
    for zt in (zt1, zt2):
        X = zt.astype(np.float64) @ Ct.astype(np.float64).T - c
        assert (X.max() - X.min()) / 0.02 <= 150.0
    # the reference is no cancellation residue: the loss and every gradient keep the size of their terms
    ref = dr.forward(*inputs)
    assert ref['loss'] >= 0.5 and min(ref['l12'], ref['l21']) >= 0.5
    for k in ('dz1', 'dz2', 'dC'):
        assert np.abs(ref[k]).max() >= 1e-3 / (2.0 * N * dr.DEFAULTS['Ts']), k
    assert all(np.array_equal(a, b) for a, b in zip(inputs, dr.unit_inputs(N, D, K)))


@pytest.mark.parametrize('N,D,K', dr.ADVERSARIAL_CASES)
def test_adversarial_inputs(N, D, K):
    eq = dr.forward(*dr.equal_scores_inputs(N, D, K))
    assert abs(eq['ent'] - math.log(K)) <= 1e-12 * math.log(K) and abs(eq['loss'] - math.log(K)) <= 1e-12 * math.log(K)
    assert np.abs(eq['probs'] * K - 1.0).max() <= 1e-12
    oh = dr.forward(*dr.one_hot_scores_inputs(N, D, K), Tt=0.04)
    small = oh['probs'][:, :, 1:]
    assert 1e-23 < small.min() and small.max() < 1e-21 and small.min() > float(np.finfo(np.float32).tiny)
    assert np.isfinite(oh['ent']) and 0.0 < oh['ent'] < 1e-15
    assert all(np.isfinite(oh[k]).all() for k in ('dz1', 'dz2', 'dC'))


# ----------------------------------------------------------------------------- schedules
def test_schedules_at_their_end_points(pkg):
    S = pkg.lib.solver
    assert S.dino_teacher_temp(0, 30, 0.04, 0.07) == 0.04
    assert S.dino_teacher_temp(30, 30, 0.04, 0.07) == 0.07 and S.dino_teacher_temp(31, 30, 0.04, 0.07) == 0.07
    assert abs(S.dino_teacher_temp(15, 30, 0.04, 0.07) - 0.055) <= 1e-15
    assert S.dino_teacher_temp(0, 0, 0.04, 0.07) == 0.07
    assert S.cosine_momentum(0, 100, 0.996) == 0.996 and S.cosine_momentum(100, 100, 0.996) == 1.0
    assert abs(S.cosine_momentum(50, 100, 0.996) - 0.998) <= 1e-15
    vals = [S.cosine_momentum(i, 100, 0.9) for i in range(101)]
    assert all(a <= b for a, b in zip(vals, vals[1:])) and all(0.9 <= v <= 1.0 for v in vals)
    for bad in ((-1, 30, 0.04, 0.07), (0, -1, 0.04, 0.07), (0, 30, 0.0, 0.07), (0, 30, 0.04, -1.0)):
        with pytest.raises(ValueError):
            S.dino_teacher_temp(*bad)
    for bad in ((-1, 100, 0.9), (101, 100, 0.9), (0, 0, 0.9), (0, 100, 1.5), (0, 100, -0.1)):
        with pytest.raises(ValueError):
            S.cosine_momentum(*bad)


# ----------------------------------------------------------------------------- host-side wiring (no device)
def test_ops_refuse_before_any_device_is_touched(pkg):
    ops = pkg.engine.ops
    z, C, c, tt = torch.zeros(4, 8), torch.zeros(6, 8), torch.zeros(6), torch.full((1,), 0.04)
    dS, dC = torch.zeros(2, 4, 6), torch.zeros(6, 8)

    def fwd(zs1=z, zs2=z, Cs=C, zt1=z, zt2=z, Ct=C, Ts=0.1, tt=tt, cm=0.9, center=c):
        return ops.dino_fwd(zs1, zs2, Cs, zt1, zt2, Ct, Ts, tt, cm, center, True)

    for kw in (dict(zs1=torch.zeros(1, 8), zs2=torch.zeros(1, 8)), dict(zs2=torch.zeros(4, 9)), dict(Cs=torch.zeros(6, 9)),
               dict(Cs=torch.zeros(1, 8)), dict(zs1=z.double(), zs2=z.double()), dict(Cs=C.double()), dict(zs1=z[0], zs2=z[0]),
               dict(zt1=torch.zeros(5, 8), zt2=torch.zeros(5, 8)), dict(Ct=torch.zeros(7, 8)), dict(zt2=torch.zeros(4, 9)),
               dict(center=torch.zeros(7)), dict(center=c.double()), dict(center=torch.zeros(6, 1)),
               dict(tt=torch.zeros(2)), dict(tt=tt.double())):
        with pytest.raises(ValueError, match='dino_fwd'):
            fwd(**kw)
    big = torch.zeros(8193, 2)
    with pytest.raises(ValueError, match='dino_fwd'):
        fwd(zs1=big, zs2=big, zt1=big, zt2=big, Cs=torch.zeros(6, 2), Ct=torch.zeros(6, 2))
    for kw, name in ((dict(Ts=0.0), 'Ts'), (dict(Ts=-0.1), 'Ts'), (dict(Ts=float('inf')), 'Ts'), (dict(Ts=float('nan')), 'Ts'),
                     (dict(Ts=1e-39), 'Ts'), (dict(cm=1.0), 'cm'), (dict(cm=-0.01), 'cm'), (dict(cm=float('nan')), 'cm')):
        with pytest.raises(ValueError, match=name):
            fwd(**kw)
    for bad in ((0.1, 0.0, 0.9), (0.1, float('nan'), 0.9), (0.1, 1e-39, 0.9), (0.1, 0.04, 1.0), (0.0, 0.04, 0.9)):
        with pytest.raises(ValueError):
            ops.dino_params('x', *bad)
    assert ops.dino_params('x', 0.1, 0.04, 0.0) == (0.1, 0.04, 0.0)
    for gs in (float('inf'), float('nan'), 1e39):
        with pytest.raises(ValueError, match='gscale_host'):
            ops.dino_bwd(z, z, C, dS, dC, False, gscale_host=gs)
    with pytest.raises(ValueError, match='dS'):
        ops.dino_bwd(z, z, C, torch.zeros(2, 4, 5), dC, False)
    with pytest.raises(ValueError, match='dC'):
        ops.dino_bwd(z, z, C, dS, torch.zeros(8, 6), False)
    for a, b, m in ((torch.zeros(4), torch.zeros(5), tt), (torch.zeros(4).double(), torch.zeros(4).double(), tt),
                    (torch.zeros(0), torch.zeros(0), tt), (torch.zeros(4), torch.zeros(4), torch.zeros(2)),
                    (torch.zeros(4, 4).t(), torch.zeros(4, 4), tt)):
        with pytest.raises(ValueError, match='ema_update_dev'):
            ops.ema_update_dev(a, b, m)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fwd()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.dino_bwd(z, z, C, dS, dC, False)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.ema_update_dev(torch.zeros(4), torch.zeros(4), tt)


def test_factories(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    DINOLoss = importlib.import_module(pkg.__name__ + '.lib.memory.dino').DINOLoss
    build = importlib.import_module(pkg.__name__ + '.lib.modeling.build')
    gw = importlib.import_module(pkg.__name__ + '.lib.modeling.graph_wrappers')
    Cc = pkg.get_defaults().CONTRAST
    assert (Cc.DINO_K, Cc.DINO_TS, Cc.DINO_TT, Cc.DINO_CM) == (4096, 0.1, 0.04, 0.9)
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'dino', 32, 16, 8)
    cfg.CONTRAST.DINO_K = 24
    c = pkg.create_contrast(cfg, 100)
    assert isinstance(c, DINOLoss) and (c.K, c.Ts, c.Tt, c.cm) == (24, 0.1, 0.04, 0.9)
    assert list(c.state_dict()) == ['center'] and tuple(c.center.shape) == (24,) and float(c.center.abs().max()) == 0.0
    assert c.l12 is None and c.l21 is None and c.ent is None
    c.set_teacher_temp(0.07)
    assert c.Tt == 0.07
    with pytest.raises(ValueError):
        c.set_teacher_temp(0.0)
    d = DINOLoss()
    assert (d.K, d.Ts, d.Tt, d.cm) == (4096, 0.1, 0.04, 0.9)
    for bad in (dict(K=1), dict(K=65537), dict(K=2.5), dict(Ts=0.0), dict(Tt=float('nan')), dict(cm=1.0), dict(cm=-0.5)):
        with pytest.raises(ValueError):
            DINOLoss(**bad)
    for key, v in (('DINO_K', 1), ('DINO_TS', -1.0), ('DINO_TT', 0.0), ('DINO_CM', 1.0)):
        bad = parity.make_cfg(pkg, 'R2P1D10T', 'dino', 32, 16, 8)
        setattr(bad.CONTRAST, key, v)
        with pytest.raises(ValueError):
            pkg.create_contrast(bad, 100)
    z, C = torch.zeros(4, 8), torch.zeros(24, 8)
    for args in ((z, torch.zeros(4, 9), C, z, z, C), (z, z, torch.zeros(23, 8), z, z, C), (z, z, C, torch.zeros(5, 8), z, C),
                 (z, z, C, z, z, torch.zeros(24, 9))):
        with pytest.raises(ValueError, match='DINOLoss'):
            c(*args)
    # the model factory: an EMA twin of the same layout for 'dino', still None for the six others
    torch.manual_seed(5)
    model, ema = build.create_visual_model(cfg)
    assert isinstance(model.model, gw.DINO) and isinstance(ema.model, gw.DINO) and isinstance(model.model, gw.ContrastWrapper)
    assert ema is not model and ema.model.encoder is not model.model.encoder
    keys = list(model.state_dict())
    assert list(ema.state_dict()) == keys
    assert [tuple(v.shape) for v in ema.state_dict().values()] == [tuple(v.shape) for v in model.state_dict().values()]
    assert all(k.startswith(('model.encoder.', 'model.proj_head.', 'model.prototypes.')) for k in keys)
    assert [k for k in keys if k.startswith('model.prototypes.')] == ['model.prototypes.weight']
    w = model.model.prototypes.weight
    assert isinstance(w, torch.nn.Parameter) and tuple(w.shape) == (24, 32) and float((w.detach().norm(dim=1) - 1.0).abs().max()) <= 1e-6
    simclr, none = build.create_visual_model(parity.make_cfg(pkg, 'R2P1D10T', 'simclr', 32, 16, 8))
    assert none is None and list(simclr.state_dict()) == [k for k in keys if k != 'model.prototypes.weight']
    for mem in OTHERS:
        _, e = build.create_visual_model(parity.make_cfg(pkg, 'R2P1D10T', mem, 32, 16, 8))
        assert (e is not None) == (mem == 'moco'), mem
    assert tuple(gw.GraphWrapper(model.model.encoder, 32, 'mlp', 'dino').model.prototypes.weight.shape) == (4096, 32)
    for bad in (1, 65537, 2.5):
        with pytest.raises(ValueError):
            gw.DINO(model.model.encoder, 32, 'mlp', bad)
    import dino_model as dm                                                      # the oracle of the GPU test has the same keys
    om, oe = dm.oracle_dino('R2P1D10T', 8, 32, 24)
    assert list(om.state_dict()) == keys == list(oe.state_dict())


def test_trainer_is_exported_and_shares_the_two_view_step(pkg):
    tr = importlib.import_module(pkg.__name__ + '.engine.trainer')
    assert pkg.DINOTrainer is tr.DINOTrainer and issubclass(tr.DINOTrainer, tr._TwoViewTrainer)
    assert tr.DINOTrainer._fwd_bwd is tr._TwoViewTrainer._fwd_bwd and tr.DINOTrainer._bwd_stage is tr._TwoViewTrainer._bwd_stage
    import inspect
    src = inspect.getsource(tr.DINOTrainer.train_step)
    assert 'super().train_step(images)' in src and '_Graphed' not in src         # the step plumbing is not copied


def test_abi_and_build_lists_name_the_kernel(pkg):
    sig = pkg._hip.SIGNATURES
    assert len(sig['gca_dino_fwd'][1]) == 19 and len(sig['gca_dino_fwd_grid'][1]) == 20 and len(sig['gca_dino_ws_bytes'][1]) == 3 and len(sig['gca_ema_update_dev'][1]) == 5
    lib = pkg._hip.lib
    for N, D, K in dr.KERNEL_CASES + [(64, 128, 4096), (64, 128, 65536), (8192, 8192, 65536)]:
        assert lib.gca_dino_ws_bytes(N, D, K) == dr.ws_bytes(N, D, K) > 0
    for N, D, K in [(1, 8, 8), (0, 8, 8), (8193, 4, 8), (4, 0, 8), (4, 8193, 8), (4, 8, 1), (4, 8, 65537), (-2, 8, 8)]:
        assert lib.gca_dino_ws_bytes(N, D, K) == -1
    # NULL pointers and bad parameters are refused before anything is launched (no device needed to see it)
    assert lib.gca_dino_fwd(None, None, None, None, None, None, 4, 8, 6, 0.1, None, 0.9, None, 1, None, None, None, None, None) == -1
    assert lib.gca_ema_update_dev(None, None, 4, None, None) == -1
    entry = importlib.import_module('__graft_entry__')
    assert 'dino' in entry.SOURCES
    sh = open(os.path.join(ROOT, 'build_hip.sh')).read()
    assert ' dino ' in sh and 'dino.o' in sh
    hdr = open(os.path.join(ROOT, 'include', 'gca_hip.h')).read()
    for name in ('gca_dino_fwd', 'gca_dino_fwd_grid', 'gca_dino_ws_bytes', 'gca_ema_update_dev'):
        assert name in hdr
    src = open(os.path.join(ROOT, pkg.__name__, 'csrc', 'dino.hip')).read()
    assert '#include "mma_tile.h"' in src and 'chunk_mma(' in src and '__builtin_amdgcn_mfma' not in src
    assert 'atomic' not in src.lower().replace('no atomics', '') and 'cooperative' not in src.lower()
