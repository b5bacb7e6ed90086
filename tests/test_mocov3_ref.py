"""tests/mocov3_ref.py against torch's fp64 autograd of the literal MoCo v3 loss, the properties of the test inputs that
tests/test_gpu_mocov3.py relies on, the wrong variants its bar must tell apart, the dispatch rule at its edges, and the host
layers (MoCoV3Loss, the MoCoV3 wrapper, both factories) -- all without a GPU."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mocov3_ref as mr                  # noqa: E402

BAR = 1e-5                               # the GPU tests' bar
ROOM = 6                                 # ... must sit this far above what fp32 arithmetic itself costs (measured below)
ALL_FLOAT = [(N, D, T, False) for N, D in mr.FLOAT_CASES for T in mr.FLOAT_TS] + [(N, D, mr.HARD_T, True) for N, D, _ in mr.HARD_CASES]


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def autograd(xs, T, loss_fn=None):
    """fp64 torch autograd of the literal loss -> (loss, dq1, dq2, dk1, dk2)."""
    ts = [torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_(True) for x in xs]
    loss = (loss_fn or mr.torch_chain)(*ts, T)
    loss.backward()
    return (float(loss),) + tuple(None if t.grad is None else t.grad.numpy() for t in ts)


# ----------------------------------------------------------------------------- the specification
@pytest.mark.parametrize('N,D,T,hard', ALL_FLOAT + [(1, 8, 0.2, False), (2, 3, 1.0, True)])
def test_spec_equals_fp64_autograd(N, D, T, hard):
    xs = mr.float_inputs(N, D, hard=hard)
    ref = mr.mocov3(*xs, 1.0 / T, w=2.0 * T)
    loss, dq1, dq2, dk1, dk2 = autograd(xs, T)
    assert abs(ref['loss'] - loss) <= 1e-12 * max(abs(loss), 1.0)
    if N > 1:
        assert rel(ref['dq'][0], dq1) <= 1e-12 and rel(ref['dq'][1], dq2) <= 1e-12
    else:
        assert np.abs(ref['dq'][0]).max() <= 1e-15 and np.abs(dq1).max() <= 1e-15 and ref['loss'] == 0.0
    # the teacher is detached: the specification has no dk at all, and through detached keys autograd agrees
    det = autograd(xs, T, lambda q1, q2, k1, k2, T_: mr.torch_chain(q1, q2, k1.detach(), k2.detach(), T_))
    assert det[3] is None and det[4] is None and np.array_equal(det[1], dq1)
    assert set(ref) == {'s', 'lse', 'sp', 'l', 'rank', 'P', 'dq', 'loss'}
    for d in range(2):
        assert np.array_equal(ref['rank'][d], mr.rank_by_sort(ref['s'][d]))
        assert np.allclose(ref['P'][d].sum(axis=1), 1.0, atol=1e-12)
    assert abs(ref['loss'] - 2.0 * T * (ref['l'][0] + ref['l'][1])) <= 1e-12


def test_weight_and_gradient_scale():
    assert mr.weight(5.0) == float(np.float32(0.4)) and mr.weight(16.0) == 0.125
    xs = mr.float_inputs(5, 8)
    a, b = mr.mocov3(*xs, 5.0), mr.mocov3(*xs, 5.0, g=3.0)
    assert rel(b['dq'][0], 3.0 * a['dq'][0]) <= 1e-15 and b['loss'] == a['loss']


# ----------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize('N,D', mr.EXACT_CASES)
def test_exact_inputs_are_what_they_claim(N, D):
    xs = mr.exact_inputs(N, D)
    for x in xs:
        assert x.dtype == np.float32 and np.abs(x).max() <= 1.0 and np.array_equal(x * 8, np.round(x * 8))
    ref = mr.mocov3(*xs, mr.EXACT_INV_T)
    for d, (q, k) in enumerate(((xs[0], xs[3]), (xs[1], xs[2]))):
        s = ref['s'][d]
        assert np.array_equal(s * 4, np.round(s * 4)) and np.abs(s).max() <= 4096
        # the same number in fp32 under another order of summation (reversed features, fp32 accumulation)
        s32 = np.zeros((N, N), dtype=np.float32)
        for e in range(D - 1, -1, -1):
            s32 += np.outer(q[:, e], k[:, e])
        assert np.array_equal((s32 * np.float32(mr.EXACT_INV_T)).astype(np.float64), s)
        assert s[0, 0] == 16.0 * D
        if D >= 8:                                                       # without the max subtraction exp overflows fp32
            assert s[0, 0] > 88.0 and not np.isfinite(np.exp(np.float32(s[0, 0])))
        if N >= 2:                                                       # a tie with the positive, counted by `>=`
            assert s[1, 0] == s[1, 1] and ref['rank'][d][1] >= 1
            if D >= 3:
                assert not np.array_equal(k[0], k[1])
        if N >= 5:                                                       # a column that beats the positive
            assert s[2, 3] > s[2, 2] and ref['rank'][d][2] >= 1
        if N >= 2:
            assert np.abs(ref['dq'][d]).max() > 1e-3                     # a gradient worth comparing
    if N == 1:
        assert ref['loss'] == 0.0 and np.array_equal(ref['lse'][0], ref['sp'][0])


def test_the_cases_straddle_every_edge():
    assert mr.EXACT_CASES == [(1, 8), (2, 8), (5, 32), (32, 128), (33, 128), (64, 256), (97, 256), (33, 130), (4, 1)]
    assert [mr.mocov3_path(N, D)[0] for N, D in mr.EXACT_CASES] == mr.EXACT_PATHS
    assert mr.FLOAT_CASES == [(5, 32), (33, 128), (100, 256), (257, 256)] and mr.FLOAT_TS == (0.2, 0.5)
    assert mr.HARD_CASES == [(33, 256, 'fast'), (40, 130, 'generic')] and mr.HARD_T == 0.5
    assert all(mr.mocov3_path(N, D)[0] == 'fast' for N, D in mr.FLOAT_CASES)
    assert [mr.mocov3_path(N, D)[0] for N, D, _ in mr.HARD_CASES] == [p for _, _, p in mr.HARD_CASES]
    # more than one split and more than one tile per wave appear
    assert mr.mocov3_path(257, 256)[2] > 1 and mr.mocov3_path(33, 130)[2] > 1


@pytest.mark.parametrize('N,D,T,hard', ALL_FLOAT)
def test_float_inputs_and_the_room_under_the_bar(N, D, T, hard):
    """What the inputs claim; how far the unfused fp32 torch chain sits from fp64 (the bar must leave about 10x room: the worst
    case, dq at T = 0.2, leaves 8x); and the
    GPU rank check's condition on the reference alone."""
    xs = mr.float_inputs(N, D, hard=hard)
    q1, q2, k1, k2 = (x.astype(np.float64) for x in xs)
    norm = lambda x: np.linalg.norm(x, axis=1)           # noqa: E731
    cos = (q1 * k2).sum(axis=1) / (norm(q1) * norm(k2))
    assert 0.85 < np.median(cos) < 0.95
    if hard:
        for x in (q1, q2, k1, k2):
            assert norm(x).max() / norm(x).min() > 3.0
        assert np.array_equal(xs[0][0], xs[3][0]) and np.array_equal(xs[1][0], xs[2][0])
        base = q1 / norm(q1)[:, None]
        assert np.median(base @ base.T) > 0.5                            # rows share a direction
        assert np.abs(mr.mocov3(*xs, 1.0 / T)['s'][0]).max() < 10.0
    else:
        for x in (q1, q2, k1, k2):
            assert np.abs(norm(x) - 1.0).max() < 1e-6
    ref = mr.mocov3(*xs, np.float32(1.0 / T))
    # the fp32 torch chain on the CPU against fp64
    t32 = [torch.from_numpy(x).requires_grad_(True) for x in xs]
    loss32 = mr.torch_chain(*t32, T)
    loss32.backward()
    e_loss = abs(float(loss32) - ref['loss']) / abs(ref['loss'])
    e_dq = max(rel(t32[0].grad.numpy(), ref['dq'][0]), rel(t32[1].grad.numpy(), ref['dq'][1]))
    print('MEASURED mocov3 cpu chain N=%d D=%d T=%g hard=%d: rel_err loss %.3e dq %.3e' % (N, D, T, hard, e_loss, e_dq))
    assert e_loss <= BAR / ROOM and e_dq <= BAR / ROOM
    for d in range(2):
        clear = mr.clear_rows(ref['s'][d])
        assert clear.sum() >= (N + 1) // 2


# ----------------------------------------------------------------------------- what the GPU bar must tell apart
def _ce(s):
    m = s.max(axis=1)
    return float((m + np.log(np.exp(s - m[:, None]).sum(axis=1)) - np.diagonal(s)).mean())


def _variant(xs, inv_T, kind):
    """-> (loss, dq1) of a wrong implementation, fp64."""
    q1, q2, k1, k2 = (np.asarray(x, dtype=np.float64) for x in xs)
    N = q1.shape[0]
    w = mr.weight(inv_T)
    right = mr.mocov3(*xs, inv_T)
    s, P, lse = right['s'][0], right['P'][0], right['lse'][0]
    coef = w * inv_T / N
    if kind == 'diagonal_masked':                # the NT-Xent habit: the positive outside the softmax
        off = ~np.eye(N, dtype=bool)
        out = []
        for q, k in ((q1, k2), (q2, k1)):
            sd = (q @ k.T) * inv_T
            sm = np.where(off, sd, -np.inf)
            m = sm.max(axis=1)
            l_ = m + np.log(np.exp(sm - m[:, None]).sum(axis=1))
            out.append((float((l_ - np.diagonal(sd)).mean()), np.where(off, np.exp(sm - l_[:, None]), 0.0)))
        return w * (out[0][0] + out[1][0]), coef * (out[0][1] @ k2 - k2)
    if kind == 'pt_term':                        # gradient into keys / symmetrised
        return right['loss'], coef * ((P + P.T) @ k2 - 2 * k2)
    if kind == 'same_view':                      # q1 paired with k1
        r = mr.mocov3(xs[0], xs[1], xs[3], xs[2], inv_T)
        return r['loss'], r['dq'][0]
    if kind == 'no_2T':
        return right['loss'] / w, right['dq'][0] / w
    if kind == 'over_2N':
        return right['loss'] / 2, right['dq'][0] / 2
    if kind == 'softmax_over_rows':              # softmax over the rows of s^T
        st = s.T
        lt = _ce(st)
        Pt = np.exp(st - (st.max(axis=1) + np.log(np.exp(st - st.max(axis=1)[:, None]).sum(axis=1)))[:, None])
        return w * (lt + _ce(right['s'][1].T)), coef * (Pt.T @ k2 - k2)
    raise KeyError(kind)


@pytest.mark.parametrize('kind', ['diagonal_masked', 'pt_term', 'same_view', 'no_2T', 'over_2N', 'softmax_over_rows'])
@pytest.mark.parametrize('N,D,_path', mr.HARD_CASES)
def test_wrong_variants_miss_by_100_bars(N, D, _path, kind):
    xs = mr.float_inputs(N, D, hard=True)
    # at HARD_T = 0.5 the factor 2 T is 1 and dropping it shows nothing: that variant is held against T = 0.2, the other
    # temperature of the GPU tests
    inv_T = 1.0 / (mr.FLOAT_TS[0] if kind == 'no_2T' else mr.HARD_T)
    right = mr.mocov3(*xs, inv_T)
    loss, dq1 = _variant(xs, inv_T, kind)
    moved = max(abs(loss - right['loss']) / abs(right['loss']), rel(dq1, right['dq'][0]))
    assert moved >= 100 * BAR, (kind, moved)


# ----------------------------------------------------------------------------- dispatch
def test_dispatch_rule_at_every_edge():
    assert mr.FAST_MAX_D == 256
    for D, want in ((4, 'fast'), (128, 'fast'), (132, 'fast'), (252, 'fast'), (256, 'fast'), (260, 'generic'), (512, 'generic'),
                    (255, 'generic'), (254, 'generic'), (130, 'generic'), (1, 'generic'), (3, 'generic')):
        assert mr.mocov3_path(64, D)[0] == want, D
        assert mr.mocov3_path(64, D, aligned=False)[0] == 'generic'
    assert mr.mocov3_path(64, 256) == ('fast', 4, 1) and mr.mocov3_path(64, 260) == ('generic', 1, 2)
    assert mr.mocov3_path(1, 8) == ('fast', 4, 1) and mr.mocov3_path(257, 256) == ('fast', 4, 3)
    assert mr.mocov3_path(4096, 256) == ('fast', 4, 2) and mr.mocov3_path(65536, 256) == ('fast', 4, 1)
    assert mr.mocov3_path(4096, 256, aligned=False) == ('generic', 1, 2)


def test_dispatch_rule_is_the_librarys(pkg):
    import ctypes as C
    lib = pkg._hip.lib
    for N in (1, 2, 31, 32, 33, 257, 1024, 4096, 65536):
        for D in (1, 4, 128, 130, 132, 256, 257, 260, 1024):
            if N * D >= 2 ** 31:
                continue
            for al in (0, 1):
                w, s = C.c_int32(-1), C.c_int32(-1)
                rc = lib.gca_mocov3_path(N, D, al, C.addressof(w), C.addressof(s))
                assert (('generic', 'fast')[rc], w.value, s.value) == mr.mocov3_path(N, D, bool(al)), (N, D, al)
            assert lib.gca_mocov3_ws_bytes(N, D) > 0
    for N, D in ((0, 8), (-1, 8), (65537, 8), (8, 0), (65536, 32768)):
        assert lib.gca_mocov3_path(N, D, 1, None, None) == -1 and lib.gca_mocov3_ws_bytes(N, D) == -1


# ----------------------------------------------------------------------------- the host layers
def test_ops_refuse_before_any_device_is_touched(pkg):
    ops = pkg.engine.ops
    z = torch.zeros(4, 8)
    for args in ((z, z, z, torch.zeros(3, 8)), (z, z, torch.zeros(4, 9), z), (z.double(), z, z, z), (z[0], z[0], z[0], z[0]),
                 tuple(torch.zeros(0, 8) for _ in range(4)), tuple(torch.zeros(65537, 1) for _ in range(4))):
        with pytest.raises(ValueError, match='mocov3_fwd'):
            ops.mocov3_fwd(*args, 5.0)
    for bad in (0.0, -1.0, float('nan'), float('inf'), 1e39):
        with pytest.raises(ValueError, match='mocov3_fwd'):
            ops.mocov3_fwd(z, z, z, z, bad)
        with pytest.raises(ValueError, match='mocov3_fwd'):
            ops.mocov3_fwd(z, z, z, z, 5.0, w=bad)
        with pytest.raises(ValueError, match='mocov3_bwd'):
            ops.mocov3_bwd(z, z, z, z, torch.zeros(8), bad)
    with pytest.raises(ValueError, match='lse'):
        ops.mocov3_bwd(z, z, z, z, torch.zeros(4), 5.0)
    for gs in (float('inf'), float('nan'), 1e39):
        with pytest.raises(ValueError, match='gscale_host'):
            ops.mocov3_bwd(z, z, z, z, torch.zeros(8), 5.0, gscale_host=gs)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.mocov3_fwd(z, z, z, z, 5.0)
    assert ops.mocov3_weight(5.0) == mr.weight(5.0)


def test_factories(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    MoCoV3Loss = importlib.import_module(pkg.__name__ + '.lib.memory.mocov3').MoCoV3Loss
    build = importlib.import_module(pkg.__name__ + '.lib.modeling.build')
    gw = importlib.import_module(pkg.__name__ + '.lib.modeling.graph_wrappers')
    assert pkg.get_defaults().CONTRAST.V3_HID == 4096 and hasattr(pkg, 'MoCoV3Trainer')
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'mocov3', 32, 16, 8)
    cfg.CONTRAST.NCE_T = 0.2
    cfg.CONTRAST.V3_HID = 48
    c = pkg.create_contrast(cfg, 100)
    assert isinstance(c, MoCoV3Loss) and c.T == 0.2 and c.rank is None and c.l12 is None and c.l21 is None
    assert list(c.state_dict()) == [] and MoCoV3Loss().T == 0.2
    for bad in (0.0, -0.2, float('nan'), float('inf'), 1e-39):
        with pytest.raises(ValueError, match='MoCoV3Loss'):
            MoCoV3Loss(bad)
        badcfg = parity.make_cfg(pkg, 'R2P1D10T', 'mocov3', 32, 16, 8)
        badcfg.CONTRAST.NCE_T = bad
        with pytest.raises(ValueError):
            pkg.create_contrast(badcfg, 100)
    z = torch.zeros(4, 8)
    for args in ((z, torch.zeros(4, 9), z, z), (z, z, torch.zeros(5, 8), z), (z, z, z, torch.zeros(4, 7)), (z[0], z[0], z[0], z[0])):
        with pytest.raises(ValueError, match='MoCoV3Loss'):
            c(*args)
    # the model factory: a student with a predictor and a teacher without, whose parameters are the student's leading ones
    torch.manual_seed(5)
    model, ema = build.create_visual_model(cfg)
    assert isinstance(model.model, gw.MoCoV3) and isinstance(ema.model, gw.MoCoV3) and ema.model.encoder is not model.model.encoder
    assert [n for n, _ in model.model.named_children()] == ['encoder', 'projection', 'prediction']
    assert [n for n, _ in ema.model.named_children()] == ['encoder', 'projection']
    sk, tk = list(model.state_dict()), list(ema.state_dict())
    assert not any('.prediction.' in k for k in tk) and any('.prediction.' in k for k in sk)
    assert [k for k in sk if '.prediction.' not in k] == tk
    assert all(k.startswith(('model.encoder.', 'model.projection.', 'model.prediction.')) for k in sk)
    sp, tp = [(n, tuple(p.shape)) for n, p in model.named_parameters()], [(n, tuple(p.shape)) for n, p in ema.named_parameters()]
    assert sp[:len(tp)] == tp and all('.prediction.' in n for n, _ in sp[len(tp):]) and len(sp) == len(tp) + 6
    st = model.state_dict()
    assert tuple(st['model.projection.l1.0.weight'].shape) == (48, model.model.feature_dim)
    assert tuple(st['model.projection.l3.0.weight'].shape) == (32, 48)
    assert tuple(st['model.prediction.l1.0.weight'].shape) == (48, 32) and tuple(st['model.prediction.l2.weight'].shape) == (32, 48)
    # SimSiam's names: a SimSiam wrapper of the same widths loads the student's state
    simsiam_keys = set(gw.SimSiam(build._encoder(cfg), 32).state_dict())
    assert {k[len('model.'):] for k in sk} == simsiam_keys
    for bad in (dict(out_dim=0), dict(hid_dim=0), dict(out_dim=2.5), dict(hid_dim=True)):
        with pytest.raises(ValueError, match='MoCoV3'):
            gw.MoCoV3(model.model.encoder, **{**dict(out_dim=32, hid_dim=48), **bad})
    for mem in ('simsiam', 'simclr', 'barlow', 'vicreg', 'swav'):
        assert build.create_visual_model(parity.make_cfg(pkg, 'R2P1D10T', mem, 32, 16, 8))[1] is None


def test_trainer_refusals_without_a_device(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    for mem in ('simsiam', 'moco', 'simclr', 'dino'):
        with pytest.raises(ValueError, match='mocov3'):
            pkg.MoCoV3Trainer(parity.make_cfg(pkg, 'R2P1D10T', mem, 32, 16, 8), 'cpu')
    with pytest.raises(NotImplementedError, match='one GPU'):
        pkg.MoCoV3Trainer(parity.make_cfg(pkg, 'R2P1D10T', 'mocov3', 32, 16, 8), 'cpu', ctx=pkg.parallel.DistCtx(force_active=True))
