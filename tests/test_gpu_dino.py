"""gca_dino_fwd / gca_ema_update_dev, ops.dino_* / ema_update_dev, lib.memory.dino.DINOLoss, the DINO wrapper and DINOTrainer on
the device, against tests/dino_ref.py (fp64 numpy) and tests/dino_model.py (the fp64 torch oracle of student and teacher).

Kernel parity: parts (loss, l12, l21, ent), probs, the new centre, dz1, dz2, dC against the specification fed the same fp32
inputs, each array's max-norm error relative to its largest reference entry; loss, l12 and l21 each relative to itself; ent on
the scale of its range, log K (where the teacher is nearly one-hot the entropy is a residue of size K exp(-2 / Tt) that no
relative error measures).  The bar is dino_ref.BAR: the next power of ten above 4 x the worst error measured on these cases,
and no more than 1e-4 -- the largest exponent argument is about 2.1 / Tt, 50 to 100, whose fp32 rounding is a few 1e-6.  Every
wrong variant of tests/test_dino_ref.py misses by more than 100 bars.

Measured on an MI355X (printed as `MEASURED dino ...`), worst over the cases:
MEASURED dino unit rows      loss 5.96e-7   l12 5.97e-7 (3 x 5 x 7)   l21 9.60e-7 (2 x 8 x 65536)   ent 3.87e-7 (2 x 1 x 2)   probs 1.91e-6
                             (4096 x 16 x 64)   centre 8.45e-8   dz1 1.64e-6 (4 x 16 x 16384)   dz2 1.27e-6   dC 1.21e-6 (3 x 5 x 7); with Ts 0.5, Tt 0.02:
                             dz1 2.45e-6 (65 x 128 x 3000), the worst of all, probs 2.10e-6; with Ts 0.1, Tt 0.07: 9.76e-7
MEASURED dino wave per row   the same figures to two digits (1.21e-6 / 1.07e-6 / 1.05e-6 at its three shapes)
MEASURED dino adversarial    every score equal: ent 1.10e-6 of log K, loss 1.19e-6 of log K, probs 1.35e-6 of 1 / K, gradients 4.89e-7 of
                             1 / (2 N Ts); one prototype at +1 and the rest at -1, Tt 0.04: probs down to 1.9e-22, ent 6e-25 of log K,
                             dz 6.16e-7 of 1 / (2 N Ts), dC 6.16e-7 of 1 / Ts, nothing non-finite, no zero probability
MEASURED dino pointers offset by 4 bytes (33 x 130 x 65): 1.07e-6      replay at a rewritten Tt 0.07 (65 x 128 x 3000): 1.13e-6   [bar 1e-5]
MEASURED dino model          loss against the fp64 oracle: 8.60e-7 relative (l12 7.41e-7, l21 8.96e-7, ent 5.40e-6, centre 1.68e-7)  [bar 1e-3]
                             parameter gradients: median 5.68e-6, 95th percentile 1.07e-5, worst 1.19e-5 over 68 tensors; prototypes 1.22e-6
MEASURED dino trainer        loss on one repeated batch, SGD lr 3e-4: 2.532916 2.033290 1.860677 against the oracle's 2.532918 2.033317
                             1.860730 (7.9e-7, 1.3e-5, 2.8e-5 relative); centre 5.95e-6, teacher prototypes 1.21e-7                 [bar 1e-3]
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dino_ref as dr                    # noqa: E402
import dino_model as dm                  # noqa: E402
from parity import check_grad_errors, make_cfg, register_tiny, rel           # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = -1
BAR = dr.BAR
DEFAULT = (dr.DEFAULTS['Ts'], dr.DEFAULTS['Tt'], dr.DEFAULTS['cm'])
ARRAYS = ('probs', 'center', 'dz1', 'dz2', 'dC')
_REF = {}


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def f32(v):
    return float(np.float32(v))


def unit_ref(N, D, K, params=DEFAULT, seed=0):
    """The fp64 specification on the seeded unit-row inputs: computed once per case, shared, left unchanged."""
    key = (N, D, K, params, seed)
    if key not in _REF:
        inputs = dr.unit_inputs(N, D, K, seed)
        _REF[key] = (inputs, dr.forward(*inputs, *(f32(p) for p in params)))
    return _REF[key]


def run(ops, inputs, params=DEFAULT, update=True, accumulate=False, dC=None, **kw):
    """inputs: the seven device tensors (the centre is left alone: the kernels move a copy) -> (parts, probs, centre, dz1, dz2, dC)"""
    zs1, zs2, Cs, zt1, zt2, Ct, c = inputs
    Ts, Tt, cm = params
    center = c.clone()
    parts, dS, probs = ops.dino_fwd(zs1, zs2, Cs, zt1, zt2, Ct, Ts, torch.tensor([Tt], device=DEV), cm, center, update, want_probs=True)
    dC = torch.empty_like(Cs) if dC is None else dC
    dz1, dz2 = ops.dino_bwd(zs1, zs2, Cs, dS, dC, accumulate, **kw)
    return parts, probs, center, dz1, dz2, dC


def errors(got, ref, K):
    """max-norm errors of (parts, probs, centre, dz1, dz2, dC) on the device, each relative to its largest reference entry"""
    parts = got[0].cpu().numpy().astype(np.float64)
    e = {k: abs(parts[i] - ref[k]) / abs(ref[k]) for i, k in enumerate(('loss', 'l12', 'l21'))}
    e['ent'] = abs(parts[3] - ref['ent']) / math.log(K)
    for k, t in zip(ARRAYS, got[1:]):
        e[k] = rel(t, torch.from_numpy(np.ascontiguousarray(ref[k])))
    return e


def show(what, e):
    print('MEASURED dino %s: rel_err %s  worst %.2e' % (what, ' '.join('%s %.2e' % kv for kv in e.items()), max(e.values())))


# ----------------------------------------------------------------------------- 1. the kernels against the specification
@pytest.mark.parametrize('N,D,K', dr.KERNEL_CASES)
def test_kernel_parity(pkg, N, D, K):
    assert pkg._hip.lib.gca_dino_ws_bytes(N, D, K) == dr.ws_bytes(N, D, K)
    inputs, ref = unit_ref(N, D, K)
    got = run(pkg.engine.ops, [dev(a) for a in inputs])
    torch.cuda.synchronize()
    e = errors(got, ref, K)
    show('unit rows N=%d D=%d K=%d' % (N, D, K), e)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert max(e.values()) <= BAR, e
    assert float((got[1].sum(dim=2) - 1.0).abs().max()) <= 1e-5               # every row of the teacher's probabilities sums to 1


@pytest.mark.parametrize('Ts,Tt', dr.TEMPERATURES)
@pytest.mark.parametrize('N,D,K', dr.TEMPERATURE_CASES)
def test_temperatures(pkg, N, D, K, Ts, Tt):
    params = (Ts, Tt, 0.9)
    inputs, ref = unit_ref(N, D, K, params)
    got = run(pkg.engine.ops, [dev(a) for a in inputs], params)
    torch.cuda.synchronize()
    e = errors(got, ref, K)
    show('unit rows N=%d D=%d K=%d Ts=%g Tt=%g' % (N, D, K, Ts, Tt), e)
    assert max(e.values()) <= BAR, e


@pytest.mark.parametrize('N,D,K', [(3, 5, 7), (33, 130, 65), (65, 128, 3000)])
def test_wave_per_row_grid(pkg, N, D, K):
    """gca_dino_fwd_grid's other row grid, one wave per row and direction (4 rows to a workgroup: N below, off and above a
    multiple of 4): the same bar, reproducible on its own, and row_grid 0 is gca_dino_fwd bit for bit."""
    ops = pkg.engine.ops
    inputs, ref = unit_ref(N, D, K)
    d = [dev(a) for a in inputs]

    def fwd(grid):
        center = d[6].clone()
        parts, dS, probs = ops.dino_fwd(*d[:6], DEFAULT[0], torch.tensor([DEFAULT[1]], device=DEV), DEFAULT[2], center, True,
                                        want_probs=True, row_grid=grid)
        dC = torch.empty_like(d[2])
        return (parts, probs, center) + ops.dino_bwd(d[0], d[1], d[2], dS, dC, False) + (dC,)

    wave, again, wg, plain = fwd(1), fwd(1), fwd(0), fwd(None)
    torch.cuda.synchronize()
    e = errors(wave, ref, K)
    show('wave per row N=%d D=%d K=%d' % (N, D, K), e)
    assert max(e.values()) <= BAR, e
    for x, y in zip(wave, again):
        assert torch.equal(bits(x), bits(y))
    for x, y in zip(wg, plain):
        assert torch.equal(bits(x), bits(y))
    with pytest.raises(ValueError):
        ops.dino_fwd(*d[:6], 0.1, torch.tensor([0.04], device=DEV), 0.9, d[6].clone(), True, row_grid=2)
    lib, p = pkg._hip.lib, pkg._hip.ptr
    sent = torch.full((4,), 7.0, device=DEV)
    ws = torch.empty(lib.gca_dino_ws_bytes(N, D, K), dtype=torch.uint8, device=DEV)
    dS = torch.empty(2, N, K, device=DEV)
    for grid in (2, -1):
        assert lib.gca_dino_fwd_grid(*(p(x) for x in d[:6]), N, D, K, 0.1, p(sent), 0.9, p(d[6].clone()), 1, p(sent), p(dS), None, grid,
                                     p(ws), pkg._hip.stream()) == EINVAL
    torch.cuda.synchronize()
    assert float(sent.min()) == 7.0 == float(sent.max())


@pytest.mark.parametrize('make', [dr.equal_scores_inputs, dr.one_hot_scores_inputs], ids=['equal', 'one_hot'])
@pytest.mark.parametrize('N,D,K', dr.ADVERSARIAL_CASES)
def test_adversarial_scores(pkg, N, D, K, make):
    """Every score equal: uniform probabilities, ent = loss = log K.  One prototype at +1 and the rest at -1 at Tt = 0.04: the
    probabilities go down to exp(-50), nothing may turn non-finite or underflow to zero, the entropy stays finite.  In both the
    gradient is a residue -- softmax - p is 1 / K - 1 / K, or (1 - K e^-20) - 1 -- with no scale of its own, so it is held to
    the bar of the size it would have had with entries of dS of their full size 1 / (2 N Ts): a row of dS, whose entries sum to
    0, has an L1 norm of at most 2 / (2 N Ts) and C has unit rows, so dz is held to 1 / (2 N Ts); a column of dS over the 2 N
    rows has an L1 norm of up to 2 N / (2 N Ts), so dC is held to 1 / Ts (here every row is the same, and the 2 N roundings
    of 1 - K e^-20 do add up).  The one-hot loss, about K e^-20, is held likewise to the size of its terms, 2 / Ts."""
    params = (0.1, 0.04, 0.9)
    inputs = make(N, D, K)
    ref = dr.forward(*inputs, *(f32(p) for p in params))
    got = run(pkg.engine.ops, [dev(a) for a in inputs], params)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert float(got[1].min()) > 0.0
    e = errors(got, ref, K)
    scale = 1.0 / (2.0 * N * params[0])
    for k in ('dz1', 'dz2', 'dC'):
        e[k] = float((got[ARRAYS.index(k) + 1].double().cpu() - torch.from_numpy(ref[k])).abs().max()) / (scale * (2 * N if k == 'dC' else 1))
    parts = got[0].double().cpu().numpy()
    if make is dr.equal_scores_inputs:
        assert abs(parts[3] - math.log(K)) <= BAR * math.log(K) and float((got[1] * K - 1.0).abs().max()) <= 1e-4
    else:
        for i, k in enumerate(('loss', 'l12', 'l21')):
            e[k] = abs(parts[i] - ref[k]) / (2.0 / params[0])
        assert 0.0 <= parts[3] < 1e-12 and float(got[1][:, :, 1:].max()) < 1e-21
    show('%s N=%d D=%d K=%d' % (make.__name__, N, D, K), e)
    assert max(e.values()) <= BAR, e


@pytest.mark.parametrize('N,D,K', [(33, 130, 65), (65, 128, 3000)])
def test_centre_is_left_bitwise_alone_without_update(pkg, N, D, K):
    inputs, ref = unit_ref(N, D, K)
    d = [dev(a) for a in inputs]
    kept = run(pkg.engine.ops, d, update=False)
    moved = run(pkg.engine.ops, d, update=True)
    torch.cuda.synchronize()
    assert torch.equal(bits(kept[2]), bits(d[6])) and not torch.equal(bits(moved[2]), bits(d[6]))
    for x, y in zip(kept[:2] + kept[3:], moved[:2] + moved[3:]):                # everything else does not depend on the flag
        assert torch.equal(bits(x), bits(y))


def test_pointers_offset_by_four_bytes(pkg):
    """Nothing assumes 16-byte alignment: inputs, centre, temperature, saved state, workspace and outputs all start 4 bytes
    into their buffers."""
    N, D, K = 33, 130, 65
    inputs, ref = unit_ref(N, D, K)
    lib, H = pkg._hip.lib, pkg._hip

    def off(shape, src=None):
        n = int(np.prod(shape))
        buf = torch.zeros(n + 1, device=DEV)
        v = buf[1:].view(*shape)
        if src is not None:
            v.copy_(dev(src))
        assert v.data_ptr() % 8 == 4
        return v

    shapes = [(N, D), (N, D), (K, D), (N, D), (N, D), (K, D), (K,)]
    t = [off(s, a) for s, a in zip(shapes, inputs)]
    tt = off((1,), np.float32([DEFAULT[1]]))
    parts, dS, probs, dz1, dz2, dC = off((4,)), off((2, N, K)), off((2, N, K)), off((N, D)), off((N, D)), off((K, D))
    ws = torch.empty(max(lib.gca_dino_ws_bytes(N, D, K), lib.gca_swav_ws_bytes(N, D, K)) + 4, dtype=torch.uint8, device=DEV)
    p = H.ptr
    assert lib.gca_dino_fwd(*(p(x) for x in t[:6]), N, D, K, DEFAULT[0], p(tt), DEFAULT[2], p(t[6]), 1, p(parts), p(dS), p(probs),
                            p(ws) + 4, H.stream()) == 0
    assert lib.gca_swav_bwd(p(t[0]), p(t[1]), p(t[2]), p(dS), N, D, K, None, 1.0, p(dz1), p(dz2), p(dC), 0, p(ws) + 4, H.stream()) == 0
    torch.cuda.synchronize()
    e = errors((parts, probs, t[6], dz1, dz2, dC), ref, K)
    show('offset pointers N=%d D=%d K=%d' % (N, D, K), e)
    assert max(e.values()) <= BAR, e


@pytest.mark.parametrize('N,D,K', [(33, 130, 65), (65, 128, 3000)])
def test_accumulate_dC(pkg, N, D, K):
    ops = pkg.engine.ops
    inputs, ref = unit_ref(N, D, K)
    d = [dev(a) for a in inputs]
    base = torch.from_numpy(np.random.RandomState(3).randn(K, D).astype(np.float32)).to(DEV) * float(np.abs(ref['dC']).max())
    fresh = run(ops, d, dC=torch.full((K, D), float('nan'), device=DEV))[5]
    added = run(ops, d, accumulate=True, dC=base.clone())[5]
    torch.cuda.synchronize()
    assert rel(fresh, torch.from_numpy(ref['dC'])) <= BAR                       # accumulate False overwrites, NaNs included
    assert torch.equal(bits(added), bits(base + fresh))                         # accumulate True adds exactly one rounding


def test_gradient_scale(pkg):
    ops = pkg.engine.ops
    N, D, K = 33, 130, 65
    d = [dev(t) for t in dr.unit_inputs(N, D, K, seed=5)]
    one = run(ops, d)[3:]
    scaled = run(ops, d, gscale_dev=torch.tensor([1024.0, 7.0], device=DEV))[3:]
    half = run(ops, d, gscale_host=0.5)[3:]
    both = run(ops, d, gscale_dev=torch.tensor([3.0], device=DEV), gscale_host=-0.7)[3:]
    torch.cuda.synchronize()
    for v in range(3):
        assert float(one[v].abs().max()) > 0
        assert rel(scaled[v], one[v] * 1024.0) <= 1e-6 and rel(half[v], one[v] * 0.5) <= 1e-6
        assert rel(both[v], one[v].double() * (3.0 * np.float64(np.float32(-0.7)))) <= 1e-6


@pytest.mark.parametrize('N,D,K', [(33, 130, 65), (64, 128, 128), (65, 128, 3000)])
def test_deterministic(pkg, N, D, K):
    d = [dev(t) for t in dr.unit_inputs(N, D, K, seed=3)]
    outs = [run(pkg.engine.ops, d) for _ in range(3)]
    torch.cuda.synchronize()
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert torch.equal(bits(x), bits(y))


def test_refused_arguments_touch_nothing(pkg):
    lib, H = pkg._hip.lib, pkg._hip
    N, D, K = 8, 8, 6
    t = [dev(a) for a in dr.unit_inputs(N, D, K)]
    SENT = 12345.0
    parts, dS, probs, center, pe = (torch.full((n,), SENT, device=DEV) for n in (4, 2 * N * K, 2 * N * K, K, 16))
    tt, mom = torch.tensor([0.04], device=DEV), torch.tensor([0.9], device=DEV)
    src = torch.ones(16, device=DEV)
    ws = torch.empty(max(lib.gca_dino_ws_bytes(N, D, K), 1 << 16), dtype=torch.uint8, device=DEV)
    p = H.ptr
    nan, inf = float('nan'), float('inf')

    def fwd(a=p(t[0]), b=p(t[1]), c=p(t[2]), ta=p(t[3]), tb=p(t[4]), tc=p(t[5]), N=N, D=D, K=K, Ts=0.1, ttp=p(tt), cm=0.9,
            ce=p(center), upd=1, pa=p(parts), s=p(dS), q=p(probs), w=p(ws)):
        return lib.gca_dino_fwd(a, b, c, ta, tb, tc, N, D, K, Ts, ttp, cm, ce, upd, pa, s, q, w, H.stream())

    for kw in (dict(N=1), dict(N=0), dict(N=-2), dict(N=8193), dict(D=0), dict(D=-1), dict(D=8193), dict(K=1), dict(K=0),
               dict(K=65537), dict(N=1 << 31), dict(a=None), dict(b=None), dict(c=None), dict(ta=None), dict(tb=None), dict(tc=None),
               dict(ttp=None), dict(ce=None), dict(pa=None), dict(s=None), dict(w=None), dict(Ts=0.0), dict(Ts=-0.1), dict(Ts=inf),
               dict(Ts=nan), dict(Ts=1e-39), dict(cm=1.0), dict(cm=-0.01), dict(cm=1.5), dict(cm=nan), dict(cm=inf)):
        assert fwd(**kw) == EINVAL, kw
    for args in ((None, p(src), 16, p(mom)), (p(pe), None, 16, p(mom)), (p(pe), p(src), 16, None), (p(pe), p(src), 0, p(mom)),
                 (p(pe), p(src), -4, p(mom))):
        assert lib.gca_ema_update_dev(*args, H.stream()) == EINVAL, args
    assert lib.gca_dino_ws_bytes(1, 8, 8) == -1 and lib.gca_dino_ws_bytes(8, 8193, 8) == -1 and lib.gca_dino_ws_bytes(8, 8, 1) == -1
    torch.cuda.synchronize()
    for x in (parts, dS, probs, center, pe):
        assert float(x.min()) == SENT == float(x.max())
    # and the accepted calls write all of their outputs (probs only when asked for, the centre only when asked to)
    assert fwd(q=None, upd=0) == 0
    torch.cuda.synchronize()
    assert float((dS == SENT).sum()) == 0 and float((parts == SENT).sum()) == 0
    assert float(probs.min()) == SENT == float(probs.max()) and float(center.min()) == SENT == float(center.max())
    assert fwd() == 0 and lib.gca_ema_update_dev(p(pe), p(src), 16, p(mom), H.stream()) == 0
    torch.cuda.synchronize()
    for x in (parts, dS, probs, center, pe):
        assert float((x == SENT).sum()) == 0


def test_ops_refuse_what_the_entry_refuses(pkg):
    ops = pkg.engine.ops
    z, C, c, tt = torch.zeros(4, 8, device=DEV), torch.zeros(6, 8, device=DEV), torch.zeros(6, device=DEV), torch.full((1,), 0.04, device=DEV)
    one = torch.zeros(1, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.dino_fwd(one, one, C, one, one, C, 0.1, tt, 0.9, c, True)
    with pytest.raises(ValueError):
        ops.dino_fwd(z, z, C[:1], z, z, C[:1], 0.1, tt, 0.9, c[:1], True)
    with pytest.raises(ValueError):
        ops.dino_fwd(z, z, C, z, z, torch.zeros(6, 7, device=DEV), 0.1, tt, 0.9, c, True)
    for Ts, cm in ((0.0, 0.9), (float('nan'), 0.9), (0.1, 1.0), (0.1, -0.1)):
        with pytest.raises(ValueError):
            ops.dino_fwd(z, z, C, z, z, C, Ts, tt, cm, c, True)
    with pytest.raises(ValueError):
        ops.dino_bwd(z, z, C, torch.zeros(2, 4, 7, device=DEV), torch.zeros(6, 8, device=DEV), False)
    with pytest.raises(ValueError):
        ops.ema_update_dev(torch.zeros(4, device=DEV), torch.zeros(5, device=DEV), tt)
    assert float(c.abs().max()) == 0.0


def test_capturable_and_a_replay_follows_the_rewritten_teacher_temperature(pkg):
    """Forward and backward inside one captured graph: replays track the static inputs and equal the eager bits; after the
    teacher temperature's device scalar is rewritten, a replay follows the specification at the new temperature."""
    ops = pkg.engine.ops
    N, D, K = 65, 128, 3000
    inputs, ref = unit_ref(N, D, K)
    s = [dev(a).clone() for a in inputs]
    center, tt = s[6].clone(), torch.tensor([DEFAULT[1]], device=DEV)

    def step():
        parts, dS, probs = ops.dino_fwd(*s[:6], DEFAULT[0], tt, DEFAULT[2], center, True, want_probs=True)
        dC = torch.empty_like(s[2])
        dz1, dz2 = ops.dino_bwd(s[0], s[1], s[2], dS, dC, False)
        return parts, probs, center, dz1, dz2, dC

    eager = [x.clone() for x in step()]
    torch.cuda.synchronize()
    center.copy_(s[6])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = step()
    center.copy_(s[6])
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, captured):
        assert torch.equal(bits(x), bits(y))
    params = (0.1, 0.07, 0.9)
    new = dr.unit_inputs(N, D, K, seed=9)
    for dst, a in zip(s, new):
        dst.copy_(dev(a))
    center.copy_(s[6])
    tt.fill_(params[1])
    g.replay()
    torch.cuda.synchronize()
    want = dr.forward(*new, *(f32(p) for p in params))
    e = errors(captured, want, K)
    show('replay at Tt=0.07 N=%d D=%d K=%d' % (N, D, K), e)
    assert max(e.values()) <= BAR, e
    stale = dr.forward(*new, f32(0.1), f32(DEFAULT[1]), f32(0.9))                # the captured temperature would have missed
    assert abs(stale['loss'] - want['loss']) > 100 * BAR * want['loss']
    g.reset()


@pytest.mark.parametrize('n', [1, 255, 257, 3000001])
def test_ema_update_dev_equals_ema_update_bit_for_bit(pkg, n):
    """gca_ema_update takes whole float4s only, so it runs on the buffers padded to a multiple of four; gca_ema_update_dev on
    the n elements, once on 16-byte-aligned pointers (float4 body, scalar tail) and once 4 bytes off (all scalar)."""
    ops = pkg.engine.ops
    gen = torch.Generator().manual_seed(n)
    n4 = (n + 3) // 4 * 4
    pe0, p0 = torch.randn(n4, generator=gen).to(DEV), torch.randn(n4, generator=gen).to(DEV)
    for m in (0.999, 0.9, 0.0, 1.0):
        want = pe0.clone()
        ops.ema_update(want, p0, m)
        md = torch.tensor([m], device=DEV)
        got = pe0.clone()
        ops.ema_update_dev(got[:n], p0[:n], md)
        buf = torch.full((n + 2,), 777.0, device=DEV)
        src = torch.zeros(n + 1, device=DEV)
        buf[1:1 + n].copy_(pe0[:n])
        src[1:].copy_(p0[:n])
        assert buf[1:].data_ptr() % 8 == 4
        ops.ema_update_dev(buf[1:1 + n], src[1:], md)
        torch.cuda.synchronize()
        assert torch.equal(bits(got[:n]), bits(want[:n])) and torch.equal(bits(got[n:]), bits(pe0[n:])), m
        assert torch.equal(bits(buf[1:1 + n]), bits(want[:n])) and float(buf[0]) == 777.0 == float(buf[-1]), m
    ref = dr.ema(pe0[:n].double().cpu().numpy(), p0[:n].double().cpu().numpy(), f32(0.999))
    ops.ema_update_dev(pe0[:n], p0[:n], torch.tensor([0.999], device=DEV))
    torch.cuda.synchronize()
    assert rel(pe0[:n], torch.from_numpy(ref)) <= 1e-6


# ----------------------------------------------------------------------------- 2. the module
def test_module_forward_backward(pkg):
    import importlib
    DINOLoss = importlib.import_module(pkg.__name__ + '.lib.memory.dino').DINOLoss
    N, D, K = 33, 130, 65
    inputs, _ = unit_ref(N, D, K)
    ref = dr.forward(*inputs, *(f32(p) for p in DEFAULT), g=3.0)
    t = [dev(a) for a in inputs]
    for a in t[:3]:
        a.requires_grad_(True)
    crit = DINOLoss(K, *DEFAULT).to(DEV)
    crit.center.copy_(t[6])
    loss = crit(*t[:6])
    assert loss.dim() == 0 and abs(float(loss.detach()) - ref['loss']) <= BAR * abs(ref['loss'])
    (loss * 3.0).backward()
    torch.cuda.synchronize()
    for a, k in ((t[0], 'dz1'), (t[1], 'dz2'), (t[2], 'dC')):
        assert rel(a.grad, torch.from_numpy(ref[k])) <= BAR, k
    for got, k in ((crit.l12, 'l12'), (crit.l21, 'l21'), (crit.ent, 'ent')):
        assert got.is_cuda and got.dim() == 0 and abs(float(got) - ref[k]) <= BAR * max(ref[k], math.log(K) if k == 'ent' else 0.0), k
    assert rel(crit.center, torch.from_numpy(ref['center'])) <= BAR             # training mode: the centre moved
    moved = crit.center.clone()
    crit.eval()
    again = crit(*(a.detach() for a in t[:6]))
    torch.cuda.synchronize()
    assert torch.equal(bits(crit.center), bits(moved))                          # eval mode: it stays
    want = dr.forward(*inputs[:6], moved.cpu().numpy(), *(f32(p) for p in DEFAULT))
    assert abs(float(again) - want['loss']) <= BAR * want['loss']
    crit.set_teacher_temp(0.07)                                                 # the device scalar follows
    third = crit(*(a.detach() for a in t[:6]))
    want = dr.forward(*inputs[:6], moved.cpu().numpy(), f32(0.1), f32(0.07), f32(0.9))
    assert abs(float(third) - want['loss']) <= BAR * want['loss']


# ----------------------------------------------------------------------------- 3. model and trainer
CLIP = (8, 6, 8, 48, 48)
PROTOS = 24
ALPHA = 0.9              # a teacher momentum at which three steps move the teacher's prototypes visibly


def clips(seed, n=4):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*CLIP, generator=gen).to(DEV) for _ in range(n)]


def dino_cfg(pkg, **solver):
    register_tiny(pkg)
    cfg = make_cfg(pkg, 'R2P1D10T', 'dino', 32, 16, 8, **solver)
    cfg.CONTRAST.DINO_K = PROTOS
    cfg.CONTRAST.ALPHA = ALPHA
    return cfg


def cpu_state(module):
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def test_model_against_the_fp64_oracle(pkg):
    import importlib
    DINOLoss = importlib.import_module(pkg.__name__ + '.lib.memory.dino').DINOLoss
    tr = pkg.DINOTrainer(dino_cfg(pkg), DEV, use_graph=False, seed=21)
    with torch.no_grad():                                                       # a teacher that differs from its student
        gen = torch.Generator().manual_seed(5)
        tr.arena_t.flat.mul_(1.0 + 0.05 * torch.randn(tr.arena_t.flat.shape, generator=gen).to(DEV))
        pkg.engine.ops.rows_normalize_(tr.model_ema.model.prototypes.weight.data)
    state, state_t = cpu_state(tr.model), cpu_state(tr.model_ema)
    assert list(state) == list(state_t) and not torch.equal(state['model.prototypes.weight'], state_t['model.prototypes.weight'])
    x = clips(31, 1)[0]
    center = 0.1 * torch.randn(PROTOS, generator=torch.Generator().manual_seed(6))
    student, teacher = dm.oracle_dino('R2P1D10T', 8, 32, PROTOS, state, state_t)
    want, l12, l21, ent, new_c = dm.model_loss(student, teacher, x.cpu().double(), center.double())
    want.backward()
    crit = DINOLoss(PROTOS, *DEFAULT).to(DEV)
    crit.center.copy_(center)
    tr.optimizer.zero_grad()
    x1, x2 = (v.contiguous() for v in torch.chunk(x, 2, dim=1))
    with torch.no_grad():
        zt1, zt2 = tr.model_ema(x1), tr.model_ema(x2)
    got = crit(tr.model(x1), tr.model(x2), tr.model.model.prototypes.weight, zt1, zt2, tr.model_ema.model.prototypes.weight)
    got.backward()
    torch.cuda.synchronize()
    got = got.detach()
    e = dict(loss=abs(float(got) - float(want)) / abs(float(want)), center=rel(crit.center, new_c))
    for k, mine, ref in (('l12', crit.l12, l12), ('l21', crit.l21, l21), ('ent', crit.ent, ent)):
        e[k] = abs(float(mine) - float(ref)) / abs(float(ref))
    print('MEASURED dino model loss %.6f vs oracle %.6f: rel err %s' % (float(got), float(want), ' '.join('%s %.3e' % kv for kv in e.items())))
    assert got.dim() == 0 and max(e.values()) < 1e-3, e
    g64 = {n: p.grad for n, p in student.named_parameters()}
    errs = {n: rel(p.grad, g64[n]) for n, p in tr.model.named_parameters() if g64[n] is not None and g64[n].abs().max() > 0}
    assert len(errs) > 40 and 'model.prototypes.weight' in errs and 'model.proj_head.head.2.weight' in errs
    med, p95, worst = check_grad_errors(errs, 'dino parameter gradients')
    print('MEASURED dino model parameter gradients: median %.2e p95 %.2e worst %.2e over %d tensors; prototypes %.2e'
          % (med, p95, worst, len(errs), errs['model.prototypes.weight']))
    assert errs['model.prototypes.weight'] < 1e-3
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in tr.model_ema.parameters())      # no gradient reaches the teacher
    tr.close()


LR = 3e-4


def test_trainer_graph_equals_eager_and_follows_the_oracle(pkg):
    """Three steps on one repeated batch: the captured run equals the eager run bit for bit, and loss, centre and the teacher's
    prototypes follow the fp64 oracle at the project's 1e-3.  The rate is chosen by the oracle's own error, as in
    tests/test_gpu_swav.py: this tiny model on 8 clips is badly conditioned over several steps -- at a rate of 0.01 the fp32 run
    of the ORACLE leaves its fp64 run by 1.1e-4 at the second loss and 2.9e-2 at the third (centre 2.2e-3, teacher prototypes
    3.8e-4); at 3e-4 by 1.3e-5 and 4.7e-5 (centre 6.2e-6, teacher prototypes 1.7e-7), a twentieth of the 1e-3 bar.  The fp64
    oracle's loss falls on this batch at this rate (checked on the CPU: 2.5329, 2.0333, 1.8607), so the product's must."""
    cfg = dino_cfg(pkg, WARMUP_FACTOR=1.0, BASE_LR=LR)
    x = clips(33, 1)[0]
    runs, finals, state = {}, {}, None
    keys = ('loss', 'l12', 'l21', 'ent')
    for use_graph in (True, False):
        tr = pkg.DINOTrainer(cfg, DEV, use_graph=use_graph, seed=7)
        if state is None:
            state = cpu_state(tr.model)
            assert all(torch.equal(v, state[k]) for k, v in cpu_state(tr.model_ema).items())       # the teacher starts as the student
        outs = []
        for _ in range(3):
            out = tr.train_step(x)
            torch.cuda.synchronize()
            assert set(out) >= set(keys)
            outs.append(tuple(out[k].detach().clone() for k in keys))
        assert (tr._segments[0].graph is not None) == use_graph
        runs[use_graph] = outs
        finals[use_graph] = (tr.contrast.center.detach().clone(), tr.model_ema.model.prototypes.weight.detach().clone(),
                             tr.model.model.prototypes.weight.detach().clone())
        sd = tr.state_dict()
        assert list(sd['contrast']) == ['center'] and list(sd['model_ema']) == list(sd['state_dict'])
        assert sd['teacher_temp'] == DEFAULT[1] and sd['momentum'] == ALPHA
        tr.close()
    for ga, ea in zip(runs[True], runs[False]):
        for a, b_ in zip(ga, ea):
            assert torch.equal(bits(a), bits(b_))
    for a, b_ in zip(finals[True], finals[False]):
        assert torch.equal(bits(a), bits(b_))
    vals = [float(o[0]) for o in runs[False]]
    student, teacher = dm.oracle_dino('R2P1D10T', 8, 32, PROTOS, state)
    want, want_c, want_ct = dm.oracle_steps(student, teacher, x.cpu().double(), 3, LR, ALPHA, PROTOS)
    center, ct, cs = finals[False]
    e = dict(center=rel(center, want_c), teacher_prototypes=rel(ct, want_ct))
    print('MEASURED dino trainer losses on one repeated batch: %s  oracle: %s  centre %.2e teacher prototypes %.2e'
          % (' '.join('%.6f' % v for v in vals), ' '.join('%.6f' % v for v in want), e['center'], e['teacher_prototypes']))
    assert all(np.isfinite(vals))
    for got, ref in zip(vals, want):
        assert abs(got - ref) <= 1e-3 * abs(ref), (vals, want)
    assert max(e.values()) <= 1e-3, e
    if want[-1] < want[0]:
        assert vals[-1] < vals[0]
    assert float(center.abs().max()) > 0 and not torch.equal(ct, cs) and not torch.equal(ct, state['model.prototypes.weight'].to(DEV))
    first = [float(v) for v in runs[False][0]]
    assert abs(0.5 * (first[1] + first[2]) - first[0]) <= 1e-6 * abs(first[0])
    assert 0.0 < first[3] <= math.log(PROTOS)


def test_set_schedule_between_replays(pkg):
    """The captured step reads both schedule values from the device: a graph trainer whose schedule is moved after capture
    equals, bit for bit, an eager trainer given the same values at the same steps."""
    cfg = dino_cfg(pkg, WARMUP_FACTOR=1.0, BASE_LR=LR)
    xs = clips(35, 5)
    sched = [(None, None)] * 3 + [(0.07, 0.99), (0.05, 1.0)]                    # the graph is captured at the third step
    res = {}
    for use_graph in (True, False):
        tr = pkg.DINOTrainer(cfg, DEV, use_graph=use_graph, seed=9)
        losses = []
        for x, (tt, m) in zip(xs, sched):
            tr.set_schedule(teacher_temp=tt, momentum=m)
            if m == 1.0:
                frozen = {n: p.detach().clone() for n, p in tr.model_ema.named_parameters()}
            losses.append(tr.train_step(x)['loss'].detach().clone())
        torch.cuda.synchronize()
        if use_graph:
            graph = tr._segments[0].graph
            assert graph is not None
        for n, p in tr.model_ema.named_parameters():                            # momentum 1: the teacher stands still ...
            if n != 'model.prototypes.weight':
                assert torch.equal(bits(frozen[n]), bits(p)), n
        was = dr.ema(frozen['model.prototypes.weight'].double().cpu().numpy(), 0.0, 1.0)
        was /= np.sqrt((was * was).sum(axis=1, keepdims=True))                   # ... but for the step's renormalisation of its prototypes
        assert rel(tr.model_ema.model.prototypes.weight, torch.from_numpy(was)) <= 1e-6
        assert (tr.teacher_temp, tr.momentum) == (0.05, 1.0) and float(tr.tt_dev) == f32(0.05) and float(tr.m_dev) == 1.0
        res[use_graph] = (losses, tr.arena_t.flat.clone(), tr.contrast.center.clone())
        for bad in (dict(teacher_temp=0.0), dict(teacher_temp=float('nan')), dict(teacher_temp=-0.04), dict(momentum=1.01),
                    dict(momentum=-0.1), dict(momentum=float('nan')), dict(teacher_temp=0.07, momentum=2.0)):
            with pytest.raises(ValueError):
                tr.set_schedule(**bad)
        assert (tr.teacher_temp, tr.momentum) == (0.05, 1.0) and float(tr.tt_dev) == f32(0.05)     # a refusal changes nothing
        tr.close()
    for a, b_ in zip(res[True][0], res[False][0]):
        assert torch.equal(bits(a), bits(b_))
    assert torch.equal(bits(res[True][1]), bits(res[False][1])) and torch.equal(bits(res[True][2]), bits(res[False][2]))


def test_checkpoint_resume_is_exact_and_loads_downstream(pkg):
    import copy
    import classify_model as cm
    from test_gpu_adam import action_cfg, assert_resume_is_exact
    cm.register()
    cfg = dino_cfg(pkg)

    def make(seed):
        tr = pkg.DINOTrainer(cfg, DEV, use_graph=False, seed=seed)
        if seed == 5:
            tr.set_schedule(teacher_temp=0.055, momentum=0.95)                  # the resumed trainer must pick these up
        return tr

    a, b_, sd = assert_resume_is_exact(make, clips(13, 5), ('epoch', 'state_dict', 'optimizer', 'contrast', 'model_ema',
                                                            'teacher_temp', 'momentum'))
    assert (b_.teacher_temp, b_.momentum) == (0.055, 0.95) and float(b_.tt_dev) == f32(0.055) and float(b_.m_dev) == f32(0.95)
    sa, sb = a.model_ema.state_dict(), b_.model_ema.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(bits(a.contrast.center), bits(b_.contrast.center)) and float(a.contrast.center.abs().max()) > 0
    assert all(k.startswith(('model.encoder.', 'model.proj_head.', 'model.prototypes.')) for k in sd['state_dict'])
    assert 'model.prototypes.weight' in sd['state_dict'] and list(sd['contrast']) == ['center']
    sd = copy.deepcopy(sd)
    from tests import parity
    tr = pkg.ActionTrainer(action_cfg(pkg, parity, False), DEV, seed=47)
    tr.load_pretrained(sd)
    n = 0
    for k, v in tr.model.state_dict().items():
        if not k.startswith('base_model.fc.'):
            src = [s for s in sd['state_dict'] if s.endswith('encoder.' + k)]
            assert len(src) == 1 and torch.equal(v, sd['state_dict'][src[0]].to(v.device)), k
            n += 1
    assert n == 126
    a.close(), b_.close()


def test_trainer_refusals(pkg):
    register_tiny(pkg)
    for mem in ('simsiam', 'moco', 'simclr', 'barlow', 'vicreg', 'swav'):
        with pytest.raises(ValueError, match='dino'):
            pkg.DINOTrainer(make_cfg(pkg, 'R2P1D10T', mem, 32, 16, 8), DEV)
    with pytest.raises(NotImplementedError, match='one GPU'):
        pkg.DINOTrainer(dino_cfg(pkg), DEV, ctx=pkg.parallel.DistCtx(force_active=True))
    for other in (pkg.SimCLRTrainer, pkg.SwAVTrainer):
        with pytest.raises(ValueError):
            other(dino_cfg(pkg), DEV)


def test_lars_step_moves_the_student_prototypes_and_through_the_ema_the_teachers(pkg):
    tr = pkg.DINOTrainer(dino_cfg(pkg, OPTIMIZER_NAME='LARS', BASE_LR=0.3), DEV, use_graph=False, seed=11)
    assert type(tr.optimizer).__name__ == 'HipLARS'
    before = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
    before_t = tr.model_ema.model.prototypes.weight.detach().clone()
    out = tr.train_step(clips(7, 1)[0])
    torch.cuda.synchronize()
    assert np.isfinite(float(out['loss']))
    adapted = [n for n, p in tr.model.named_parameters() if p.ndim > 1]
    assert len(adapted) > 20 and 'model.prototypes.weight' in adapted
    for n, p in tr.model.named_parameters():
        assert bool(torch.isfinite(p).all()), n
        if p.ndim > 1:
            assert not torch.equal(p.detach(), before[n]), n
    cs, ct = tr.model.model.prototypes.weight.detach(), tr.model_ema.model.prototypes.weight.detach()
    assert not torch.equal(ct, before_t)
    want = dr.ema(before_t.double().cpu().numpy(), cs.double().cpu().numpy(), f32(ALPHA))   # (before_t had unit rows already)
    assert rel(ct, torch.from_numpy(want)) <= 1e-6
    tr.close()
