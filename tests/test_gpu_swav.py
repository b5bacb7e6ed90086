"""gca_rows_normalize / gca_swav_fwd / gca_swav_bwd, ops.swav_*, lib.memory.swav.SwAVLoss, the SwAV wrapper and SwAVTrainer on
the device, against tests/swav_ref.py (fp64 numpy) and tests/swav_model.py (the fp64 torch oracle of the model).

Kernel parity: parts (loss, l12, l21), codes, dz1, dz2, dC against the specification fed the same fp32 inputs, each array's
max-norm error relative to its largest reference entry.  The bar is swav_ref.BAR = 1e-5: the next power of ten above 4 x the
worst error measured on these cases (1.87e-6), and no more than 1e-4 -- the largest exponential argument is 2 / eps = 80, whose
fp32 rounding is 80 x 2^-24, about 5e-6 per term, and the Sinkhorn rounds and the softmax add a small multiple of that.  Every
wrong variant of tests/test_swav_ref.py misses by more than 100 bars.

Measured on an MI355X (printed as `MEASURED swav ...`), worst over the cases:
    unit rows      loss 1.02e-7   l12 1.41e-7   l21 8.45e-8   codes 1.26e-6 (65 x 128 x 3000)   dz1 1.05e-6   dz2 1.12e-6 (33 x 130 x
                   65)   dC 1.48e-6 (65 x 128 x 3000); with eps 0.025, T 0.5, 1 round: codes 1.87e-6 (65 x 128 x 3000), the worst
                   of all; with eps 1, T 0.07, 16 rounds: 1.06e-6
    adversarial    eps 0.025, every score -1: codes 1.20e-7 of 1 / K, loss 1.59e-7 of log K, gradients 4.24e-7 of 1 / (2 N T);
                   one prototype at +1 and the rest at -1: 1.38e-6 (dC, 65 x 7 x 130); nothing non-finite, no zero code
    pointers offset by 4 bytes (33 x 130 x 65): 1.14e-6        rows_normalize (67 x 130): 7.5e-8                       [bar 1e-5]
    model          loss of SwAV.forward against the fp64 oracle: 4.99e-7 relative (l12 4.92e-7, l21 4.05e-7)             [bar 1e-3]
                   parameter gradients: median 7.39e-6, 95th percentile 1.16e-5, worst 1.43e-5 over 68 tensors; prototypes 9.7e-7
    trainer        loss on one repeated batch, SGD lr 3e-4: 4.236870 3.801836 3.457883 against the oracle's 4.236871 3.801815
                   3.457691 (2.2e-7, 5.5e-6, 5.6e-5 relative)                                                           [bar 1e-3]
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swav_ref as sr                    # noqa: E402
import swav_model as sm                  # noqa: E402
from parity import check_grad_errors, make_cfg, register_tiny, rel           # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = -1
BAR = sr.BAR
DEFAULT = (sr.DEFAULTS['eps'], sr.DEFAULTS['T'], sr.DEFAULTS['iters'])
PARAMS = [DEFAULT, (0.025, 0.5, 1), (1.0, 0.07, 16)]
ARRAYS = ('codes', 'dz1', 'dz2', 'dC')
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
        z1, z2, C = sr.unit_inputs(N, D, K, seed)
        eps, T, iters = params
        _REF[key] = (z1, z2, C, sr.grads(z1, z2, C, f32(eps), f32(T), iters))
    return _REF[key]


def run(ops, a, b, c, params=DEFAULT, accumulate=False, dC=None, **kw):
    """-> (parts, codes, dz1, dz2, dC)"""
    parts, dS, codes = ops.swav_fwd(a, b, c, *params, want_codes=True)
    dC = torch.empty_like(c) if dC is None else dC
    dz1, dz2 = ops.swav_bwd(a, b, c, dS, dC, accumulate, **kw)
    return parts, codes, dz1, dz2, dC


def errors(got, ref):
    """max-norm errors of (parts, codes, dz1, dz2, dC) on the device, each relative to its largest reference entry"""
    parts = got[0].cpu().numpy().astype(np.float64)
    e = {k: abs(parts[i] - ref[k]) / abs(ref[k]) for i, k in enumerate(('loss', 'l12', 'l21'))}
    for k, t in zip(ARRAYS, got[1:]):
        e[k] = rel(t, torch.from_numpy(np.ascontiguousarray(ref[k])))
    return e


def show(what, e):
    print('MEASURED swav %s: rel_err %s  worst %.2e' % (what, ' '.join('%s %.2e' % kv for kv in e.items()), max(e.values())))


# ----------------------------------------------------------------------------- 1. the kernels against the specification
@pytest.mark.parametrize('N,D,K', sr.KERNEL_CASES)
def test_kernel_parity(pkg, N, D, K):
    assert sr.route(N, D, K) == 'tiled' and pkg._hip.lib.gca_swav_dz_splits(N, D, K) == sr.dz_splits(N, D, K)
    z1, z2, C, ref = unit_ref(N, D, K)
    got = run(pkg.engine.ops, dev(z1), dev(z2), dev(C))
    torch.cuda.synchronize()
    e = errors(got, ref)
    show('unit rows N=%d D=%d K=%d' % (N, D, K), e)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert max(e.values()) <= BAR, e
    assert float((got[1].sum(dim=2) - 1.0).abs().max()) <= 1e-5               # every row of the codes sums to 1


@pytest.mark.parametrize('params', PARAMS[1:])
@pytest.mark.parametrize('N,D,K', [(33, 130, 65), (65, 128, 3000)])
def test_eps_temperature_and_iterations(pkg, N, D, K, params):
    z1, z2, C, ref = unit_ref(N, D, K, params)
    got = run(pkg.engine.ops, dev(z1), dev(z2), dev(C), params)
    torch.cuda.synchronize()
    e = errors(got, ref)
    show('unit rows N=%d D=%d K=%d eps=%g T=%g iters=%d' % ((N, D, K) + params), e)
    assert max(e.values()) <= BAR, e


@pytest.mark.parametrize('make', [sr.equal_scores_inputs, sr.one_hot_scores_inputs], ids=['equal', 'one_hot'])
@pytest.mark.parametrize('N,D,K', sr.ADVERSARIAL_CASES)
def test_adversarial_scores_at_the_smallest_eps(pkg, N, D, K, make):
    """(max - min) / eps = 80 and, with the bound 1 as the shift, entries of P down to exp(-80): nothing may underflow to a zero
    column or turn non-finite; the codes come out uniform."""
    params = (sr.ADVERSARIAL_EPS, 0.1, 3)
    z1, z2, C = make(N, D, K)
    ref = sr.grads(z1, z2, C, f32(params[0]), f32(params[1]), params[2])
    got = run(pkg.engine.ops, dev(z1), dev(z2), dev(C), params)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert float(got[1].min()) > 0.0 and float((got[1] * K - 1.0).abs().max()) <= 1e-4
    e = errors(got, ref)
    if make is sr.equal_scores_inputs:
        # softmax - q is 1 / K - 1 / K: the reference's gradients are pure rounding, no scale for a relative error.  They are held
        # to the bar of the size one entry of dS would have had, 1 / (2 N T), instead.
        scale = 1.0 / (2.0 * N * params[1])
        for k in ('dz1', 'dz2', 'dC'):
            e[k] = float((got[1 + ARRAYS.index(k)].double().cpu() - torch.from_numpy(ref[k])).abs().max()) / scale
    show('%s N=%d D=%d K=%d eps=%g' % (make.__name__, N, D, K, params[0]), e)
    assert max(e.values()) <= BAR, e


def test_rows_normalize(pkg):
    """An offset matrix, neither size a multiple of 64, rows of very different lengths and one zero row."""
    ops = pkg.engine.ops
    K, D = 67, 130
    rng = np.random.RandomState(11)
    C = (rng.randn(K, D) * rng.uniform(1e-3, 1e3, size=(K, 1))).astype(np.float32)
    C[5] = 0.0
    buf = torch.full((K * D + 2,), 777.0, device=DEV)
    view = buf[1:1 + K * D].view(K, D)
    view.copy_(dev(C))
    assert view.data_ptr() % 8 == 4
    out = ops.rows_normalize_(view)
    torch.cuda.synchronize()
    assert out is view and float(buf[0]) == 777.0 and float(buf[-1]) == 777.0
    want = sr.rows_normalize(C)
    err = rel(view, torch.from_numpy(want))
    print('MEASURED swav rows_normalize K=%d D=%d: rel_err %.2e' % (K, D, err))
    assert err <= 1e-6 and float(view[5].abs().max()) == 0.0
    again = view.clone()
    ops.rows_normalize_(view)                                                   # unit rows stay unit rows, to rounding
    torch.cuda.synchronize()
    assert rel(view, again) <= 2e-7


@pytest.mark.parametrize('N,D,K', [(33, 130, 65), (65, 128, 3000)])
def test_accumulate_dC(pkg, N, D, K):
    ops = pkg.engine.ops
    z1, z2, C, ref = unit_ref(N, D, K)
    a, b, c = dev(z1), dev(z2), dev(C)
    base = torch.from_numpy(np.random.RandomState(3).randn(K, D).astype(np.float32)).to(DEV) * float(np.abs(ref['dC']).max())
    fresh = run(ops, a, b, c, dC=torch.full((K, D), float('nan'), device=DEV))[4]
    added = run(ops, a, b, c, accumulate=True, dC=base.clone())[4]
    torch.cuda.synchronize()
    assert rel(fresh, torch.from_numpy(ref['dC'])) <= BAR                       # accumulate False overwrites, NaNs included
    assert torch.equal(bits(added), bits(base + fresh))                         # accumulate True adds exactly one rounding


@pytest.mark.parametrize('N,D,K', [(33, 130, 65), (64, 128, 128)])
def test_gradient_scale(pkg, N, D, K):
    ops = pkg.engine.ops
    a, b, c = (dev(t) for t in sr.unit_inputs(N, D, K, seed=5))
    _, dS = ops.swav_fwd(a, b, c, *DEFAULT)

    def bwd(**kw):
        dC = torch.empty_like(c)
        return ops.swav_bwd(a, b, c, dS, dC, False, **kw) + (dC,)

    one = bwd()
    scaled = bwd(gscale_dev=torch.tensor([1024.0, 7.0], device=DEV))
    half = bwd(gscale_host=0.5)
    both = bwd(gscale_dev=torch.tensor([3.0], device=DEV), gscale_host=-0.7)
    torch.cuda.synchronize()
    for v in range(3):
        assert float(one[v].abs().max()) > 0
        assert rel(scaled[v], one[v] * 1024.0) <= 1e-6 and rel(half[v], one[v] * 0.5) <= 1e-6
        assert rel(both[v], one[v].double() * (3.0 * np.float64(np.float32(-0.7)))) <= 1e-6


def test_pointers_offset_by_four_bytes(pkg):
    """Nothing assumes 16-byte alignment: inputs, saved state, workspace and outputs all start 4 bytes into their buffers."""
    N, D, K = 33, 130, 65
    z1, z2, C, ref = unit_ref(N, D, K)
    lib, H = pkg._hip.lib, pkg._hip

    def off(shape, src=None):
        n = int(np.prod(shape))
        buf = torch.zeros(n + 1, device=DEV)
        v = buf[1:].view(*shape)
        if src is not None:
            v.copy_(dev(src))
        assert v.data_ptr() % 8 == 4
        return v

    a, b, c = off((N, D), z1), off((N, D), z2), off((K, D), C)
    parts, dS, codes, dz1, dz2, dC = off((3,)), off((2, N, K)), off((2, N, K)), off((N, D)), off((N, D)), off((K, D))
    ws = torch.empty(lib.gca_swav_ws_bytes(N, D, K) + 4, dtype=torch.uint8, device=DEV)
    p = H.ptr
    assert lib.gca_swav_fwd(p(a), p(b), p(c), N, D, K, *DEFAULT, p(parts), p(dS), p(codes), p(ws) + 4, H.stream()) == 0
    assert lib.gca_swav_bwd(p(a), p(b), p(c), p(dS), N, D, K, None, 1.0, p(dz1), p(dz2), p(dC), 0, p(ws) + 4, H.stream()) == 0
    torch.cuda.synchronize()
    e = errors((parts, codes, dz1, dz2, dC), ref)
    show('offset pointers N=%d D=%d K=%d' % (N, D, K), e)
    assert max(e.values()) <= BAR, e


@pytest.mark.parametrize('N,D,K', [(33, 130, 65), (64, 128, 128), (65, 128, 3000)])
def test_deterministic(pkg, N, D, K):
    a, b, c = (dev(t) for t in sr.unit_inputs(N, D, K, seed=3))
    outs = [run(pkg.engine.ops, a, b, c) for _ in range(2)]
    torch.cuda.synchronize()
    for x, y in zip(*outs):
        assert torch.equal(bits(x), bits(y))


def test_refused_arguments_touch_nothing(pkg):
    lib, H = pkg._hip.lib, pkg._hip
    N, D, K = 8, 8, 6
    z1, z2, C = (dev(t) for t in sr.unit_inputs(N, D, K))
    SENT = 12345.0
    parts, dS, codes, dz1, dz2, dC, Cn = (torch.full((n,), SENT, device=DEV) for n in (3, 2 * N * K, 2 * N * K, N * D, N * D, K * D, K * D))
    good = pkg.engine.ops.swav_fwd(z1, z2, C, *DEFAULT)
    ws = torch.empty(max(lib.gca_swav_ws_bytes(N, D, K), 1 << 16), dtype=torch.uint8, device=DEV)
    p = H.ptr
    nan, inf = float('nan'), float('inf')

    def fwd(a=p(z1), b=p(z2), c=p(C), N=N, D=D, K=K, eps=0.05, T=0.1, iters=3, pa=p(parts), s=p(dS), q=p(codes), w=p(ws)):
        return lib.gca_swav_fwd(a, b, c, N, D, K, eps, T, iters, pa, s, q, w, H.stream())

    def bwd(a=p(z1), b=p(z2), c=p(C), s=p(good[1]), N=N, D=D, K=K, gs=1.0, d1=p(dz1), d2=p(dz2), dc=p(dC), acc=0, w=p(ws)):
        return lib.gca_swav_bwd(a, b, c, s, N, D, K, None, gs, d1, d2, dc, acc, w, H.stream())

    shared = [dict(N=1), dict(N=0), dict(N=-2), dict(N=8193), dict(D=0), dict(D=-1), dict(D=8193), dict(K=1), dict(K=0),
              dict(K=65537), dict(N=1 << 31), dict(a=None), dict(b=None), dict(c=None), dict(s=None), dict(w=None)]
    for f in (fwd, bwd):
        for kw in shared:
            assert f(**kw) == EINVAL, (f.__name__, kw)
    for kw in (dict(eps=0.0249), dict(eps=1.0001), dict(eps=-0.05), dict(eps=nan), dict(eps=inf), dict(T=0.0), dict(T=-0.1),
               dict(T=inf), dict(T=nan), dict(iters=0), dict(iters=17), dict(iters=-1), dict(pa=None)):
        assert fwd(**kw) == EINVAL, kw
    for kw in (dict(gs=inf), dict(gs=-inf), dict(gs=nan), dict(d1=None), dict(d2=None), dict(dc=None)):
        assert bwd(**kw) == EINVAL, kw
    for kw in (dict(K=0), dict(K=65537), dict(D=0), dict(D=8193)):
        args = dict(K=K, D=D)
        args.update(kw)
        assert lib.gca_rows_normalize(p(Cn), args['K'], args['D'], H.stream()) == EINVAL, kw
    assert lib.gca_rows_normalize(None, K, D, H.stream()) == EINVAL
    assert lib.gca_swav_ws_bytes(1, 8, 8) == -1 and lib.gca_swav_ws_bytes(8, 8193, 8) == -1 and lib.gca_swav_ws_bytes(8, 8, 1) == -1
    torch.cuda.synchronize()
    for t in (parts, dS, codes, dz1, dz2, dC, Cn):
        assert float(t.min()) == SENT == float(t.max())
    # and the accepted calls write all of their outputs (codes only when asked for)
    assert fwd(q=None) == 0
    torch.cuda.synchronize()
    assert float((dS == SENT).sum()) == 0 and float((parts == SENT).sum()) == 0 and float(codes.min()) == SENT == float(codes.max())
    assert fwd() == 0 and bwd() == 0 and lib.gca_rows_normalize(p(Cn), K, D, H.stream()) == 0
    torch.cuda.synchronize()
    for t in (parts, dS, codes, dz1, dz2, dC, Cn):
        assert float((t == SENT).sum()) == 0


def test_ops_refuse_what_the_entry_refuses(pkg):
    ops = pkg.engine.ops
    z, C = torch.zeros(4, 8, device=DEV), torch.zeros(6, 8, device=DEV)
    dS, dC = torch.zeros(2, 4, 6, device=DEV), torch.zeros(6, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.swav_fwd(torch.zeros(1, 8, device=DEV), torch.zeros(1, 8, device=DEV), C, *DEFAULT)
    with pytest.raises(ValueError):
        ops.swav_fwd(z, z, torch.zeros(1, 8, device=DEV), *DEFAULT)
    with pytest.raises(ValueError):
        ops.swav_fwd(z, z, torch.zeros(6, 7, device=DEV), *DEFAULT)
    for params in ((0.02, 0.1, 3), (0.05, float('nan'), 3), (0.05, 0.0, 3), (0.05, 0.1, 0), (0.05, 0.1, 17)):
        with pytest.raises(ValueError):
            ops.swav_fwd(z, z, C, *params)
    with pytest.raises(ValueError):
        ops.swav_bwd(z, z, C, torch.zeros(2, 4, 7, device=DEV), dC, False)
    with pytest.raises(ValueError):
        ops.swav_bwd(z, z, C, dS, torch.zeros(6, 7, device=DEV), False)
    with pytest.raises(ValueError):
        ops.swav_bwd(z, z, C, dS, dC, False, gscale_host=float('inf'))
    with pytest.raises(ValueError):
        ops.rows_normalize_(torch.zeros(6, 8193, device=DEV))


def test_capturable_in_a_graph(pkg):
    """Prototype normalisation, forward and backward inside one captured graph: replays track the static inputs and equal the
    eager bits."""
    ops = pkg.engine.ops
    N, D, K = 65, 128, 3000
    z1, z2, C, _ = unit_ref(N, D, K)
    s1, s2, sc = dev(z1).clone(), dev(z2).clone(), dev(C).clone()

    def step():
        ops.rows_normalize_(sc)
        return run(ops, s1, s2, sc)

    eager = step()
    torch.cuda.synchronize()
    sc.copy_(dev(C))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = step()
    sc.copy_(dev(C))
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, captured):
        assert torch.equal(bits(x), bits(y))
    n1, n2, nc = sr.unit_inputs(N, D, K, seed=9)
    s1.copy_(dev(n1))
    s2.copy_(dev(n2))
    sc.copy_(dev(nc) * 3.0)                                                     # the captured normalisation undoes the factor
    g.replay()
    torch.cuda.synchronize()
    assert row_norm_error(sc) <= 1e-6
    ref = sr.grads(n1, n2, sc.cpu().numpy(), f32(DEFAULT[0]), f32(DEFAULT[1]), DEFAULT[2])   # the prototypes the kernels met
    e = errors(captured, ref)
    assert max(e.values()) <= BAR, e
    g.reset()


# ----------------------------------------------------------------------------- 2. the module
def test_module_forward_backward(pkg):
    import importlib
    SwAVLoss = importlib.import_module(pkg.__name__ + '.lib.memory.swav').SwAVLoss
    N, D, K = 33, 130, 65
    z1, z2, C, _ = unit_ref(N, D, K)
    ref = sr.grads(z1, z2, C, f32(DEFAULT[0]), f32(DEFAULT[1]), DEFAULT[2], g=3.0)
    t1, t2, tc = (dev(t).requires_grad_(True) for t in (z1, z2, C))
    crit = SwAVLoss(*DEFAULT)
    loss = crit(t1, t2, tc)
    assert loss.dim() == 0 and abs(float(loss.detach()) - ref['loss']) <= BAR * abs(ref['loss'])
    (loss * 3.0).backward()
    torch.cuda.synchronize()
    for t, k in ((t1, 'dz1'), (t2, 'dz2'), (tc, 'dC')):
        assert rel(t.grad, torch.from_numpy(ref[k])) <= BAR, k
    for got, k in ((crit.l12, 'l12'), (crit.l21, 'l21')):
        assert got.is_cuda and got.dim() == 0 and abs(float(got) - ref[k]) <= BAR * ref[k], k


# ----------------------------------------------------------------------------- 3. model and trainer
CLIP = (8, 6, 8, 48, 48)
PROTOS = 24


def clips(seed, n=4):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*CLIP, generator=gen).to(DEV) for _ in range(n)]


def swav_cfg(pkg, **solver):
    register_tiny(pkg)
    cfg = make_cfg(pkg, 'R2P1D10T', 'swav', 32, 16, 8, **solver)
    cfg.CONTRAST.SWAV_K = PROTOS
    return cfg


def row_norm_error(w):
    return float((w.detach().double().norm(dim=1) - 1.0).abs().max())


def test_model_against_the_fp64_oracle(pkg):
    tr = pkg.SwAVTrainer(swav_cfg(pkg), DEV, use_graph=False, seed=21)
    inner = tr.model.model
    with torch.no_grad():
        inner.prototypes.weight.mul_(1.7)                                       # the forward has something to normalise
    state = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    x = clips(31, 1)[0]
    oracle = sm.oracle_swav('R2P1D10T', 8, 32, PROTOS, state)
    want, l12, l21, _, _ = sm.model_loss(oracle, x.cpu().double())
    want.backward()
    tr.optimizer.zero_grad()
    got = tr.model(x)
    got.backward()
    torch.cuda.synchronize()
    got, want = got.detach(), want.detach()
    assert row_norm_error(inner.prototypes.weight) <= 1e-6                      # unit rows after the forward
    e = dict(loss=abs(float(got) - float(want)) / abs(float(want)))
    for k, mine, ref in (('l12', inner.l12, l12), ('l21', inner.l21, l21)):
        e[k] = abs(float(mine) - float(ref.detach())) / abs(float(ref.detach()))
    print('MEASURED swav model loss %.6f vs oracle %.6f: rel err %s' % (float(got), float(want), ' '.join('%s %.3e' % kv for kv in e.items())))
    assert got.dim() == 0 and max(e.values()) < 1e-3, e
    g64 = {n: p.grad for n, p in oracle.named_parameters()}
    errs = {n: rel(p.grad, g64[n]) for n, p in tr.model.named_parameters() if g64[n] is not None and g64[n].abs().max() > 0}
    assert len(errs) > 40 and 'model.prototypes.weight' in errs and 'model.proj_head.head.2.weight' in errs
    med, p95, worst = check_grad_errors(errs, 'swav parameter gradients')
    print('MEASURED swav model parameter gradients: median %.2e p95 %.2e worst %.2e over %d tensors; prototypes %.2e'
          % (med, p95, worst, len(errs), errs['model.prototypes.weight']))
    assert errs['model.prototypes.weight'] < 1e-3
    tr.close()


def test_trainer_graph_equals_eager_and_follows_the_oracle(pkg):
    """Three steps on one repeated batch.  The rate is chosen by the oracle's own error: this tiny model on 8 clips is badly
    conditioned over several steps -- at a rate of 0.01 the fp32 run of the ORACLE leaves its fp64 run by 3.6e-4 at the second loss
    and 9.6e-3 at the third (and weights perturbed by 1e-6 move the fp64 run as far), at 3e-4 by 5.1e-6 and 5.5e-5, a twentieth
    of the 1e-3 bar.  The fp64 oracle's loss falls on this batch at this rate (checked on the CPU: 4.2369, 3.8018, 3.4577), so
    the product's must."""
    lr = 3e-4
    cfg = swav_cfg(pkg, WARMUP_FACTOR=1.0, BASE_LR=lr)
    x = clips(33, 1)[0]
    ops = pkg.engine.ops
    runs, norms, state = {}, [], None
    keys = ('loss', 'l12', 'l21')
    for use_graph in (True, False):
        tr = pkg.SwAVTrainer(cfg, DEV, use_graph=use_graph, seed=7)
        if state is None:
            state = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
        real = ops.swav_fwd

        def spy(z1, z2, C, *a, **kw):
            norms.append(row_norm_error(C))                                     # the prototypes as the loss kernels meet them
            return real(z1, z2, C, *a, **kw)

        if not use_graph:
            ops.swav_fwd = spy
        try:
            outs = []
            for _ in range(3):
                out = tr.train_step(x)
                torch.cuda.synchronize()
                assert set(out) >= set(keys)
                outs.append(tuple(out[k].detach().clone() for k in keys))
                if use_graph:                                                   # (the next forward renormalises what the step moved)
                    w = tr.model.model.prototypes.weight.detach().clone()
                    ops.rows_normalize_(w)
                    assert row_norm_error(w) <= 1e-6
        finally:
            ops.swav_fwd = real
        assert (tr._segments[0].graph is not None) == use_graph
        runs[use_graph] = outs
        sd = tr.state_dict()
        assert sd['contrast'] is None and 'model_ema' not in sd
        tr.close()
    for ga, ea in zip(runs[True], runs[False]):
        for a, b_ in zip(ga, ea):
            assert torch.equal(bits(a), bits(b_))
    assert len(norms) == 3 and max(norms) <= 1e-6, norms
    vals = [float(o[0]) for o in runs[False]]
    oracle = sm.oracle_swav('R2P1D10T', 8, 32, PROTOS, state)
    want = sm.oracle_steps(oracle, x.cpu().double(), 3, lr)
    print('MEASURED swav trainer losses on one repeated batch: %s  oracle: %s'
          % (' '.join('%.6f' % v for v in vals), ' '.join('%.6f' % v for v in want)))
    assert all(np.isfinite(vals))
    for got, ref in zip(vals, want):
        assert abs(got - ref) <= 1e-3 * abs(ref), (vals, want)
    if want[-1] < want[0]:
        assert vals[-1] < vals[0]
    first = [float(v) for v in runs[False][0]]
    assert abs(0.5 * (first[1] + first[2]) - first[0]) <= 1e-6 * abs(first[0])


def test_checkpoint_resume_is_exact_and_loads_downstream(pkg):
    import copy
    import classify_model as cm
    from test_gpu_adam import action_cfg, assert_resume_is_exact
    cm.register()
    cfg = swav_cfg(pkg)
    a, b_, sd = assert_resume_is_exact(lambda seed: pkg.SwAVTrainer(cfg, DEV, use_graph=False, seed=seed), clips(13, 5),
                                       ('epoch', 'state_dict', 'optimizer', 'contrast'))
    assert sd['contrast'] is None and 'model_ema' not in sd
    assert all(k.startswith(('model.encoder.', 'model.proj_head.', 'model.prototypes.')) for k in sd['state_dict'])
    assert 'model.prototypes.weight' in sd['state_dict']
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
    E = pkg.lib.evaluation
    enc = E.load_encoder(sd, 'R2P1D10T', 8)
    assert not enc.training
    feats = E.extract_feature_single(enc.to(DEV), clips(3, 1)[0][:2, :3].contiguous(), 1, 8)
    assert tuple(feats.shape) == (2, enc.feature_dim) and bool(torch.isfinite(feats).all()) and float(feats.abs().max()) > 0
    a.close(), b_.close()


def test_trainer_refusals(pkg):
    register_tiny(pkg)
    for mem in ('simsiam', 'moco', 'simclr', 'barlow', 'vicreg'):
        with pytest.raises(ValueError, match='swav'):
            pkg.SwAVTrainer(make_cfg(pkg, 'R2P1D10T', mem, 32, 16, 8), DEV)
    with pytest.raises(NotImplementedError, match='one GPU'):
        pkg.SwAVTrainer(swav_cfg(pkg), DEV, ctx=pkg.parallel.DistCtx(force_active=True))
    for other in (pkg.SimCLRTrainer, pkg.VICRegTrainer):
        with pytest.raises(ValueError):
            other(swav_cfg(pkg), DEV)


def test_lars_step_changes_the_prototypes(pkg):
    tr = pkg.SwAVTrainer(swav_cfg(pkg, OPTIMIZER_NAME='LARS', BASE_LR=0.3), DEV, use_graph=False, seed=11)
    assert type(tr.optimizer).__name__ == 'HipLARS'
    before = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
    out = tr.train_step(clips(7, 1)[0])
    torch.cuda.synchronize()
    assert np.isfinite(float(out['loss']))
    adapted = [n for n, p in tr.model.named_parameters() if p.ndim > 1]
    assert len(adapted) > 20 and 'model.prototypes.weight' in adapted
    for n, p in tr.model.named_parameters():
        assert bool(torch.isfinite(p).all()), n
        if p.ndim > 1:
            assert not torch.equal(p.detach(), before[n]), n
    tr.close()
