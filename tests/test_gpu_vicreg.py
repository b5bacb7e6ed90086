"""gca_vicreg_fwd / gca_vicreg_bwd, ops.vicreg_*, lib.memory.VICRegLoss, the VICReg wrapper and VICRegTrainer on the device,
against tests/vicreg_ref.py (fp64 numpy) and tests/vicreg_model.py (the fp64 torch oracle of the model).

Exact inputs (N = 2^k + 1, columns of +-1/2 in equal counts and one 0, eps = 0, sim = 0, std = 16, cov = 1: every quantity is the
same number in fp32 and fp64 under any order of summation, tests/test_vicreg_ref.py): stats, covm (and covm[v] == covm[v].T),
loss4, dz1, dz2 bit for bit -- loss4[1] = inv, a division by N D with N odd, is the fp32 rounding of the fp64 quotient.  With
sim = 16 that quotient enters the loss and the gradient, which are then held to the float bar.

Float inputs (hinges active and not, a constant and a nearly collapsed column, means of a few units, view 2 a noisy copy of view
1; coefficients (25, 25, 1) and (1, 0, 4)): loss, inv, varl, covl, stats, covm, dz1, dz2 within 1e-5 (max-norm relative) of the
fp64 specification on the same fp32 inputs -- Barlow's rule, which stands because the unfused fp32 torch chain, gradient
included, stays within a third of it on these inputs (tests/test_vicreg_ref.py: at most 5.8e-7), while each of the wrong
variants of tests/vicreg_ref.py misses by 1e-3 or more.

Measured on an MI355X (printed as `MEASURED vicreg ...`), worst over the cases:
    exact inputs   every output equals fp64 at all eight sizes (e.g. N = 17, D = 128: loss 9.0247802734375, varl 0.5,
                   covl 1.0247802734375); with sim = 16: loss 5.14e-8, inv 2.98e-8, dz 4.88e-8, the rest exact
    float inputs   loss 7.20e-8   inv 7.86e-8   varl 6.28e-8   covl 2.34e-7 (4100 x 40)   stats 1.14e-7   covm 5.99e-7 (256 x 512)
                   dz1 1.40e-6 (5 x 1, coefficients 25 / 25 / 1)   dz2 1.02e-6 (40 x 512, coefficients 1 / 0 / 4)
                   pointers offset by 4 bytes (33 x 130): 3.29e-7                                                   [bar 1e-5]
    model          loss of VICReg.forward against the fp64 oracle: 3.65e-7 relative (inv 2.01e-6, var 3.25e-7, cov 1.52e-6) [bar 1e-3]
                   parameter gradients: median 1.25e-5, 95th percentile 1.93e-5, worst 2.91e-5 over 70 tensors
    trainer        loss on one repeated batch, SGD lr 0.01: 21.62 22.44 21.93 19.45 18.69 17.66 15.77 14.71 13.48 12.79
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vicreg_ref as vr                  # noqa: E402
import vicreg_model as vm                # noqa: E402
from parity import check_grad_errors, make_cfg, register_tiny, rel           # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = -1
BAR = 1e-5
PARTS = ('loss', 'inv', 'varl', 'covl')
_REF = {}


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def float_ref(N, D, coeffs, seed=0):
    """The fp64 specification on the float inputs: computed once per case, shared, left unchanged."""
    key = (N, D, coeffs, seed)
    if key not in _REF:
        z1, z2 = vr.float_inputs(N, D, seed)
        _REF[key] = (z1, z2, vr.vicreg(z1, z2, *(np.float32(c) for c in coeffs), eps=np.float32(1e-4)))
    return _REF[key]


def errors(got, ref):
    """max-norm relative errors of (loss4, stats, covm, dz1, dz2) on the device against a vicreg_ref dict."""
    loss4, stats, covm, dz1, dz2 = got
    l4 = loss4.cpu().numpy().astype(np.float64)
    e = {k: abs(l4[i] - ref[k]) / max(abs(ref[k]), 1e-30) for i, k in enumerate(PARTS) if ref[k] != 0}
    for k, t in (('stats', stats), ('covm', covm), ('dz1', dz1), ('dz2', dz2)):
        e[k] = rel(t, torch.from_numpy(np.ascontiguousarray(ref[k])))
    return e


def run(ops, a, b, coeffs, eps=1e-4, **kw):
    loss4, stats, covm = ops.vicreg_fwd(a, b, *coeffs, eps)
    return (loss4, stats, covm) + ops.vicreg_bwd(a, b, stats, covm, *coeffs, **kw)


# ----------------------------------------------------------------------------- 1. the kernels against the specification
@pytest.mark.parametrize('N,D', vr.EXACT_CASES)
def test_exact_inputs_bit_for_bit(pkg, N, D):
    z1, z2 = vr.exact_inputs(N, D)
    ref = vr.vicreg(z1, z2, *vr.EXACT_COEFFS, eps=0.0)
    loss4, stats, covm, dz1, dz2 = run(pkg.engine.ops, dev(z1), dev(z2), vr.EXACT_COEFFS, eps=0.0)
    torch.cuda.synchronize()
    # inv is the one quotient that is not dyadic (N odd): fp32 holds the rounding of the fp64 value, everything else equals it
    want = dict(stats=ref['stats'], covm=ref['covm'], dz1=ref['dz1'], dz2=ref['dz2'],
                loss4=np.array([ref['loss'], float(np.float32(ref['inv'])), ref['varl'], ref['covl']]))
    got = dict(stats=stats, covm=covm, dz1=dz1, dz2=dz2, loss4=loss4)
    for k in want:
        g = got[k].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == want[k].shape, k
        assert np.array_equal(g.astype(np.float64), want[k]), (k, np.abs(g - want[k]).max())
    assert torch.equal(bits(covm), bits(covm.transpose(1, 2)))
    print('MEASURED vicreg exact N=%d D=%d: loss %.10g inv %.10g varl %.10g covl %.10g, every output equals fp64'
          % ((N, D) + tuple(loss4.tolist())))


@pytest.mark.parametrize('N,D', vr.EXACT_CASES)
def test_exact_inputs_with_the_invariance_term(pkg, N, D):
    coeffs = (16.0,) + vr.EXACT_COEFFS[1:]
    z1, z2 = vr.exact_inputs(N, D)
    ref = vr.vicreg(z1, z2, *coeffs, eps=0.0)
    got = run(pkg.engine.ops, dev(z1), dev(z2), coeffs, eps=0.0)
    torch.cuda.synchronize()
    e = errors(got, ref)
    print('MEASURED vicreg exact sim=16 N=%d D=%d: rel_err %s' % (N, D, ' '.join('%s %.2e' % kv for kv in e.items())))
    assert max(e.values()) <= BAR, e
    assert e['stats'] == 0 and e['covm'] == 0 and e['varl'] == 0                 # what sim does not touch stays exact
    assert torch.equal(bits(got[2]), bits(got[2].transpose(1, 2)))


@pytest.mark.parametrize('coeffs', vr.FLOAT_COEFFS)
@pytest.mark.parametrize('N,D', vr.FLOAT_CASES)
def test_float_inputs(pkg, N, D, coeffs):
    z1, z2, ref = float_ref(N, D, coeffs)
    got = run(pkg.engine.ops, dev(z1), dev(z2), coeffs)
    torch.cuda.synchronize()
    e = errors(got, ref)
    print('MEASURED vicreg float N=%d D=%d coeffs=%s: rel_err %s' % (N, D, coeffs, ' '.join('%s %.2e' % kv for kv in e.items())))
    assert max(e.values()) <= BAR, e
    assert torch.equal(bits(got[2]), bits(got[2].transpose(1, 2)))               # the mirrored tiles: covm[v] == covm[v].T
    if D >= 3:                                                                    # the constant column: sd = sqrt(eps)
        assert abs(float(got[1][1, -1]) - 0.01) <= 1e-8 and abs(float(got[1][3, -1]) - 0.01) <= 1e-8


def test_long_batch(pkg):
    """N past the 2048 rows after which the forward moves its accumulator tile aside, and a multiple of nothing: the
    reduction over N (column sums of 4100 terms, Cov over 129 chunks) is held to the same bar."""
    N, D, coeffs = 4100, 40, vr.FLOAT_COEFFS[0]
    z1, z2, ref = float_ref(N, D, coeffs)
    got = run(pkg.engine.ops, dev(z1), dev(z2), coeffs)
    torch.cuda.synchronize()
    e = errors(got, ref)
    print('MEASURED vicreg float N=%d D=%d coeffs=%s: rel_err %s' % (N, D, coeffs, ' '.join('%s %.2e' % kv for kv in e.items())))
    assert max(e.values()) <= BAR, e


def test_pointers_offset_by_four_bytes(pkg):
    """Nothing assumes 16-byte alignment: inputs, saved state and outputs all start 4 bytes into their buffers."""
    N, D, coeffs = 33, 130, vr.FLOAT_COEFFS[0]
    z1, z2, ref = float_ref(N, D, coeffs)
    lib, H = pkg._hip.lib, pkg._hip

    def off(shape, src=None):
        n = int(np.prod(shape))
        buf = torch.zeros(n + 1, device=DEV)
        v = buf[1:].view(*shape)
        if src is not None:
            v.copy_(dev(src))
        assert v.data_ptr() % 8 == 4
        return v

    a, b = off((N, D), z1), off((N, D), z2)
    loss4, stats, covm, dz1, dz2 = off((4,)), off((4, D)), off((2, D, D)), off((N, D)), off((N, D))
    ws = torch.empty(lib.gca_vicreg_ws_bytes(N, D) + 4, dtype=torch.uint8, device=DEV)
    p = H.ptr
    assert lib.gca_vicreg_fwd(p(a), p(b), N, D, *coeffs, 1e-4, p(stats), p(covm), p(loss4), p(ws) + 4, H.stream()) == 0
    assert lib.gca_vicreg_bwd(p(a), p(b), p(stats), p(covm), N, D, *coeffs, None, 1.0, p(dz1), p(dz2), p(ws) + 4, H.stream()) == 0
    torch.cuda.synchronize()
    e = errors((loss4, stats, covm, dz1, dz2), ref)
    print('MEASURED vicreg offset pointers N=%d D=%d: worst rel_err %.2e' % (N, D, max(e.values())))
    assert max(e.values()) <= BAR, e


@pytest.mark.parametrize('N,D', [(33, 130), (64, 128), (40, 512)])
def test_deterministic(pkg, N, D):
    z1, z2 = (dev(z) for z in vr.float_inputs(N, D, seed=3))
    outs = [run(pkg.engine.ops, z1, z2, vr.FLOAT_COEFFS[0]) for _ in range(2)]
    torch.cuda.synchronize()
    for x, y in zip(*outs):
        assert torch.equal(bits(x), bits(y))


@pytest.mark.parametrize('N,D', [(33, 130), (64, 128)])
def test_gradient_scale(pkg, N, D):
    ops = pkg.engine.ops
    z1, z2 = (dev(z) for z in vr.float_inputs(N, D, seed=5))
    _, stats, covm = ops.vicreg_fwd(z1, z2, 25.0, 25.0, 1.0)
    saved = (z1, z2, stats, covm, 25.0, 25.0, 1.0)
    one = ops.vicreg_bwd(*saved)
    scaled = ops.vicreg_bwd(*saved, gscale_dev=torch.tensor([1024.0, 7.0], device=DEV))
    half = ops.vicreg_bwd(*saved, gscale_host=0.5)
    both = ops.vicreg_bwd(*saved, gscale_dev=torch.tensor([3.0], device=DEV), gscale_host=-0.7)
    torch.cuda.synchronize()
    for v in range(2):
        assert float(one[v].abs().max()) > 0
        assert rel(scaled[v], one[v] * 1024.0) <= 1e-6 and rel(half[v], one[v] * 0.5) <= 1e-6
        assert rel(both[v], one[v].double() * (3.0 * np.float64(np.float32(-0.7)))) <= 1e-6


def test_refused_arguments_touch_nothing(pkg):
    lib, H = pkg._hip.lib, pkg._hip
    z1, z2 = (dev(z) for z in vr.float_inputs(8, 8))
    SENT = 12345.0
    stats, covm, loss, dz1, dz2 = (torch.full((n,), SENT, device=DEV) for n in (4 * 8, 2 * 8 * 8, 4, 8 * 8, 8 * 8))
    good = pkg.engine.ops.vicreg_fwd(z1, z2, 25.0, 25.0, 1.0)
    ws = torch.empty(max(lib.gca_vicreg_ws_bytes(8, 8), 1 << 16), dtype=torch.uint8, device=DEV)
    p = H.ptr
    nan, inf = float('nan'), float('inf')

    def fwd(a=p(z1), b=p(z2), N=8, D=8, sim=25.0, std=25.0, cov=1.0, eps=1e-4, s=p(stats), c=p(covm), lo=p(loss), w=p(ws)):
        return lib.gca_vicreg_fwd(a, b, N, D, sim, std, cov, eps, s, c, lo, w, H.stream())

    def bwd(a=p(z1), b=p(z2), N=8, D=8, sim=25.0, std=25.0, cov=1.0, s=p(good[1]), c=p(good[2]), gs=1.0, d1=p(dz1), d2=p(dz2),
            w=p(ws)):
        return lib.gca_vicreg_bwd(a, b, s, c, N, D, sim, std, cov, None, gs, d1, d2, w, H.stream())

    shared = [dict(N=1), dict(N=0), dict(N=-2), dict(N=65537, D=1), dict(D=0), dict(D=-1), dict(D=8193), dict(N=1 << 31, D=1),
              dict(a=None), dict(b=None), dict(s=None), dict(c=None), dict(w=None)]
    shared += [{k: v} for k in ('sim', 'std', 'cov') for v in (-1.0, inf, nan)]
    for f in (fwd, bwd):
        for kw in shared:
            assert f(**kw) == EINVAL, (f.__name__, kw)
    for kw in (dict(eps=-1e-5), dict(eps=inf), dict(eps=nan), dict(lo=None)):
        assert fwd(**kw) == EINVAL, kw
    for kw in (dict(gs=inf), dict(gs=-inf), dict(gs=nan), dict(d1=None), dict(d2=None)):
        assert bwd(**kw) == EINVAL, kw
    assert lib.gca_vicreg_ws_bytes(1, 8) == -1 and lib.gca_vicreg_ws_bytes(8, 8193) == -1
    torch.cuda.synchronize()
    for t in (stats, covm, loss, dz1, dz2):
        assert float(t.min()) == SENT == float(t.max())
    # and the accepted calls write all of their outputs
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    for t in (stats, covm, loss, dz1, dz2):
        assert float((t == SENT).sum()) == 0


def test_ops_refuse_what_the_entry_refuses(pkg):
    ops = pkg.engine.ops
    z = torch.zeros(4, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.vicreg_fwd(torch.zeros(1, 8, device=DEV), torch.zeros(1, 8, device=DEV), 25.0, 25.0, 1.0)
    with pytest.raises(ValueError):
        ops.vicreg_fwd(z, z, 25.0, float('nan'), 1.0)
    with pytest.raises(ValueError):
        ops.vicreg_bwd(z, z, torch.zeros(4, 8, device=DEV), torch.zeros(2, 8, 7, device=DEV), 25.0, 25.0, 1.0)


def test_capturable_in_a_graph(pkg):
    """Forward and backward inside one captured graph: replays track the static inputs and equal the eager bits."""
    ops = pkg.engine.ops
    N, D, coeffs = 40, 512, vr.FLOAT_COEFFS[0]
    z1, z2, _ = float_ref(N, D, coeffs)
    s1, s2 = dev(z1).clone(), dev(z2).clone()
    eager = run(ops, s1, s2, coeffs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = run(ops, s1, s2, coeffs)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, captured):
        assert torch.equal(bits(x), bits(y))
    n1, n2, ref = float_ref(N, D, coeffs, seed=9)
    s1.copy_(dev(n1))
    s2.copy_(dev(n2))
    g.replay()
    torch.cuda.synchronize()
    e = errors(captured, ref)
    assert max(e.values()) <= BAR, e
    g.reset()


# ----------------------------------------------------------------------------- 2. the module
def test_module_forward_backward(pkg):
    import importlib
    VICRegLoss = importlib.import_module(pkg.__name__ + '.lib.memory.vicreg').VICRegLoss
    N, D, coeffs = 33, 130, vr.FLOAT_COEFFS[0]
    z1, z2, _ = float_ref(N, D, coeffs)
    ref = vr.vicreg(z1, z2, *(np.float32(c) for c in coeffs), eps=np.float32(1e-4), g=3.0)
    t1, t2 = dev(z1).requires_grad_(True), dev(z2).requires_grad_(True)
    crit = VICRegLoss(*coeffs)
    loss = crit(t1, t2)
    assert loss.dim() == 0 and abs(float(loss.detach()) - ref['loss']) <= BAR * abs(ref['loss'])
    (loss * 3.0).backward()
    torch.cuda.synchronize()
    assert rel(t1.grad, torch.from_numpy(ref['dz1'])) <= BAR and rel(t2.grad, torch.from_numpy(ref['dz2'])) <= BAR
    for got, k in ((crit.inv, 'inv'), (crit.var, 'varl'), (crit.cov, 'covl')):
        assert got.is_cuda and got.dim() == 0 and abs(float(got) - ref[k]) <= BAR * ref[k], k


# ----------------------------------------------------------------------------- 3. model and trainer
CLIP = (8, 6, 8, 48, 48)


def clips(seed, n=4):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*CLIP, generator=gen).to(DEV) for _ in range(n)]


def vicreg_cfg(pkg, **solver):
    register_tiny(pkg)
    return make_cfg(pkg, 'R2P1D10T', 'vicreg', 32, 16, 8, **solver)


def test_model_against_the_fp64_oracle(pkg):
    tr = pkg.VICRegTrainer(vicreg_cfg(pkg), DEV, use_graph=False, seed=21)
    state = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    x = clips(31, 1)[0]
    oracle = vm.oracle_vicreg('R2P1D10T', 8, 32, state)
    want, inv, varl, covl, _, _ = vm.model_loss(oracle, x.cpu().double())
    want.backward()
    tr.optimizer.zero_grad()
    got = tr.model(x)
    got.backward()
    torch.cuda.synchronize()
    got, want = got.detach(), want.detach()
    inner = tr.model.model
    e = dict(loss=abs(float(got) - float(want)) / abs(float(want)))
    for k, mine, ref in (('inv', inner.inv, inv), ('var', inner.var, varl), ('cov', inner.cov, covl)):
        e[k] = abs(float(mine) - float(ref.detach())) / abs(float(ref.detach()))
    print('MEASURED vicreg model loss %.6f vs oracle %.6f: rel err %s' % (float(got), float(want), ' '.join('%s %.3e' % kv for kv in e.items())))
    assert got.dim() == 0 and max(e.values()) < 1e-3, e
    g64 = {n: p.grad for n, p in oracle.named_parameters()}
    got_g = dict(tr.model.named_parameters())
    # A Linear bias in front of a train-mode BatchNorm has a gradient of exactly zero (the column mean removes it): fp64 leaves
    # rounding noise there, which is no reference for a relative error.  Both sides must see (next to) nothing instead.
    dead = ['model.projection.l1.0.bias', 'model.projection.l2.0.bias']
    for n in dead:
        w = n.replace('.bias', '.weight')
        assert float(g64[n].abs().max()) <= 1e-12 * float(g64[w].abs().max())
        assert float(got_g[n].grad.abs().max()) <= 1e-4 * float(got_g[w].grad.abs().max())
    errs = {n: rel(p.grad, g64[n]) for n, p in got_g.items() if n not in dead and g64[n] is not None and g64[n].abs().max() > 0}
    assert len(errs) > 40 and 'model.projection.l3.weight' in errs
    med, p95, worst = check_grad_errors(errs, 'vicreg parameter gradients')
    print('MEASURED vicreg model parameter gradients: median %.2e p95 %.2e worst %.2e over %d tensors' % (med, p95, worst, len(errs)))
    tr.close()


def test_trainer_graph_equals_eager_and_loss_decreases(pkg):
    cfg = vicreg_cfg(pkg, WARMUP_FACTOR=1.0, BASE_LR=0.01)
    x = clips(33, 1)[0]
    runs = {}
    keys = ('loss', 'inv', 'var', 'cov')
    for use_graph in (True, False):
        tr = pkg.VICRegTrainer(cfg, DEV, use_graph=use_graph, seed=7)
        outs = []
        for _ in range(10 if not use_graph else 4):
            out = tr.train_step(x)
            torch.cuda.synchronize()
            assert set(out) >= set(keys)
            outs.append(tuple(out[k].detach().clone() for k in keys))
        assert (tr._segments[0].graph is not None) == use_graph
        runs[use_graph] = outs
        sd = tr.state_dict()
        assert sd['contrast'] is None and 'model_ema' not in sd
        tr.close()
    for ga, ea in zip(runs[True][:4], runs[False][:4]):
        for a, b_ in zip(ga, ea):
            assert torch.equal(bits(a), bits(b_))
    vals = [float(o[0]) for o in runs[False]]
    print('MEASURED vicreg trainer losses on one repeated batch: %s' % ' '.join('%.4f' % v for v in vals))
    assert all(np.isfinite(vals)) and vals[-1] < vals[0]
    lo = [float(v) for v in runs[False][0]]
    assert abs(25.0 * lo[1] + 25.0 * lo[2] + 1.0 * lo[3] - lo[0]) <= 1e-5 * abs(lo[0])


def test_checkpoint_resume_is_exact_and_loads_downstream(pkg):
    import copy
    import classify_model as cm
    from test_gpu_adam import action_cfg, assert_resume_is_exact
    cm.register()
    cfg = vicreg_cfg(pkg)
    a, b_, sd = assert_resume_is_exact(lambda seed: pkg.VICRegTrainer(cfg, DEV, use_graph=False, seed=seed), clips(13, 5),
                                       ('epoch', 'state_dict', 'optimizer', 'contrast'))
    assert sd['contrast'] is None and 'model_ema' not in sd
    assert all(k.startswith(('model.encoder.', 'model.projection.')) for k in sd['state_dict'])
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
    gen = torch.Generator().manual_seed(3)
    bank = [(torch.randn(2, 3, 8, 48, 48, generator=gen), torch.tensor([2 * i, 2 * i + 1])) for i in range(3)]
    query = [(torch.randn(2, 3, 8, 48, 48, generator=gen), torch.tensor(c)) for c in ([2, 0], [7, 5])]
    mon = E.KNNMonitor(cfg, bank, query, 8, k=4, T=0.07, device=DEV)                   # the k-NN feature pass
    res = mon.evaluate(a)
    assert res['count'] == 4 and 0.0 <= res['top1'] <= 100.0 and a.model.training
    assert mon.evaluate({'state_dict': a.state_dict()['state_dict']}) == res          # a checkpoint dict works like the trainer
    feats = E.extract_feature_single(enc.to(DEV), query[0][0].to(DEV), 1, 8)            # the retrieval feature pass
    assert tuple(feats.shape) == (2, enc.feature_dim) and bool(torch.isfinite(feats).all()) and float(feats.abs().max()) > 0
    a.close(), b_.close()


def test_trainer_refusals(pkg):
    register_tiny(pkg)
    for mem in ('simsiam', 'moco', 'simclr', 'barlow'):
        with pytest.raises(ValueError, match='vicreg'):
            pkg.VICRegTrainer(make_cfg(pkg, 'R2P1D10T', mem, 32, 16, 8), DEV)
    with pytest.raises(NotImplementedError, match='one GPU'):
        pkg.VICRegTrainer(vicreg_cfg(pkg), DEV, ctx=pkg.parallel.DistCtx(force_active=True))


def test_lars_step_changes_every_adapted_tensor(pkg):
    tr = pkg.VICRegTrainer(vicreg_cfg(pkg, OPTIMIZER_NAME='LARS', BASE_LR=0.3), DEV, use_graph=False, seed=11)
    assert type(tr.optimizer).__name__ == 'HipLARS'
    before = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
    out = tr.train_step(clips(7, 1)[0])
    torch.cuda.synchronize()
    assert np.isfinite(float(out['loss']))
    adapted = [n for n, p in tr.model.named_parameters() if p.ndim > 1]
    assert len(adapted) > 20 and 'model.projection.l3.weight' in adapted
    for n, p in tr.model.named_parameters():
        assert bool(torch.isfinite(p).all()), n
        if p.ndim > 1:
            assert not torch.equal(p.detach(), before[n]), n
    tr.close()
