"""gca_barlow_fwd / gca_barlow_bwd, ops.barlow_*, lib.memory.BarlowTwinsLoss, the BarlowTwins wrapper and BarlowTwinsTrainer on
the device, against tests/barlow_ref.py (fp64 numpy) and tests/barlow_model.py (the fp64 torch oracle of the model).

Exact inputs (+-1 columns with equal counts, N a power of two, eps = 0, lambda = 2^-7: every quantity is the same number in
fp32 and fp64 under any order of summation, tests/test_barlow_ref.py): stats, cmat, loss[3], rsum, dz1, dz2 bit for bit.

Float inputs (column scales spread 20x, means of a few units, view 2 a noisy copy of view 1; lambda = 0.0051 and 1): loss, on,
off, stats, cmat, rsum, dz1, dz2 within 1e-5 (max-norm relative) of the fp64 specification on the same fp32 inputs, the suite's
per-op bar; the unfused fp32 torch chain sits at up to 2.1e-6 on the gradients of these inputs (tests/test_barlow_ref.py
holds it to 3e-6), while each of the wrong variants of tests/barlow_ref.py misses by 1e-3 or more.

Measured on an MI355X (printed as `MEASURED barlow ...`), worst over the cases:
    exact inputs   every output equals fp64 at all five sizes (e.g. N = 16, D = 128: loss 12.39990234375, on 4, off 1075.1875)
    float inputs   loss 1.49e-7 (256 x 512, lambda 0.0051)   on 1.79e-7   off 7.42e-8   stats 1.82e-7   cmat 7.94e-7 (256 x 512)
                   rsum 2.50e-6 (256 x 512, lambda 0.0051)   dz1 2.03e-6 (40 x 512, lambda 1)   dz2 2.72e-6 (256 x 512, lambda 0.0051)
                   pointers offset by 4 bytes (33 x 130): 9.24e-7
                   long batch (4100 x 40, lambda 0.0051): cmat 1.22e-6, rsum 4.14e-6, dz1 2.17e-6, dz2 2.09e-6       [bar 1e-5]
    model          loss of BarlowTwins.forward against the fp64 oracle: 1.28e-6 relative (on 1.29e-6, off 4.93e-7)    [bar 1e-3]
                   parameter gradients: median 1.30e-5, 95th percentile 1.91e-5, worst 2.24e-5 over 70 tensors
    trainer        loss on one repeated batch, SGD lr 0.01: 31.70 47.67 36.10 37.58 7.04 3.86 3.69 4.39 3.84 3.86
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import barlow_ref as br                  # noqa: E402
import barlow_model as bm                # noqa: E402
from parity import check_grad_errors, make_cfg, register_tiny, rel           # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = -1
BAR = 1e-5
_REF = {}


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def float_ref(N, D, lambd, seed=0):
    """The fp64 specification on the float inputs: computed once per case, shared, left unchanged."""
    key = (N, D, lambd, seed)
    if key not in _REF:
        z1, z2 = br.float_inputs(N, D, seed)
        _REF[key] = (z1, z2, br.barlow(z1, z2, np.float32(lambd), eps=np.float32(1e-5)))
    return _REF[key]


def errors(got, ref):
    """max-norm relative errors of (loss3, stats, cmat, rsum, dz1, dz2) on the device against a barlow_ref dict."""
    loss3, stats, cmat, rsum, dz1, dz2 = got
    l3 = loss3.cpu().numpy().astype(np.float64)
    e = {k: abs(l3[i] - ref[k]) / max(abs(ref[k]), 1e-30) for i, k in enumerate(('loss', 'on', 'off')) if ref[k] != 0}
    for k, t, r in (('stats', stats, ref['stats']), ('cmat', cmat, ref['C']), ('rsum', rsum, ref['rsum']), ('dz1', dz1, ref['dz1']),
                    ('dz2', dz2, ref['dz2'])):
        e[k] = rel(t, torch.from_numpy(np.ascontiguousarray(r)))
    return e


# ----------------------------------------------------------------------------- 1. the kernels against the specification
@pytest.mark.parametrize('N,D', br.EXACT_CASES)
def test_exact_inputs_bit_for_bit(pkg, N, D):
    ops = pkg.engine.ops
    z1, z2 = br.exact_inputs(N, D)
    ref = br.barlow(z1, z2, br.EXACT_LAMBDA, eps=0.0)
    a, b = dev(z1), dev(z2)
    loss3, stats, cmat, rsum = ops.barlow_fwd(a, b, br.EXACT_LAMBDA, 0.0)
    dz1, dz2 = ops.barlow_bwd(a, b, stats, cmat, rsum, br.EXACT_LAMBDA)
    torch.cuda.synchronize()
    want = dict(stats=ref['stats'], cmat=ref['C'], rsum=ref['rsum'], dz1=ref['dz1'], dz2=ref['dz2'],
                loss3=np.array([ref['loss'], ref['on'], ref['off']]))
    got = dict(stats=stats, cmat=cmat, rsum=rsum, dz1=dz1, dz2=dz2, loss3=loss3)
    for k in want:
        g = got[k].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == want[k].shape, k
        assert np.array_equal(g.astype(np.float64), want[k]), (k, np.abs(g - want[k]).max())
    print('MEASURED barlow exact N=%d D=%d: loss %.10g on %.10g off %.10g, every output equals fp64' % ((N, D) + tuple(loss3.tolist())))


@pytest.mark.parametrize('lambd', br.FLOAT_LAMBDAS)
@pytest.mark.parametrize('N,D', br.FLOAT_CASES)
def test_float_inputs(pkg, N, D, lambd):
    ops = pkg.engine.ops
    z1, z2, ref = float_ref(N, D, lambd)
    a, b = dev(z1), dev(z2)
    loss3, stats, cmat, rsum = ops.barlow_fwd(a, b, lambd)
    dz1, dz2 = ops.barlow_bwd(a, b, stats, cmat, rsum, lambd)
    torch.cuda.synchronize()
    e = errors((loss3, stats, cmat, rsum, dz1, dz2), ref)
    print('MEASURED barlow float N=%d D=%d lambda=%g: rel_err %s' % (N, D, lambd, ' '.join('%s %.2e' % kv for kv in e.items())))
    assert max(e.values()) <= BAR, e


def test_long_batch(pkg):
    """N past the 2048 rows after which the forward moves its accumulator tile aside, and a multiple of nothing: the
    reduction over N (column sums of 4100 terms, C over 129 chunks) is held to the same bar."""
    ops = pkg.engine.ops
    N, D, lambd = 4100, 40, 0.0051
    z1, z2, ref = float_ref(N, D, lambd)
    a, b = dev(z1), dev(z2)
    loss3, stats, cmat, rsum = ops.barlow_fwd(a, b, lambd)
    dz1, dz2 = ops.barlow_bwd(a, b, stats, cmat, rsum, lambd)
    torch.cuda.synchronize()
    e = errors((loss3, stats, cmat, rsum, dz1, dz2), ref)
    print('MEASURED barlow float N=%d D=%d lambda=%g: rel_err %s' % (N, D, lambd, ' '.join('%s %.2e' % kv for kv in e.items())))
    assert max(e.values()) <= BAR, e


def test_pointers_offset_by_four_bytes(pkg):
    """Nothing assumes 16-byte alignment: inputs, saved state and outputs all start 4 bytes into their buffers."""
    N, D, lambd = 33, 130, 0.0051
    z1, z2, ref = float_ref(N, D, lambd)
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
    loss3, stats, cmat, rsum, dz1, dz2 = off((3,)), off((4, D)), off((D, D)), off((2, D)), off((N, D)), off((N, D))
    ws = torch.empty(lib.gca_barlow_ws_bytes(N, D) + 4, dtype=torch.uint8, device=DEV)
    p = H.ptr
    assert lib.gca_barlow_fwd(p(a), p(b), N, D, lambd, 1e-5, p(stats), p(cmat), p(rsum), p(loss3), p(ws) + 4, H.stream()) == 0
    assert lib.gca_barlow_bwd(p(a), p(b), p(stats), p(cmat), p(rsum), N, D, lambd, None, 1.0, p(dz1), p(dz2), p(ws) + 4,
                              H.stream()) == 0
    torch.cuda.synchronize()
    e = errors((loss3, stats, cmat, rsum, dz1, dz2), ref)
    print('MEASURED barlow offset pointers N=%d D=%d: worst rel_err %.2e' % (N, D, max(e.values())))
    assert max(e.values()) <= BAR, e


@pytest.mark.parametrize('N,D', [(33, 130), (64, 128), (40, 512)])
def test_deterministic(pkg, N, D):
    ops = pkg.engine.ops
    z1, z2 = (dev(z) for z in br.float_inputs(N, D, seed=3))
    outs = []
    for _ in range(2):
        loss3, stats, cmat, rsum = ops.barlow_fwd(z1, z2, 0.0051)
        outs.append((loss3, stats, cmat, rsum) + ops.barlow_bwd(z1, z2, stats, cmat, rsum, 0.0051))
    torch.cuda.synchronize()
    for x, y in zip(*outs):
        assert torch.equal(bits(x), bits(y))


@pytest.mark.parametrize('N,D', [(33, 130), (64, 128)])
def test_gradient_scale(pkg, N, D):
    ops = pkg.engine.ops
    z1, z2 = (dev(z) for z in br.float_inputs(N, D, seed=5))
    _, stats, cmat, rsum = ops.barlow_fwd(z1, z2, 0.0051)
    saved = (z1, z2, stats, cmat, rsum, 0.0051)
    one = ops.barlow_bwd(*saved)
    scaled = ops.barlow_bwd(*saved, gscale_dev=torch.tensor([1024.0, 7.0], device=DEV))
    half = ops.barlow_bwd(*saved, gscale_host=0.5)
    both = ops.barlow_bwd(*saved, gscale_dev=torch.tensor([3.0], device=DEV), gscale_host=-0.7)
    torch.cuda.synchronize()
    for v in range(2):
        assert float(one[v].abs().max()) > 0
        assert rel(scaled[v], one[v] * 1024.0) <= 1e-6 and rel(half[v], one[v] * 0.5) <= 1e-6
        assert rel(both[v], one[v].double() * (3.0 * np.float64(np.float32(-0.7)))) <= 1e-6


def test_refused_arguments_touch_nothing(pkg):
    lib, H = pkg._hip.lib, pkg._hip
    z1, z2 = (dev(z) for z in br.float_inputs(8, 8))
    SENT = 12345.0
    stats, cmat, rsum, loss, dz1, dz2 = (torch.full((n,), SENT, device=DEV) for n in (4 * 8, 8 * 8, 2 * 8, 3, 8 * 8, 8 * 8))
    good = pkg.engine.ops.barlow_fwd(z1, z2, 0.005)
    ws = torch.empty(max(lib.gca_barlow_ws_bytes(8, 8), 1 << 16), dtype=torch.uint8, device=DEV)
    p = H.ptr
    nan, inf = float('nan'), float('inf')

    def fwd(a=p(z1), b=p(z2), N=8, D=8, lam=0.005, eps=1e-5, s=p(stats), c=p(cmat), r=p(rsum), lo=p(loss), w=p(ws)):
        return lib.gca_barlow_fwd(a, b, N, D, lam, eps, s, c, r, lo, w, H.stream())

    def bwd(a=p(z1), b=p(z2), N=8, D=8, lam=0.005, s=p(good[1]), c=p(good[2]), r=p(good[3]), gs=1.0, d1=p(dz1), d2=p(dz2), w=p(ws)):
        return lib.gca_barlow_bwd(a, b, s, c, r, N, D, lam, None, gs, d1, d2, w, H.stream())

    shared = (dict(N=1), dict(N=0), dict(N=-2), dict(N=65537, D=1), dict(D=0), dict(D=-1), dict(D=8193), dict(N=1 << 31, D=1),
              dict(lam=-1.0), dict(lam=inf), dict(lam=nan), dict(a=None), dict(b=None), dict(s=None), dict(c=None), dict(r=None),
              dict(w=None))
    for f in (fwd, bwd):
        for kw in shared:
            assert f(**kw) == EINVAL, (f.__name__, kw)
    for kw in (dict(eps=-1e-5), dict(eps=inf), dict(eps=nan), dict(lo=None)):
        assert fwd(**kw) == EINVAL, kw
    for kw in (dict(gs=inf), dict(gs=-inf), dict(gs=nan), dict(d1=None), dict(d2=None)):
        assert bwd(**kw) == EINVAL, kw
    assert lib.gca_barlow_ws_bytes(1, 8) == -1 and lib.gca_barlow_ws_bytes(8, 8193) == -1
    torch.cuda.synchronize()
    for t in (stats, cmat, rsum, loss, dz1, dz2):
        assert float(t.min()) == SENT == float(t.max())
    # and the accepted calls write all of their outputs
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    for t in (stats, cmat, rsum, loss, dz1, dz2):
        assert float((t == SENT).sum()) == 0


def test_ops_refuse_what_the_entry_refuses(pkg):
    ops = pkg.engine.ops
    z = torch.zeros(4, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.barlow_fwd(torch.zeros(1, 8, device=DEV), torch.zeros(1, 8, device=DEV), 0.005)
    with pytest.raises(ValueError):
        ops.barlow_fwd(z, z, float('nan'))
    with pytest.raises(ValueError):
        ops.barlow_bwd(z, z, torch.zeros(4, 8, device=DEV), torch.zeros(8, 8, device=DEV), torch.zeros(2, 7, device=DEV), 0.005)


def test_capturable_in_a_graph(pkg):
    """Forward and backward inside one captured graph: replays track the static inputs and equal the eager bits."""
    ops = pkg.engine.ops
    N, D, lambd = 40, 512, 0.0051
    z1, z2, _ = float_ref(N, D, lambd)
    s1, s2 = dev(z1).clone(), dev(z2).clone()
    l3, stats, cmat, rsum = ops.barlow_fwd(s1, s2, lambd)
    eager = (l3, cmat) + ops.barlow_bwd(s1, s2, stats, cmat, rsum, lambd)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gl3, gstats, gcmat, grsum = ops.barlow_fwd(s1, s2, lambd)
        gdz = ops.barlow_bwd(s1, s2, gstats, gcmat, grsum, lambd)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, (gl3, gcmat) + gdz):
        assert torch.equal(bits(x), bits(y))
    n1, n2, ref = float_ref(N, D, lambd, seed=9)
    s1.copy_(dev(n1))
    s2.copy_(dev(n2))
    g.replay()
    torch.cuda.synchronize()
    e = errors((gl3, gstats, gcmat, grsum) + gdz, ref)
    assert max(e.values()) <= BAR, e
    g.reset()


# ----------------------------------------------------------------------------- 2. the module
def test_module_forward_backward(pkg):
    import importlib
    BarlowTwinsLoss = importlib.import_module(pkg.__name__ + '.lib.memory.barlow').BarlowTwinsLoss
    N, D, lambd = 33, 130, 0.0051
    z1, z2, _ = float_ref(N, D, lambd)
    ref = br.barlow(z1, z2, np.float32(lambd), eps=np.float32(1e-5), g=3.0)
    t1, t2 = dev(z1).requires_grad_(True), dev(z2).requires_grad_(True)
    crit = BarlowTwinsLoss(lambd)
    loss = crit(t1, t2)
    assert loss.dim() == 0 and abs(float(loss.detach()) - ref['loss']) <= BAR * abs(ref['loss'])
    (loss * 3.0).backward()
    torch.cuda.synchronize()
    assert rel(t1.grad, torch.from_numpy(ref['dz1'])) <= BAR and rel(t2.grad, torch.from_numpy(ref['dz2'])) <= BAR
    assert crit.on_diag.is_cuda and crit.on_diag.dim() == 0 and crit.off_diag.dim() == 0
    assert abs(float(crit.on_diag) - ref['on']) <= BAR * ref['on'] and abs(float(crit.off_diag) - ref['off']) <= BAR * ref['off']


# ----------------------------------------------------------------------------- 3. model and trainer
CLIP = (8, 6, 8, 48, 48)


def clips(seed, n=4):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*CLIP, generator=gen).to(DEV) for _ in range(n)]


def barlow_cfg(pkg, **solver):
    register_tiny(pkg)
    return make_cfg(pkg, 'R2P1D10T', 'barlow', 32, 16, 8, **solver)


def test_model_against_the_fp64_oracle(pkg):
    tr = pkg.BarlowTwinsTrainer(barlow_cfg(pkg), DEV, use_graph=False, seed=21)
    state = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    x = clips(31, 1)[0]
    oracle = bm.oracle_barlow('R2P1D10T', 8, 32, state)
    want, on, off, _, _ = bm.model_loss(oracle, x.cpu().double(), 0.0051)
    want.backward()
    tr.optimizer.zero_grad()
    got = tr.model(x)
    got.backward()
    torch.cuda.synchronize()
    got, want = got.detach(), want.detach()
    err = abs(float(got) - float(want)) / abs(float(want))
    inner = tr.model.model
    on, off = float(on.detach()), float(off.detach())
    e_on, e_off = abs(float(inner.on_diag) - on) / on, abs(float(inner.off_diag) - off) / off
    print('MEASURED barlow model loss %.6f vs oracle %.6f: rel err %.3e (on %.3e, off %.3e)' % (float(got), float(want), err, e_on, e_off))
    assert got.dim() == 0 and err < 1e-3 and e_on < 1e-3 and e_off < 1e-3
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
    med, p95, worst = check_grad_errors(errs, 'barlow parameter gradients')
    print('MEASURED barlow model parameter gradients: median %.2e p95 %.2e worst %.2e over %d tensors' % (med, p95, worst, len(errs)))
    tr.close()


def test_trainer_graph_equals_eager_and_loss_decreases(pkg):
    cfg = barlow_cfg(pkg, WARMUP_FACTOR=1.0, BASE_LR=0.01)
    x = clips(33, 1)[0]
    runs = {}
    for use_graph in (True, False):
        tr = pkg.BarlowTwinsTrainer(cfg, DEV, use_graph=use_graph, seed=7)
        outs = []
        for _ in range(10 if not use_graph else 4):
            out = tr.train_step(x)
            torch.cuda.synchronize()
            assert set(out) >= {'loss', 'on_diag', 'off_diag'}
            outs.append(tuple(out[k].detach().clone() for k in ('loss', 'on_diag', 'off_diag')))
        assert (tr._segments[0].graph is not None) == use_graph
        if use_graph:
            runs['flat'] = tr.arena.flat.detach().clone()
        runs[use_graph] = outs
        sd = tr.state_dict()
        assert sd['contrast'] is None and 'model_ema' not in sd
        tr.close()
    for ga, ea in zip(runs[True][:4], runs[False][:4]):
        for a, b_ in zip(ga, ea):
            assert torch.equal(bits(a), bits(b_))
    vals = [float(o[0]) for o in runs[False]]
    print('MEASURED barlow trainer losses on one repeated batch: %s' % ' '.join('%.4f' % v for v in vals))
    assert all(np.isfinite(vals)) and vals[-1] < vals[0]
    lo = runs[False][0]
    assert abs(float(lo[1]) + 0.0051 * float(lo[2]) - float(lo[0])) <= 1e-5 * abs(float(lo[0]))


def test_checkpoint_resume_is_exact_and_loads_downstream(pkg):
    import copy
    import classify_model as cm
    from test_gpu_adam import action_cfg, assert_resume_is_exact
    cm.register()
    cfg = barlow_cfg(pkg)
    a, b_, sd = assert_resume_is_exact(lambda seed: pkg.BarlowTwinsTrainer(cfg, DEV, use_graph=False, seed=seed), clips(13, 5),
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
    mon = E.KNNMonitor(cfg, bank, query, 8, k=4, T=0.07, device=DEV)
    res = mon.evaluate(a)
    assert res['count'] == 4 and 0.0 <= res['top1'] <= 100.0 and a.model.training
    assert mon.evaluate({'state_dict': a.state_dict()['state_dict']}) == res          # a checkpoint dict works like the trainer
    a.close(), b_.close()


def test_trainer_refusals(pkg):
    register_tiny(pkg)
    for mem in ('simsiam', 'moco', 'simclr'):
        with pytest.raises(ValueError, match='barlow'):
            pkg.BarlowTwinsTrainer(make_cfg(pkg, 'R2P1D10T', mem, 32, 16, 8), DEV)
    with pytest.raises(NotImplementedError, match='one GPU'):
        pkg.BarlowTwinsTrainer(barlow_cfg(pkg), DEV, ctx=pkg.parallel.DistCtx(force_active=True))


def test_lars_step_changes_every_adapted_tensor(pkg):
    tr = pkg.BarlowTwinsTrainer(barlow_cfg(pkg, OPTIMIZER_NAME='LARS', BASE_LR=0.3), DEV, use_graph=False, seed=11)
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
