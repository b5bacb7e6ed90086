"""gca_ressl_fwd / gca_ressl_bwd, ops.ressl_*, lib.memory.ReSSLLoss and ReSSLTrainer on the device, against tests/ressl_ref.py
(fp64 numpy) and tests/ressl_model.py (the fp64 torch oracle of a training step, EMA teacher and queue update included).

Bars.  row_lse, row_loss, loss and ent: within 1e-5 max(|s|, |t|), the suite's bar on the logit scale (a relative bar on the loss
would be wrong: lse_s - sum Pt s cancels).  dq: max error within 1e-5 coef max(|O_s|inf, |O_t|inf) of the fp64 values -- the scale
of the two terms, not of their difference.  The same formulas in plain fp32 numpy stay below 3.3e-6 of those scales on every one
of these inputs (tests/test_ressl_ref.py prints it), and each wrong variant there misses the bars by more than 100x.

Measured on an MI355X (printed as `MEASURED ressl ...`), worst over the cases, in units of the bar's scale:
    fast path      dq 2.81e-6 (overflow, N = 97, D = 256, K = 1000, Ts 0.1, Tt 0.04); row_lse 9.22e-7, row_loss 1.08e-6, ent 6.26e-7
                   (all easy, N = 97, D = 256, K = 1000, Ts = Tt = 0.2); loss 3.51e-7 (easy, N = 1, K = 65)    [bar 1e-5]
    generic path   dq 1.57e-6 (overflow, N = 33, D = 130, K = 200, Ts 0.1, Tt 0.04); row_lse 4.70e-7, row_loss 5.01e-7, loss 2.24e-7
                   (easy, same shape, Ts = Tt = 0.2); unaligned q, k or Q at (33, 128, 100): dq 5.66e-7, the aligned run's    [bar 1e-5]
    exact          K = 1: loss, ent, dq exactly 0; q == k at one temperature: dq exactly 0, loss == ent bit for bit (both paths)
    model          loss against the fp64 oracle 8.2e-7 relative, q rows 4.4e-6, k rows 4.1e-6; parameter gradients median 7.1e-6,
                   worst 1.1e-5 over 67 tensors    [bar 1e-3]
    trainer        three losses 1.449449 2.077719 2.710382 against the oracle's 1.449450 2.077721 2.710383; after three steps
                   parameters 1.5e-7, teacher 2.5e-7, queue 5.0e-6    [bar 1e-3]
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ressl_ref as rr                   # noqa: E402
from parity import make_cfg, register_tiny, rel           # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = -1
BAR = rr.BAR


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a) if a.is_floating_point() else a, bits(b) if b.is_floating_point() else b)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def f32(x):
    return float(np.float32(x))


def aligned(*ts):
    return all(t.data_ptr() % 16 == 0 for t in ts)


def c_path(pkg, which, N, D, K, al):
    w, s = C.c_int32(-1), C.c_int32(-1)
    rc = getattr(pkg._hip.lib, 'gca_ressl_%s_path' % which)(N, D, K, int(al), C.addressof(w), C.addressof(s))
    return ('generic', 'fast')[rc] if rc in (0, 1) else rc, w.value, s.value


_REF = {}


def reference(kind, N, D, K, Ts, Tt, g=1.0):
    """The inputs of a case and their fp64 values, computed once."""
    key = (kind, N, D, K, Ts, Tt, g)
    if key not in _REF:
        q, k, Q = rr.inputs(kind, N, D, K)
        _REF[key] = (q, k, Q, rr.ressl(q, k, Q, f32(1.0 / Ts), f32(1.0 / Tt), g))
    return _REF[key]


def errors(ref, loss, row_lse, row_loss, dq):
    """Errors in units of the scales of the bars -> dict."""
    N = ref['lse_s'].shape[0]
    lse = row_lse.double().cpu().numpy()
    e = dict(lse=max(np.abs(lse[:N] - ref['lse_s']).max(), np.abs(lse[N:] - ref['lse_t']).max()) / ref['smax'],
             row_loss=np.abs(row_loss.double().cpu().numpy() - ref['row_loss']).max() / ref['smax'],
             loss=abs(float(loss[0]) - ref['loss']) / ref['smax'], ent=abs(float(loss[1]) - ref['ent']) / ref['smax'])
    if dq is not None:
        e['dq'] = np.abs(dq.double().cpu().numpy() - ref['dq']).max() / ref['oscale']
    return {n: float(v) for n, v in e.items()}


def run_pair(pkg, qd, kd, Qd, Ts, Tt, **kw):
    ops = pkg.engine.ops
    loss, row_lse, row_loss = ops.ressl_fwd(qd, kd, Qd, 1.0 / Ts, 1.0 / Tt)
    dq = ops.ressl_bwd(qd, kd, Qd, row_lse, 1.0 / Ts, 1.0 / Tt, **kw)
    torch.cuda.synchronize()
    return loss, row_lse, row_loss, dq


# ----------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize('N,D', [(5, 32), (33, 130)])
def test_one_anchor_gives_exactly_zero(pkg, N, D):
    """K = 1: both softmaxes are 1 on the one column, so loss, ent and dq are exactly 0 (fast and generic path)."""
    q, k, Q = rr.inputs('overflow', N, D, 1)
    loss, row_lse, row_loss, dq = run_pair(pkg, dev(q), dev(k), dev(Q), 0.1, 0.04)
    assert float(loss[0]) == 0.0 and float(loss[1]) == 0.0 and not bool(row_loss.any()) and not bool(dq.any())
    s = f32(10.0) * (q.astype(np.float64) @ Q.astype(np.float64).T)[:, 0]
    assert np.abs(row_lse[:N].double().cpu().numpy() - s).max() <= BAR * np.abs(s).max()


@pytest.mark.parametrize('N,D,K,path', [(33, 128, 100, 'fast'), (64, 256, 3075, 'fast'), (33, 130, 200, 'generic')])
def test_student_equal_to_teacher_gives_exactly_zero_gradient(pkg, N, D, K, path):
    """q bitwise k at one temperature: both sides of the backward pass run the same instructions on the same numbers, so dq is
    exactly 0, and the loss IS the teacher's entropy, bit for bit."""
    _, k, Q = rr.inputs('easy', N, D, K)
    kd, Qd = dev(k), dev(Q)
    qd = kd.clone()
    assert c_path(pkg, 'bwd', N, D, K, aligned(qd, kd, Qd))[0] == path
    loss, row_lse, row_loss, dq = run_pair(pkg, qd, kd, Qd, 0.2, 0.2)
    assert not bool(dq.any())
    assert same(loss[0], loss[1]) and same(row_lse[:N], row_lse[N:])
    ref = rr.ressl(k, k, Q, f32(5.0), f32(5.0))
    assert abs(float(loss[0]) - ref['ent']) <= BAR * ref['smax'] and ref['ent'] > 1.0


# ----------------------------------------------------------------------------- 2. float cases against fp64
@pytest.mark.parametrize('kind', rr.KINDS)
@pytest.mark.parametrize('Ts,Tt', rr.TEMPS)
@pytest.mark.parametrize('case,path', list(zip(rr.FLOAT_CASES, rr.FLOAT_PATHS)), ids=['N%d-D%d-K%d' % c for c in rr.FLOAT_CASES])
def test_float_inputs_against_fp64(pkg, case, path, Ts, Tt, kind):
    N, D, K = case
    q, k, Q, ref = reference(kind, N, D, K, Ts, Tt)
    qd, kd, Qd = dev(q), dev(k), dev(Q)
    al = aligned(qd, kd, Qd)
    assert c_path(pkg, 'fwd', N, D, K, al) == rr.path(N, D, K, al, 1)[:3] and rr.path(N, D, K, al, 1)[0] == path
    assert c_path(pkg, 'bwd', N, D, K, al) == rr.path(N, D, K, al, 2)[:3]
    loss, row_lse, row_loss, dq = run_pair(pkg, qd, kd, Qd, Ts, Tt)
    assert tuple(loss.shape) == (2,) and tuple(row_lse.shape) == (2 * N,) and tuple(row_loss.shape) == (N,) and tuple(dq.shape) == (N, D)
    e = errors(ref, loss, row_lse, row_loss, dq)
    print('MEASURED ressl %s N=%d D=%d K=%d Ts=%g Tt=%g (%s): %s' % (kind, N, D, K, Ts, Tt, path, ' '.join('%s %.3e' % kv for kv in e.items())))
    assert all(bool(torch.isfinite(t).all()) for t in (loss, row_lse, row_loss, dq))
    assert max(e.values()) <= BAR, e


@pytest.mark.parametrize('which', ['q', 'k', 'Q'])
def test_unaligned_operands_take_the_generic_path(pkg, which):
    N, D, K = 33, 128, 100
    Ts, Tt = rr.TEMPS[0]
    q, k, Q, ref = reference('easy', N, D, K, Ts, Tt)
    ts = {}
    for name, a in (('q', q), ('k', k), ('Q', Q)):
        if name == which:                                                       # offset by one float
            buf = torch.empty(a.size + 1, device=DEV)
            ts[name] = buf[1:].view(a.shape).copy_(dev(a))
        else:
            ts[name] = dev(a)
    al = aligned(ts['q'], ts['k'], ts['Q'])
    assert not al and ts[which].is_contiguous()
    assert c_path(pkg, 'fwd', N, D, K, al)[:2] == ('generic', 1) and c_path(pkg, 'fwd', N, D, K, True)[:2] == ('fast', 4)
    loss, row_lse, row_loss, dq = run_pair(pkg, ts['q'], ts['k'], ts['Q'], Ts, Tt)
    e = errors(ref, loss, row_lse, row_loss, dq)
    print('MEASURED ressl unaligned %s N=%d D=%d K=%d: %s' % (which, N, D, K, ' '.join('%s %.3e' % kv for kv in e.items())))
    assert max(e.values()) <= BAR, e


@pytest.mark.parametrize('N,D,K', rr.REPEAT_CASES)
def test_two_runs_are_bitwise_equal(pkg, N, D, K):
    q, k, Q = (dev(a) for a in rr.inputs('hard', N, D, K))
    a = run_pair(pkg, q, k, Q, 0.1, 0.04)
    junk = torch.randn(1 << 20, device=DEV)                                     # (the workspace is reused; the allocator moves on)
    b_ = run_pair(pkg, q, k, Q, 0.1, 0.04)
    del junk
    for x, y in zip(a, b_):
        assert same(x, y)


def test_gradient_scale_scales_dq_and_nothing_else(pkg):
    N, D, K = 33, 128, 100
    Ts, Tt = rr.TEMPS[0]
    q, k, Q, ref = reference('easy', N, D, K, Ts, Tt, g=-6.0)
    qd, kd, Qd = dev(q), dev(k), dev(Q)
    base = run_pair(pkg, qd, kd, Qd, Ts, Tt)
    gs = torch.tensor([4.0, 123.0], device=DEV)                                 # only element 0 is read
    got = run_pair(pkg, qd, kd, Qd, Ts, Tt, gscale_dev=gs, gscale_host=-1.5)
    for x, y in zip(base[:3], got[:3]):
        assert same(x, y)
    assert np.abs(got[3].double().cpu().numpy() - ref['dq']).max() <= BAR * ref['oscale']
    assert np.abs(base[3].double().cpu().numpy() * -6.0 - ref['dq']).max() <= BAR * ref['oscale']
    assert rel(got[3], base[3].double() * -6.0) <= 1e-6                          # (power-of-two-free scale: rounding only)
    assert float(gs[1]) == 123.0


# ----------------------------------------------------------------------------- 3. refusals
def test_refused_arguments_leave_the_outputs_untouched(pkg):
    lib = pkg._hip.lib
    N, D, K = 4, 8, 6
    SENT = 7.5
    q, k = torch.randn(N, D, device=DEV), torch.randn(N, D, device=DEV)
    Q = torch.randn(K, D, device=DEV)
    lse, rl, out, dq = (torch.full((n,), SENT, device=DEV) for n in (2 * N, N, 2, N * D))
    ws = torch.full((1 << 16,), SENT, device=DEV)
    nf, nb = lib.gca_ressl_fwd_ws_bytes(N, D, K), lib.gca_ressl_bwd_ws_bytes(N, D, K)
    p = lambda t: t.data_ptr()

    def fwd(**kw):
        a = dict(q=p(q), k=p(k), Q=p(Q), N=N, D=D, K=K, its=10.0, itt=25.0, lse=p(lse), rl=p(rl), out=p(out), ws=p(ws), wb=nf)
        a.update(kw)
        return lib.gca_ressl_fwd(a['q'], a['k'], a['Q'], a['N'], a['D'], a['K'], a['its'], a['itt'], a['lse'], a['rl'], a['out'],
                                 a['ws'], a['wb'], None)

    def bwd(**kw):
        a = dict(q=p(q), k=p(k), Q=p(Q), lse=p(lse), N=N, D=D, K=K, its=10.0, itt=25.0, dq=p(dq), ws=p(ws), wb=nb)
        a.update(kw)
        return lib.gca_ressl_bwd(a['q'], a['k'], a['Q'], a['lse'], a['N'], a['D'], a['K'], a['its'], a['itt'], None, 1.0, a['dq'],
                                 a['ws'], a['wb'], None)
    for kw in (dict(N=0), dict(N=65537), dict(D=0), dict(K=0), dict(K=2 ** 31), dict(its=0.0), dict(its=float('nan')), dict(itt=float('inf')),
               dict(itt=-1.0), dict(q=None), dict(Q=None), dict(lse=None), dict(rl=None), dict(out=None), dict(ws=None), dict(wb=nf - 1),
               dict(rl=p(lse) + 4), dict(out=p(rl)), dict(lse=p(q))):
        assert fwd(**kw) == EINVAL, kw
    for kw in (dict(N=0), dict(D=0), dict(K=0), dict(its=float('inf')), dict(itt=0.0), dict(k=None), dict(lse=None), dict(dq=None),
               dict(ws=None), dict(wb=nb - 1), dict(dq=p(q)), dict(dq=p(Q) + 4), dict(dq=p(lse))):
        assert bwd(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    for t in (lse, rl, out, dq, ws):
        assert float(t.min()) == SENT == float(t.max())
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    ref = rr.ressl(q.cpu().numpy(), k.cpu().numpy(), Q.cpu().numpy(), 10.0, 25.0)
    assert abs(float(out[0]) - ref['loss']) <= BAR * ref['smax']
    assert np.abs(dq.view(N, D).double().cpu().numpy() - ref['dq']).max() <= BAR * ref['oscale']


# ----------------------------------------------------------------------------- 4. the step in a graph; the module
def eager_step(ops, q, k, all_k, Q, ptr_dev, K, inv_Ts, inv_Tt):
    loss, row_lse, row_loss = ops.ressl_fwd(q, k, Q, inv_Ts, inv_Tt)
    dq = ops.ressl_bwd(q, k, Q, row_lse, inv_Ts, inv_Tt)
    ops.queue_enqueue(Q, all_k, 0, ptr_dev=ptr_dev)
    ops.queue_advance(ptr_dev, all_k.shape[0], K)
    return loss, row_lse, row_loss, dq


def test_step_capturable_in_a_graph(pkg):
    """Forward, backward, enqueue and advance in ONE captured graph: two replays equal two eager steps bit for bit, and follow
    the specification -- the second step sees the first step's rows (K = 10, N = 4)."""
    ops = pkg.engine.ops
    N, D, K, inv_Ts, inv_Tt = 4, 32, 10, 10.0, 25.0
    q, k, all_k, Q0 = (dev(x) for x in rr.step_inputs(N, D, K, seed=1))
    runs = {}
    for captured in (False, True):
        Q, ptr_dev = Q0.clone(), torch.zeros(1, dtype=torch.long, device=DEV)
        steps = []
        if captured:
            eager_step(ops, q, k, all_k, Q.clone(), ptr_dev.clone(), K, inv_Ts, inv_Tt)     # workspaces exist before the capture
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                outs = eager_step(ops, q, k, all_k, Q, ptr_dev, K, inv_Ts, inv_Tt)
        for _ in range(2):
            if captured:
                g.replay()
            else:
                outs = eager_step(ops, q, k, all_k, Q, ptr_dev, K, inv_Ts, inv_Tt)
            torch.cuda.synchronize()
            steps.append(tuple(o.clone() for o in outs) + (Q.clone(), ptr_dev.clone()))
        runs[captured] = steps
        if captured:
            g.reset()
    for a, b_ in zip(runs[True], runs[False]):
        for x, y in zip(a, b_):
            assert same(x, y)
    Qn, index = Q0.cpu().numpy(), 0
    for st in runs[True]:
        ref = rr.ressl(q.cpu().numpy(), k.cpu().numpy(), Qn, inv_Ts, inv_Tt)
        assert max(errors(ref, st[0], st[1], st[2], st[3]).values()) <= BAR
        Qn, index = rr.enqueue(Qn, all_k.cpu().numpy(), index)
        assert np.array_equal(st[4].cpu().numpy(), Qn) and int(st[5]) == index
    assert index == 8 and not same(runs[True][0][0], runs[True][1][0])


def test_module_forward_backward_and_queue(pkg):
    """Loss and q.grad come from the PRE-enqueue queue; the enqueued rows and the pointer are RGBMoCo's; k gets nothing."""
    ReSSLLoss = importlib.import_module(pkg.__name__ + '.lib.memory.ressl').ReSSLLoss
    RGBMoCo = importlib.import_module(pkg.__name__ + '.lib.memory.mem_moco').RGBMoCo
    N, D, K, Ts, Tt = 8, 64, 20, 0.1, 0.04
    qn, kn, akn, Qn = rr.step_inputs(N, D, K, seed=2)
    crit, moco = ReSSLLoss(D, K, Ts, Tt).to(DEV), RGBMoCo(D, K, 0.07).to(DEV)
    crit.memory.copy_(dev(Qn))
    moco.memory.copy_(dev(Qn))
    index = 0
    for step in range(3):
        use_all_k = step != 1
        ref = rr.ressl(qn, kn, Qn, 1.0 / Ts, 1.0 / Tt, g=3.0)
        q, k = dev(qn).requires_grad_(True), dev(kn).requires_grad_(True)
        loss = crit(q, k, all_k=dev(akn) if use_all_k else None)
        moco(q.detach(), k.detach(), all_k=dev(akn) if use_all_k else None)
        assert loss.dim() == 0 and abs(float(loss.detach()) - ref['loss']) <= BAR * ref['smax']
        assert crit.ent.dim() == 0 and abs(float(crit.ent) - ref['ent']) <= BAR * ref['smax']
        assert np.abs(crit.row_loss.double().cpu().numpy() - ref['row_loss']).max() <= BAR * ref['smax']
        (loss * 3.0).backward()
        torch.cuda.synchronize()
        assert np.abs(q.grad.double().cpu().numpy() - ref['dq']).max() <= BAR * ref['oscale']
        assert k.grad is None
        post = rr.ressl(qn, kn, rr.enqueue(Qn, akn if use_all_k else kn, index)[0], 1.0 / Ts, 1.0 / Tt, g=3.0)
        assert abs(float(loss.detach()) - post['loss']) > 100 * BAR * ref['smax']          # the post-enqueue queue would show
        Qn, index = rr.enqueue(Qn, akn if use_all_k else kn, index)
        assert crit.index == index == moco.index and np.array_equal(crit.memory.cpu().numpy(), Qn)
        assert same(crit.memory, moco.memory)
    assert index == 4
    with torch.no_grad():                                                       # no gradient asked: the loss alone
        loss = crit(dev(qn), dev(kn))
    assert not loss.requires_grad and crit.index == 12
    big = torch.zeros(K + 1, D, device=DEV)
    with pytest.raises(ValueError, match='cannot enqueue'):
        crit(dev(qn), dev(kn), all_k=big)
    assert crit.index == 12


# ----------------------------------------------------------------------------- 5. model and trainer
def cpu_state(module):
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def test_model_against_the_fp64_oracle(pkg):
    """The tiny model and its teacher through ReSSLLoss against the oracle: loss, rows and parameter gradients."""
    import ressl_model as rm
    from parity import check_grad_errors
    from test_ressl_ref import ressl_cfg
    ReSSLLoss = importlib.import_module(pkg.__name__ + '.lib.memory.ressl').ReSSLLoss
    tr = pkg.ReSSLTrainer(ressl_cfg(pkg), DEV, use_graph=False, seed=21)
    state = cpu_state(tr.model)
    x = rm.clip_batches(1, seed=31)[0]
    model, ema = rm.oracle_ressl('R2P1D10T', 8, rm.OUT, state)
    Q0 = rm.queue0()
    want, q64, k64 = rm.model_loss(model, ema, x.double(), Q0.double(), rm.TS, rm.TT)
    want.backward()
    crit = ReSSLLoss(rm.OUT, rm.QUEUE_K, rm.TS, rm.TT).to(DEV)
    crit.memory.copy_(Q0.to(DEV))
    tr.optimizer.zero_grad()
    x1, x2 = (v.contiguous() for v in torch.chunk(x.to(DEV), 2, dim=1))
    with torch.no_grad():
        k = tr.model_ema(x2)
    q = tr.model(x1)
    got = crit(q, k)
    got.backward()
    torch.cuda.synchronize()
    e = dict(loss=abs(float(got.detach()) - float(want.detach())) / abs(float(want.detach())), q=rel(q, q64), k=rel(k, k64))
    print('MEASURED ressl model loss %.6f vs oracle %.6f: rel err %s' % (float(got.detach()), float(want.detach()), ' '.join('%s %.3e' % kv for kv in e.items())))
    assert got.dim() == 0 and tuple(q.shape) == (8, rm.OUT) and max(e.values()) < 1e-3, e
    g64 = {n: p.grad for n, p in model.named_parameters()}
    floor = 1e-9 * max(float(g.abs().max()) for g in g64.values() if g is not None)
    errs = {n: rel(p.grad, g64[n]) for n, p in tr.model.named_parameters() if g64[n] is not None and g64[n].abs().max() > floor}
    assert len(errs) > 40
    med, p95, worst = check_grad_errors(errs, 'ressl parameter gradients')
    print('MEASURED ressl model parameter gradients: median %.2e p95 %.2e worst %.2e over %d tensors' % (med, p95, worst, len(errs)))
    tr.close()


def test_trainer_graph_equals_eager_and_follows_the_oracle(pkg):
    """Three steps on three batches: the captured run equals the eager run bit for bit (losses, parameters, teacher, queue,
    pointer), and losses, student parameters, teacher state and queue follow the fp64 step oracle within 1e-3."""
    import ressl_model as rm
    from test_ressl_ref import oracle_run, ressl_cfg
    keys = ('loss', 'ent', 'row_loss', 'q')
    runs, finals, run = {}, {}, None
    for use_graph in (True, False):
        tr = pkg.ReSSLTrainer(ressl_cfg(pkg, WARMUP_FACTOR=1.0, BASE_LR=rm.LR), DEV, use_graph=use_graph, seed=rm.MODEL_SEED)
        if run is None:
            run = oracle_run(pkg, cpu_state(tr.model))
        tr.contrast.memory.copy_(run['Q0'].to(DEV))
        outs = []
        for x, sh in zip(run['xs'], run['shs']):
            out = tr.train_step(x.to(DEV), shuffle_ids=sh)
            torch.cuda.synchronize()
            assert set(out) >= set(keys) and tuple(out['row_loss'].shape) == (8,) and tuple(out['q'].shape) == (8, rm.OUT)
            outs.append(tuple(out[k].detach().clone() for k in keys))
        assert (tr._segments[0].graph is not None) == use_graph
        assert int(tr.ptr_dev) == 4 == tr.contrast.index
        runs[use_graph] = outs
        finals[use_graph] = (tr.arena_q.flat.detach().clone(), tr.arena_k.flat.detach().clone(), tr.contrast.memory.detach().clone(),
                             tr.ptr_dev.clone())
        state, state_ema = cpu_state(tr.model), cpu_state(tr.model_ema)
        sd = tr.state_dict()
        assert list(sd['contrast']) == ['memory'] and sd['queue_index'] == 4
        tr.close()
    for ga, ea in zip(runs[True], runs[False]):
        for a, b_ in zip(ga, ea):
            assert same(a, b_)
    for a, b_ in zip(finals[True], finals[False]):
        assert same(a, b_)
    vals = [float(o[0]) for o in runs[False]]
    print('MEASURED ressl trainer losses: %s  oracle: %s  ent: %s' % (' '.join('%.6f' % v for v in vals), ' '.join('%.6f' % v for v in run['losses']),
                                                                        ' '.join('%.4f' % float(o[1]) for o in runs[False])))
    for got, ref in zip(vals, run['losses']):
        assert abs(got - ref) <= 1e-3 * abs(ref), (vals, run['losses'])
    for o in runs[False]:
        assert abs(float(o[2].mean()) - float(o[0])) <= 1e-5 * abs(float(o[0])) and 0.0 < float(o[1]) < float(np.log(rm.QUEUE_K))
    want, want_ema = run['model'].state_dict(), run['ema'].state_dict()
    params = sorted(n for n, _ in run['model'].named_parameters())
    floats = sorted(n for n, v in want_ema.items() if v.dtype.is_floating_point)
    e_p = rel(torch.cat([state[n].reshape(-1) for n in params]), torch.cat([want[n].reshape(-1) for n in params]))
    e_t = rel(torch.cat([state_ema[n].reshape(-1) for n in floats]), torch.cat([want_ema[n].reshape(-1) for n in floats]))
    e_q = rel(finals[False][2], run['Q'])
    print('MEASURED ressl trainer after three steps: parameters %.2e teacher %.2e queue %.2e' % (e_p, e_t, e_q))
    assert e_p <= 1e-3 and e_t <= 1e-3 and e_q <= 1e-3 and run['index'] == 4


def test_checkpoint_resume_is_exact_and_loads_downstream(pkg):
    """Save after step 2, resume in a fresh trainer built with another seed: step 3 is bitwise the uninterrupted run's."""
    import copy
    import io
    import classify_model as cm
    import ressl_model as rm
    from test_gpu_adam import action_cfg
    from test_ressl_ref import ressl_cfg
    cm.register()
    cfg = ressl_cfg(pkg)
    xs, shs = [x.to(DEV) for x in rm.clip_batches(3, seed=13)], rm.shuffles(3, seed=13)
    a = pkg.ReSSLTrainer(cfg, DEV, use_graph=False, seed=5)
    for x, sh in zip(xs[:2], shs[:2]):
        a.train_step(x, shuffle_ids=sh)
    sd = a.state_dict(epoch=7)
    assert set(sd) >= {'epoch', 'state_dict', 'optimizer', 'contrast', 'model_ema', 'queue_index'} and sd['queue_index'] == 16
    buf = io.BytesIO()
    torch.save(sd, buf)
    b_ = pkg.ReSSLTrainer(cfg, DEV, use_graph=False, seed=99)
    assert b_.load_state_dict(torch.load(io.BytesIO(buf.getvalue()), map_location='cpu', weights_only=False)) == 7
    assert int(b_.ptr_dev) == 16 == b_.contrast.index and same(b_.contrast.memory, a.contrast.memory)
    oa, ob = a.train_step(xs[2], shuffle_ids=shs[2]), b_.train_step(xs[2], shuffle_ids=shs[2])
    torch.cuda.synchronize()
    assert same(oa['loss'], ob['loss']) and same(oa['ent'], ob['ent']) and same(oa['row_loss'], ob['row_loss'])
    assert same(a.arena_q.flat, b_.arena_q.flat) and same(a.arena_k.flat, b_.arena_k.flat) and same(a.contrast.memory, b_.contrast.memory)
    assert int(a.ptr_dev) == int(b_.ptr_dev) == 4 == a.contrast.index == b_.contrast.index
    for ma, mb in ((a.model, b_.model), (a.model_ema, b_.model_ema)):
        sa, sb = ma.state_dict(), mb.state_dict()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.optimizer.buf, b_.optimizer.buf)
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
    from test_ressl_ref import ressl_cfg
    register_tiny(pkg)
    for mem in ('simsiam', 'moco', 'simclr', 'barlow', 'vicreg', 'swav', 'dino', 'mocov3', 'nnclr'):
        with pytest.raises(ValueError, match='ressl'):
            pkg.ReSSLTrainer(make_cfg(pkg, 'R2P1D10T', mem, 32, 16, 8), DEV)
    with pytest.raises(NotImplementedError, match='one GPU'):
        pkg.ReSSLTrainer(ressl_cfg(pkg), DEV, ctx=pkg.parallel.DistCtx(force_active=True))
    for other in (pkg.SimCLRTrainer, pkg.MoCoV3Trainer, pkg.DINOTrainer, pkg.NNCLRTrainer):
        with pytest.raises(ValueError):
            other(ressl_cfg(pkg), DEV)
