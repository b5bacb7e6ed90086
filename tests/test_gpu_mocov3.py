"""gca_mocov3_fwd / gca_mocov3_bwd, ops.mocov3_*, lib.memory.MoCoV3Loss, the MoCoV3 wrapper and MoCoV3Trainer on the device, against
tests/mocov3_ref.py (fp64 numpy) and tests/mocov3_model.py (the fp64 torch oracle of the model and of one training step).

Exact inputs (entries m / 8, inv_T = 16: every s[i,j] is the same number in fp32 and fp64, tests/test_mocov3_ref.py): pos_logit
bit for bit, rank exactly -- ties with the positive included -- lse and both direction losses within 1e-5 * max|s|, the suite's
bar on the logit scale, dq within 1e-5 max-norm relative.  max|s| is 16 D there, far past exp's fp32 range: the max subtraction
is exercised.  N = 1: loss 0 and dq identically 0.

Float inputs (unit rows with cos(q, k) about 0.9, T = 0.2 and 0.5; `hard`: row norms spread 4x, rows sharing a direction, one
q row equal to its key, T = 0.5): loss, l12, l21, lse, dq1, dq2 within 1e-5 (max-norm relative) of the fp64 specification on
the same fp32 inputs, the suite's per-op bar.  The unfused fp32 torch chain (tests/mocov3_ref.py: torch_chain, on the CPU)
sits at most 5.7e-7 (loss: N = 5, D = 32, T = 0.2) and 1.3e-6 (dq: N = 100, D = 256, T = 0.2; 9.4e-7 at most at T = 0.5) from
fp64 over all of these cases (printed by test_mocov3_ref.py as `MEASURED mocov3 cpu chain ...`, and held there), so the bar
leaves 8x room over fp32 arithmetic at its tightest case and 17x on the loss, while each wrong variant of
tests/test_mocov3_ref.py misses it by more than 100x.  The sparse random rows of the exact inputs are explained in
tests/mocov3_ref.py: the backward pass reads an fp32 row_lse, which resolves exp(s - lse) to the bar only while a row's
competing logits are small or its lse is a representable number.

Measured on an MI355X (printed as `MEASURED mocov3 ...`), worst over the cases:
    exact inputs   |lse - fp64| 3.76e-6 (N = 64, D = 256; bar 4.10e-2)    |l_d - fp64| 3.21e-6 (N = 5, D = 32; bar 5.12e-3)
                   dq 1.91e-6 (N = 64, D = 256)    [bar 1e-5]
    unit rows      loss 1.17e-6, l12 1.07e-6, l21 1.22e-6 (N = 5, D = 32, T = 0.2)    lse 3.32e-7 (N = 33, D = 128, T = 0.2)
                   dq 1.96e-6 (N = 5, D = 32, T = 0.2)    [bar 1e-5]
    hard rows      loss 9.01e-8    lse 1.16e-7    dq 7.34e-7 (fast path, N = 33, D = 256), 8.52e-7 (generic, N = 40, D = 130)    [bar 1e-5]
    model          loss against the fp64 oracle 1.05e-6 relative, the four row matrices 2.6e-5; parameter gradients median
                   2.6e-5, worst 5.5e-5 over 76 tensors    [bar 1e-3]
    trainer        three losses 1.565891 1.242930 1.084555 against the oracle's 1.565892 1.242927 1.084567 (1.1e-5); the
                   teacher's state after three steps 3.1e-6 at worst    [bar 1e-3]
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mocov3_ref as mr                  # noqa: E402
from parity import make_cfg, register_tiny, rel           # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = -1
BAR = 1e-5


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def aligned(*ts):
    return all(t.data_ptr() % 16 == 0 for t in ts)


def c_path(pkg, N, D, al):
    w, s = C.c_int32(-1), C.c_int32(-1)
    rc = pkg._hip.lib.gca_mocov3_path(N, D, int(al), C.addressof(w), C.addressof(s))
    return ('generic', 'fast')[rc] if rc in (0, 1) else rc, w.value, s.value


def c_fwd(pkg, xs, inv_T, w):
    """gca_mocov3_fwd itself -> (loss (3,), lse, pos_logit, rank) as device tensors."""
    N, D = xs[0].shape
    lib, H = pkg._hip.lib, pkg._hip
    lse, pos = torch.empty(2 * N, device=DEV), torch.empty(2 * N, device=DEV)
    rank = torch.empty(2 * N, dtype=torch.int32, device=DEV)
    loss = torch.empty(3, device=DEV)
    ws = torch.empty(lib.gca_mocov3_ws_bytes(N, D), dtype=torch.uint8, device=DEV)
    rc = lib.gca_mocov3_fwd(*[H.ptr(x) for x in xs], N, D, inv_T, w, H.ptr(lse), H.ptr(pos), H.ptr(rank), H.ptr(loss), H.ptr(ws),
                            H.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return loss, lse, pos, rank


def cat(ref, key):
    return np.concatenate([ref[key][0], ref[key][1]])


# ----------------------------------------------------------------------------- 1. the kernels against the specification
@pytest.mark.parametrize('case,path', list(zip(mr.EXACT_CASES, mr.EXACT_PATHS)), ids=['N%d-D%d' % c for c in mr.EXACT_CASES])
def test_exact_inputs(pkg, case, path):
    N, D = case
    xs = mr.exact_inputs(N, D)
    w = mr.weight(mr.EXACT_INV_T)
    ref = mr.mocov3(*xs, mr.EXACT_INV_T)
    xd = [dev(x) for x in xs]
    want_path = mr.mocov3_path(N, D, aligned(*xd))
    assert want_path[0] == path and c_path(pkg, N, D, aligned(*xd)) == want_path
    loss, lse, pos, rank = c_fwd(pkg, xd, mr.EXACT_INV_T, w)
    assert np.array_equal(pos.cpu().numpy().astype(np.float64), cat(ref, 'sp'))
    assert np.array_equal(rank.cpu().numpy().astype(np.int64), cat(ref, 'rank'))
    smax = float(max(np.abs(s).max() for s in ref['s']))
    e_lse = float(np.abs(lse.cpu().numpy().astype(np.float64) - cat(ref, 'lse')).max())
    got = loss.cpu().numpy().astype(np.float64)
    e_l = max(abs(got[1] - ref['l'][0]), abs(got[2] - ref['l'][1]))
    print('MEASURED mocov3 exact N=%d D=%d: |lse err| %.3e |l_d err| %.3e (bar %.3e)' % (N, D, e_lse, e_l, BAR * smax))
    assert e_lse <= BAR * smax and e_l <= BAR * smax
    assert abs(got[0] - ref['loss']) <= BAR * smax * 2 * w
    dq1, dq2 = pkg.engine.ops.mocov3_bwd(*xd, lse, mr.EXACT_INV_T)
    torch.cuda.synchronize()
    if N == 1:
        assert float(loss[0]) == 0.0 and float(loss[1]) == 0.0 and float(loss[2]) == 0.0 and torch.equal(lse, pos)
        assert float(dq1.abs().max()) == 0.0 and float(dq2.abs().max()) == 0.0
    else:
        e = (rel(dq1, t64(ref['dq'][0])), rel(dq2, t64(ref['dq'][1])))
        print('MEASURED mocov3 exact N=%d D=%d: rel_err dq1 %.3e dq2 %.3e' % (N, D, e[0], e[1]))
        assert max(e) <= BAR, e


def float_case(pkg, xs, T, tag):
    inv_T = 1.0 / T
    ref = mr.mocov3(*xs, np.float32(inv_T))
    xd = [dev(x) for x in xs]
    N = xs[0].shape[0]
    ops = pkg.engine.ops
    loss, lse, rank, _ = ops.mocov3_fwd(*xd, inv_T, want_rank=True)
    dq1, dq2 = ops.mocov3_bwd(*xd, lse, inv_T)
    torch.cuda.synchronize()
    got = loss.cpu().numpy().astype(np.float64)
    e = dict(loss=abs(got[0] - ref['loss']) / abs(ref['loss']), l12=abs(got[1] - ref['l'][0]) / abs(ref['l'][0]),
             l21=abs(got[2] - ref['l'][1]) / abs(ref['l'][1]), lse=rel(lse, t64(cat(ref, 'lse'))),
             dq1=rel(dq1, t64(ref['dq'][0])), dq2=rel(dq2, t64(ref['dq'][1])))
    print('MEASURED mocov3 %s T=%g: rel_err %s' % (tag, T, ' '.join('%s %.3e' % kv for kv in e.items())))
    assert max(e.values()) <= BAR, e
    # rank wherever no other column sits within the bar of the positive
    r = rank.cpu().numpy()
    assert r.dtype == np.int32 and r.shape == (2, N)
    for d in range(2):
        clear = mr.clear_rows(ref['s'][d])
        assert clear.sum() >= (N + 1) // 2
        assert np.array_equal(r[d][clear], ref['rank'][d][clear])
    return e


@pytest.mark.parametrize('T', mr.FLOAT_TS)
@pytest.mark.parametrize('N,D', mr.FLOAT_CASES)
def test_float_inputs(pkg, N, D, T):
    assert mr.mocov3_path(N, D)[0] == 'fast'
    float_case(pkg, mr.float_inputs(N, D), T, 'unit N=%d D=%d' % (N, D))


@pytest.mark.parametrize('N,D,path', mr.HARD_CASES, ids=[c[2] for c in mr.HARD_CASES])
def test_mistakes_that_must_show(pkg, N, D, path):
    """Row norms spread 4x, rows sharing a direction, one q row equal to its key (properties: tests/test_mocov3_ref.py)."""
    assert mr.mocov3_path(N, D)[0] == path
    float_case(pkg, mr.float_inputs(N, D, hard=True), mr.HARD_T, 'hard N=%d D=%d' % (N, D))


@pytest.mark.parametrize('which', [0, 2], ids=['q1', 'k1'])
def test_unaligned_rows_take_the_generic_path_to_the_same_answer(pkg, which):
    N, D = 33, 128
    xs = mr.float_inputs(N, D)
    ref = mr.mocov3(*xs, np.float32(2.0))
    xd = [dev(x) for x in xs]
    buf = torch.zeros(N * D + 1, device=DEV)
    xo = buf[1:].view(N, D)
    xo.copy_(xd[which])
    xd[which] = xo
    assert not aligned(*xd) and mr.mocov3_path(N, D, aligned(*xd))[0] == 'generic'
    ops = pkg.engine.ops
    loss, lse, _, _ = ops.mocov3_fwd(*xd, 2.0)
    dq1, dq2 = ops.mocov3_bwd(*xd, lse, 2.0)
    torch.cuda.synchronize()
    assert rel(lse, t64(cat(ref, 'lse'))) <= BAR and abs(float(loss[0]) - ref['loss']) <= BAR * abs(ref['loss'])
    assert rel(dq1, t64(ref['dq'][0])) <= BAR and rel(dq2, t64(ref['dq'][1])) <= BAR


@pytest.mark.parametrize('N,D', [(33, 128), (257, 256), (33, 130)])
def test_deterministic(pkg, N, D):
    xd = [dev(x) for x in mr.float_inputs(N, D, seed=3)]
    ops = pkg.engine.ops
    outs = []
    for _ in range(2):
        loss, lse, rank, pos = ops.mocov3_fwd(*xd, 5.0, want_rank=True, want_pos=True)
        outs.append((loss, lse, rank, pos) + ops.mocov3_bwd(*xd, lse, 5.0))
    torch.cuda.synchronize()
    for a, b_ in zip(*outs):
        assert torch.equal(bits(a), bits(b_))


@pytest.mark.parametrize('N,D', [(33, 128), (257, 256), (33, 130)])
def test_gradient_scale(pkg, N, D):
    xd = [dev(x) for x in mr.float_inputs(N, D, seed=5)]
    ops = pkg.engine.ops
    _, lse, _, _ = ops.mocov3_fwd(*xd, 5.0)
    one = ops.mocov3_bwd(*xd, lse, 5.0)
    scaled = ops.mocov3_bwd(*xd, lse, 5.0, gscale_dev=torch.tensor([1024.0, 7.0], device=DEV))
    half = ops.mocov3_bwd(*xd, lse, 5.0, gscale_host=0.5)
    both = ops.mocov3_bwd(*xd, lse, 5.0, gscale_dev=torch.tensor([4.0], device=DEV), gscale_host=0.25)
    torch.cuda.synchronize()
    for d in range(2):
        assert float(one[d].abs().max()) > 0
        assert torch.equal(bits(scaled[d]), bits(one[d] * 1024.0)) and torch.equal(bits(half[d]), bits(one[d] * 0.5))
        assert torch.equal(bits(both[d]), bits(one[d]))


def test_refused_arguments_touch_nothing(pkg):
    lib, H = pkg._hip.lib, pkg._hip
    N, D = 8, 8
    xs = [dev(x) for x in mr.float_inputs(N, D)]
    SENT = 12345.0
    lse, pos, loss, dq1, dq2 = (torch.full((n,), SENT, device=DEV) for n in (2 * N + 1, 2 * N + 1, 3, N * D + 8, N * D + 8))
    rank = torch.full((2 * N + 1,), 777, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(lib.gca_mocov3_ws_bytes(N, D), 1 << 16), dtype=torch.uint8, device=DEV)
    p = H.ptr
    nan, inf = float('nan'), float('inf')
    assert lib.gca_mocov3_ws_bytes(0, 8) == -1 and lib.gca_mocov3_ws_bytes(65537, 1) == -1 and lib.gca_mocov3_ws_bytes(8, 0) == -1
    assert lib.gca_mocov3_ws_bytes(65536, 32768) == -1 and lib.gca_mocov3_ws_bytes(1, 1) > 0
    assert lib.gca_mocov3_path(0, 8, 1, None, None) == EINVAL

    def fwd(a=p(xs[0]), b=p(xs[1]), c=p(xs[2]), d=p(xs[3]), N=N, D=D, inv_T=2.0, w=1.0, lp=p(lse), lo=p(loss), wsp=p(ws)):
        return lib.gca_mocov3_fwd(a, b, c, d, N, D, inv_T, w, lp, p(pos), p(rank), lo, wsp, H.stream())

    def bwd(a=p(xs[0]), b=p(xs[1]), c=p(xs[2]), d=p(xs[3]), N=N, D=D, inv_T=2.0, w=1.0, lp=p(lse), d1=p(dq1), d2=p(dq2), wsp=p(ws)):
        return lib.gca_mocov3_bwd(a, b, c, d, lp, N, D, inv_T, w, None, 1.0, d1, d2, wsp, H.stream())

    for f in (fwd, bwd):
        for kw in (dict(N=0), dict(N=-2), dict(N=65537, D=1), dict(D=0), dict(D=-1), dict(N=65536, D=32768),
                   dict(inv_T=0.0), dict(inv_T=-1.0), dict(inv_T=inf), dict(inv_T=nan), dict(w=0.0), dict(w=-1.0), dict(w=inf),
                   dict(w=nan), dict(a=None), dict(b=None), dict(c=None), dict(d=None), dict(lp=None), dict(wsp=None)):
            assert f(**kw) == EINVAL, (f.__name__, kw)
    assert fwd(lo=None) == EINVAL and bwd(d1=None) == EINVAL and bwd(d2=None) == EINVAL
    # an output that is (or overlaps) an input, or the other output
    for kw in (dict(d1=p(xs[0])), dict(d2=p(xs[1])), dict(d1=p(xs[2])), dict(d2=p(xs[3])), dict(d2=p(dq1)), dict(d2=p(dq1[4:]))):
        assert bwd(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    for t in (lse, pos, loss, dq1, dq2):
        assert float(t.min()) == SENT == float(t.max())
    assert int(rank.min()) == 777 == int(rank.max())
    # the optional outputs may be NULL, and the accepted calls write exactly their rows
    assert lib.gca_mocov3_fwd(*[p(x) for x in xs], N, D, 2.0, 1.0, p(lse), None, None, p(loss), p(ws), H.stream()) == 0
    assert bwd() == 0
    torch.cuda.synchronize()
    assert float(lse[2 * N]) == SENT and float(lse[:2 * N].max()) < SENT and float(pos.min()) == SENT
    for t in (dq1, dq2):
        assert float(t[N * D:].min()) == SENT == float(t[N * D:].max()) and float(t[:N * D].abs().max()) < SENT


def test_ops_refuse_what_the_entry_refuses(pkg):
    ops = pkg.engine.ops
    z = torch.zeros(4, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.mocov3_fwd(z, z, z, torch.zeros(3, 8, device=DEV), 2.0)
    with pytest.raises(ValueError):
        ops.mocov3_fwd(z, z, z, z.double(), 2.0)
    with pytest.raises(ValueError):
        ops.mocov3_fwd(torch.zeros(0, 8, device=DEV), *[torch.zeros(0, 8, device=DEV)] * 3, 2.0)
    for bad in (float('nan'), 0.0, -1.0, float('inf')):
        with pytest.raises(ValueError):
            ops.mocov3_fwd(z, z, z, z, bad)
        with pytest.raises(ValueError):
            ops.mocov3_fwd(z, z, z, z, 2.0, w=bad)
    with pytest.raises(ValueError):
        ops.mocov3_bwd(z, z, z, z, torch.zeros(4, device=DEV), 2.0)
    with pytest.raises(ValueError):
        ops.mocov3_bwd(z, z, z, z, torch.zeros(8, device=DEV), 2.0, gscale_host=float('inf'))


def test_capturable_in_a_graph(pkg):
    """Forward and backward inside one captured graph: replays track the static inputs and equal the eager bits."""
    ops = pkg.engine.ops
    N, D = 100, 256
    xs = [torch.empty(N, D, device=DEV) for _ in range(4)]
    for x, v in zip(xs, mr.float_inputs(N, D)):
        x.copy_(dev(v))
    eager = ops.mocov3_fwd(*xs, 5.0, want_rank=True)
    eager_dq = ops.mocov3_bwd(*xs, eager[1], 5.0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss, lse, rank, _ = ops.mocov3_fwd(*xs, 5.0, want_rank=True)
        dq1, dq2 = ops.mocov3_bwd(*xs, lse, 5.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(loss), bits(eager[0])) and torch.equal(rank, eager[2])
    assert torch.equal(bits(dq1), bits(eager_dq[0])) and torch.equal(bits(dq2), bits(eager_dq[1]))
    for x, v in zip(xs, mr.float_inputs(N, D, seed=9)):
        x.copy_(dev(v))
    g.replay()
    torch.cuda.synchronize()
    ref = mr.mocov3(*[x.cpu().numpy() for x in xs], np.float32(5.0))
    assert abs(float(loss[0]) - ref['loss']) <= BAR * abs(ref['loss'])
    assert rel(dq1, t64(ref['dq'][0])) <= BAR and rel(dq2, t64(ref['dq'][1])) <= BAR
    g.reset()


# ----------------------------------------------------------------------------- 2. the module
def test_module_forward_backward(pkg):
    import importlib
    MoCoV3Loss = importlib.import_module(pkg.__name__ + '.lib.memory.mocov3').MoCoV3Loss
    N, D, T = 33, 256, 0.2
    xs = mr.float_inputs(N, D, seed=2)
    ref = mr.mocov3(*xs, np.float32(1.0 / T), g=3.0)
    q1, q2, k1, k2 = (dev(x).requires_grad_(True) for x in xs)
    crit = MoCoV3Loss(T)
    loss = crit(q1, q2, k1, k2)
    assert loss.dim() == 0 and abs(float(loss.detach()) - ref['loss']) <= BAR * abs(ref['loss'])
    (loss * 3.0).backward()
    torch.cuda.synchronize()
    assert rel(q1.grad, t64(ref['dq'][0])) <= BAR and rel(q2.grad, t64(ref['dq'][1])) <= BAR
    assert k1.grad is None and k2.grad is None
    assert crit.rank.dtype is torch.int32 and tuple(crit.rank.shape) == (2, N)
    assert int(crit.rank.sum()) == int(ref['rank'][0].sum() + ref['rank'][1].sum())
    assert abs(float(crit.l12) - ref['l'][0]) <= BAR * ref['l'][0] and abs(float(crit.l21) - ref['l'][1]) <= BAR * ref['l'][1]


# ----------------------------------------------------------------------------- 3. model and trainer
CLIP = (8, 6, 8, 48, 48)
OUT, HID, TEMP = 32, 48, 0.2
ALPHA = 0.9              # a teacher momentum at which three steps move the teacher visibly
LR = 3e-5                # this tiny model on 8 clips is badly conditioned over several steps: the ORACLE's own fp32 run leaves its
                         # fp64 run by 3.8e-4 / 2.1e-2 at the second / third loss at a rate of 3e-4, by 1.4e-6 / 1.9e-5 at 3e-5 (checked on
                         # the CPU), where its loss falls 1.5659, 1.2429, 1.0846: a fiftieth of the 1e-3 bar


def clips(seed, n=4):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*CLIP, generator=gen).to(DEV) for _ in range(n)]


def v3_cfg(pkg, **solver):
    import mocov3_model                  # noqa: F401  (the oracle's registry is filled by register_tiny)
    register_tiny(pkg)
    cfg = make_cfg(pkg, 'R2P1D10T', 'mocov3', OUT, 16, 8, **solver)
    cfg.CONTRAST.NCE_T = TEMP
    cfg.CONTRAST.V3_HID = HID
    cfg.CONTRAST.ALPHA = ALPHA
    return cfg


def cpu_state(module):
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def test_model_against_the_fp64_oracle(pkg):
    import importlib
    import mocov3_model as mm
    from parity import check_grad_errors
    MoCoV3Loss = importlib.import_module(pkg.__name__ + '.lib.memory.mocov3').MoCoV3Loss
    tr = pkg.MoCoV3Trainer(v3_cfg(pkg), DEV, use_graph=False, seed=21)
    with torch.no_grad():                                                       # a teacher that differs from its student
        gen = torch.Generator().manual_seed(5)
        tr.arena_t.flat.mul_(1.0 + 0.05 * torch.randn(tr.arena_t.flat.shape, generator=gen).to(DEV))
    state, state_t = cpu_state(tr.model), cpu_state(tr.model_ema)
    assert [k for k in state if '.prediction.' not in k] == list(state_t)
    x = clips(31, 1)[0]
    student, teacher = mm.oracle_mocov3('R2P1D10T', 8, OUT, HID, state, state_t)
    want, rows = mm.model_loss(student, teacher, x.cpu().double(), TEMP)
    want.backward()
    crit = MoCoV3Loss(TEMP)
    tr.optimizer.zero_grad()
    x1, x2 = (v.contiguous() for v in torch.chunk(x, 2, dim=1))
    with torch.no_grad():
        k1, k2 = tr.model_ema(x1), tr.model_ema(x2)
    q1, q2 = tr.model(x1), tr.model(x2)
    got = crit(q1, q2, k1, k2)
    got.backward()
    torch.cuda.synchronize()
    want = want.detach()
    e = dict(loss=abs(float(got.detach()) - float(want)) / abs(float(want)))
    for name, mine, ref in zip(('q1', 'q2', 'k1', 'k2'), (q1, q2, k1, k2), rows):
        e[name] = rel(mine, ref)
    print('MEASURED mocov3 model loss %.6f vs oracle %.6f: rel err %s' % (float(got.detach()), float(want), ' '.join('%s %.3e' % kv for kv in e.items())))
    assert got.dim() == 0 and tuple(q1.shape) == (8, OUT) and max(e.values()) < 1e-3, e
    assert float((q1.detach().norm(dim=1) - 1).abs().max()) < 1e-5             # unit rows
    g64 = {n: p.grad for n, p in student.named_parameters()}
    # (the bias of a Linear in front of a BatchNorm has no gradient but fp64 rounding: such tensors are left out)
    floor = 1e-9 * max(float(g.abs().max()) for g in g64.values() if g is not None)
    errs = {n: rel(p.grad, g64[n]) for n, p in tr.model.named_parameters() if g64[n] is not None and g64[n].abs().max() > floor}
    assert len(errs) > 40 and 'model.prediction.l2.weight' in errs and 'model.projection.l1.0.weight' in errs
    assert 'model.prediction.l2.bias' in errs and 'model.prediction.l1.0.bias' not in errs
    med, p95, worst = check_grad_errors(errs, 'mocov3 parameter gradients')
    print('MEASURED mocov3 model parameter gradients: median %.2e p95 %.2e worst %.2e over %d tensors' % (med, p95, worst, len(errs)))
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in tr.model_ema.parameters())      # no gradient reaches the teacher
    tr.close()


def test_trainer_graph_equals_eager_and_follows_the_oracle(pkg):
    """Three steps on one repeated batch: the captured run equals the eager run bit for bit, the loss falls, and the losses (the
    second and third are functions of whole steps: SGD, then the EMA), the teacher's own BatchNorm statistics and its
    parameters follow the fp64 step oracle at the project's 1e-3.  (What the EMA does to a parameter is far below 1e-3 of the
    parameter: test_ema_after_one_step holds it to fp32 rounding instead.)"""
    import mocov3_model as mm
    cfg = v3_cfg(pkg, WARMUP_FACTOR=1.0, BASE_LR=LR)
    x = clips(33, 1)[0]
    runs, finals, state = {}, {}, None
    keys = ('loss', 'l12', 'l21', 'rank')
    for use_graph in (True, False):
        tr = pkg.MoCoV3Trainer(cfg, DEV, use_graph=use_graph, seed=7)
        if state is None:
            state = cpu_state(tr.model)
            assert all(torch.equal(v, state[k]) for k, v in cpu_state(tr.model_ema).items())       # the teacher starts as the student
        outs = []
        for _ in range(3):
            out = tr.train_step(x)
            torch.cuda.synchronize()
            assert set(out) >= set(keys) and out['rank'].dtype is torch.int32 and tuple(out['rank'].shape) == (2, 8)
            outs.append(tuple(out[k].detach().clone() for k in keys))
        assert (tr._segments[0].graph is not None) == use_graph
        runs[use_graph] = outs
        finals[use_graph] = (tr.arena.flat.detach().clone(), tr.arena_t.flat.detach().clone())
        teacher_state = cpu_state(tr.model_ema)
        sd = tr.state_dict()
        assert sd['contrast'] is None and sd['momentum'] == ALPHA
        assert list(sd['model_ema']) == [k for k in sd['state_dict'] if '.prediction.' not in k]
        tr.close()
    for ga, ea in zip(runs[True], runs[False]):
        for a, b_ in zip(ga, ea):
            assert torch.equal(bits(a), bits(b_))
    for a, b_ in zip(finals[True], finals[False]):
        assert torch.equal(bits(a), bits(b_))
    vals = [float(o[0]) for o in runs[False]]
    student, teacher = mm.oracle_mocov3('R2P1D10T', 8, OUT, HID, state)
    want = mm.oracle_steps(student, teacher, x.cpu().double(), 3, LR, ALPHA, TEMP)
    want_t = teacher.state_dict()
    params = {n for n, _ in teacher.named_parameters()}
    e_t = {k: rel(v, want_t[k]) for k, v in teacher_state.items() if v.is_floating_point() and k not in params}
    e_t['parameters'] = rel(torch.cat([teacher_state[k].reshape(-1) for k in sorted(params)]),
                            torch.cat([want_t[k].reshape(-1) for k in sorted(params)]))
    assert len(e_t) > 40
    worst = max(e_t, key=e_t.get)
    print('MEASURED mocov3 trainer losses on one repeated batch: %s  oracle: %s  teacher state worst %.2e (%s)'
          % (' '.join('%.6f' % v for v in vals), ' '.join('%.6f' % v for v in want), e_t[worst], worst))
    assert all(np.isfinite(vals)) and vals[-1] < vals[0]
    for got, ref in zip(vals, want):
        assert abs(got - ref) <= 1e-3 * abs(ref), (vals, want)
    assert e_t[worst] <= 1e-3, (worst, e_t[worst])
    assert all(int(v) == int(want_t[k]) for k, v in teacher_state.items() if not v.is_floating_point())
    first = [float(v) for v in runs[False][0][:3]]
    assert abs(2 * TEMP * (first[1] + first[2]) - first[0]) <= 1e-6 * abs(first[0])


def test_ema_after_one_step(pkg):
    """teacher = m * old teacher + (1 - m) * NEW student over encoder and projector (the optimizer steps first); the student,
    predictor included, is not touched by the EMA; BatchNorm buffers are the teacher's own, not averages."""
    cfg = v3_cfg(pkg, WARMUP_FACTOR=1.0, BASE_LR=0.03)
    x = clips(37, 1)[0]
    res = {}
    for m in (ALPHA, 0.0):
        tr = pkg.MoCoV3Trainer(cfg, DEV, use_graph=False, seed=3)
        tr.set_schedule(momentum=m)
        with torch.no_grad():
            gen = torch.Generator().manual_seed(8)
            tr.arena_t.flat.mul_(1.0 + 0.05 * torch.randn(tr.arena_t.flat.shape, generator=gen).to(DEV))
            for b_ in tr.model_ema.buffers():
                if b_.is_floating_point():
                    b_.add_(0.25)                                               # buffers that differ from the student's
        n = tr.arena_t.total
        assert 0 < n < tr.arena.total and [k for k in tr.arena.names if '.prediction.' in k] == tr.arena.names[len(tr.arena_t.names):]
        old_t, old_s = tr.arena_t.flat.clone(), tr.arena.flat.clone()
        old_buf = {k: v.clone() for k, v in tr.model_ema.named_buffers()}
        tr.train_step(x)
        torch.cuda.synchronize()
        new_s, new_t = tr.arena.flat.clone(), tr.arena_t.flat.clone()
        assert not torch.equal(new_s[n:], old_s[n:]) and not torch.equal(new_s[:n], old_s[:n])       # SGD moved all of the student
        want = m * old_t.double() + (1.0 - m) * new_s[:n].double()
        assert rel(new_t, want) <= 1e-6
        if m == 0.0:
            assert torch.equal(bits(new_t), bits(new_s[:n]))
        else:
            assert rel(new_t, m * old_t.double() + (1.0 - m) * old_s[:n].double()) > 1e-6               # not the pre-update student
        sbuf = dict(tr.model.named_buffers())
        for k, v in tr.model_ema.named_buffers():
            if v.is_floating_point():
                # one training-mode forward per view moved it from its own old value; an average with the student's would sit
                # 0.25 (1 - m) away from where it is
                assert not torch.equal(v, old_buf[k]), k
                avg = m * old_buf[k].double() + (1.0 - m) * sbuf[k].double()
                assert float((v.double() - avg).abs().max()) > 0.01, k
            else:
                assert int(v) == int(old_buf[k]) + 2, k
        res[m] = new_s
        tr.close()
    assert torch.equal(bits(res[ALPHA]), bits(res[0.0]))                        # the momentum never reaches the student


def test_set_schedule_between_replays(pkg):
    """The captured step reads the momentum from the device: a graph trainer whose schedule is moved after capture equals, bit
    for bit, an eager trainer given the same values at the same steps."""
    cfg = v3_cfg(pkg, WARMUP_FACTOR=1.0, BASE_LR=LR)
    xs = clips(35, 5)
    sched = [None] * 3 + [0.99, 1.0]                                            # the graph is captured at the third step
    res = {}
    for use_graph in (True, False):
        tr = pkg.MoCoV3Trainer(cfg, DEV, use_graph=use_graph, seed=9)
        losses = []
        for x, m in zip(xs, sched):
            tr.set_schedule(momentum=m)
            if m == 1.0:
                frozen = tr.arena_t.flat.clone()
            losses.append(tr.train_step(x)['loss'].detach().clone())
        torch.cuda.synchronize()
        if use_graph:
            assert tr._segments[0].graph is not None
        assert torch.equal(bits(frozen), bits(tr.arena_t.flat))                 # momentum 1: the teacher stands still
        assert tr.momentum == 1.0 and float(tr.m_dev) == 1.0
        res[use_graph] = (losses, tr.arena_t.flat.clone(), tr.arena.flat.clone())
        for bad in (1.01, -0.1, float('nan'), 2.0):
            with pytest.raises(ValueError):
                tr.set_schedule(momentum=bad)
        assert tr.momentum == 1.0 and float(tr.m_dev) == 1.0                    # a refusal changes nothing
        tr.close()
    for a, b_ in zip(res[True][0], res[False][0]):
        assert torch.equal(bits(a), bits(b_))
    assert torch.equal(bits(res[True][1]), bits(res[False][1])) and torch.equal(bits(res[True][2]), bits(res[False][2]))


def test_checkpoint_resume_is_exact_and_loads_downstream(pkg):
    import copy
    import classify_model as cm
    from test_gpu_adam import action_cfg, assert_resume_is_exact
    cm.register()
    cfg = v3_cfg(pkg)

    def make(seed):
        tr = pkg.MoCoV3Trainer(cfg, DEV, use_graph=False, seed=seed)
        if seed == 5:
            tr.set_schedule(momentum=0.95)                                      # the resumed trainer must pick this up
        return tr

    a, b_, sd = assert_resume_is_exact(make, clips(13, 5), ('epoch', 'state_dict', 'optimizer', 'contrast', 'model_ema', 'momentum'))
    assert b_.momentum == 0.95 and float(b_.m_dev) == float(np.float32(0.95))
    sa, sb = a.model_ema.state_dict(), b_.model_ema.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert all(k.startswith(('model.encoder.', 'model.projection.', 'model.prediction.')) for k in sd['state_dict'])
    assert not any('.prediction.' in k for k in sd['model_ema'])
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
    enc = pkg.lib.evaluation.load_encoder(sd, 'R2P1D10T', 8)
    assert not enc.training
    a.close(), b_.close()


def test_trainer_refusals(pkg, monkeypatch):
    register_tiny(pkg)
    for mem in ('simsiam', 'moco', 'simclr', 'barlow', 'vicreg', 'swav', 'dino'):
        with pytest.raises(ValueError, match='mocov3'):
            pkg.MoCoV3Trainer(make_cfg(pkg, 'R2P1D10T', mem, 32, 16, 8), DEV)
    with pytest.raises(NotImplementedError, match='one GPU'):
        pkg.MoCoV3Trainer(v3_cfg(pkg), DEV, ctx=pkg.parallel.DistCtx(force_active=True))
    for other in (pkg.SimCLRTrainer, pkg.SimSiamTrainer, pkg.DINOTrainer):
        with pytest.raises(ValueError):
            other(v3_cfg(pkg), DEV)
    trainer = pkg.engine.trainer
    real = trainer.create_visual_model
    monkeypatch.setattr(trainer, 'create_visual_model', lambda cfg: (real(cfg)[0], None))
    with pytest.raises(ValueError, match='EMA twin'):
        pkg.MoCoV3Trainer(v3_cfg(pkg), DEV)
    # a teacher whose layout is not the student's leading part
    monkeypatch.setattr(trainer, 'create_visual_model', lambda cfg: (real(cfg)[0], real(cfg)[0]))
    with pytest.raises(RuntimeError, match='leading part'):
        pkg.MoCoV3Trainer(v3_cfg(pkg), DEV)
