"""gca_nnclr_search / gca_nnclr_bwd, ops.nnclr_*, lib.memory.NNCLRLoss, the NNCLR wrapper and NNCLRTrainer on the device, against
tests/nnclr_ref.py (fp64 numpy) and tests/nnclr_model.py (the fp64 torch oracle of the model and of a training step, queue
update included).

Search, exact inputs (entries m / 8: every score is the same number in fp32 and fp64, tests/test_nnclr_ref.py): idx exactly the
specification's -- equal maxima at columns 0 and K - 1, at 31 / 32 across a tile edge, on both sides of every split boundary the
path function reports, a row whose maximum is its last column, a NaN support row and an all-NaN z row included -- sim bit for
bit, nn bit for bit Q[idx].  Search, float inputs (unit rows, every row's top-2 gap above 1e-5 max|s|, asserted on the CPU): idx
exact, sim within 1e-5 relative.  Backward: dp1, dp2 within 1e-5 max-norm relative of the fp64 specification on the same fp32
inputs and the device's own lse, the suite's per-op bar; N = 1 gives identically 0.  The float inputs of the backward have
cos(nn[i], p[i]) about 0.45, not 0.9: tests/nnclr_ref.py (bwd_float_inputs) says why -- at 0.9 and T = 0.1 the softmax of 5 rows
is saturated and fp32 rounding of the logits alone is 1.5e-4 of dp on the CPU; the first version of these inputs measured 6.0e-5
for this kernel there.  The unfused fp32 torch chain on the CPU sits at most 2.7e-7 (loss) and 1.3e-6 (dp: N = 5, D = 128,
T = 0.1) from fp64 over the float and hard cases (test_nnclr_ref.py prints it as `MEASURED nnclr cpu chain ...` and holds it to a
quarter of the bar), so the bar leaves 8x room over fp32 arithmetic, while each wrong variant there misses it by more than 100x.

Measured on an MI355X (printed as `MEASURED nnclr ...`), worst over the cases:
    search         idx exact in every case; sim 8.22e-7 (N = 100, D = 256, K = 1000; generic path 4.55e-7)    [bar 1e-5]
    exact inputs   dp 2.79e-6 (N = 5, D = 32), 2.71e-6 (N = 64, D = 256)    [bar 1e-5]
    unit rows      dp 2.98e-6 (N = 5, D = 256, T = 0.1), loss 1.97e-6 (same case)    [bar 1e-5]
    hard rows      dp 5.60e-7 (fast path, N = 33, D = 256), 4.74e-7 (generic, N = 40, D = 130); loss 9.01e-8    [bar 1e-5]
    model          loss against the fp64 oracle 5.3e-7 relative, z and p rows 2.6e-5 at worst; parameter gradients median
                   2.7e-5, worst 5.5e-5 over 76 tensors    [bar 1e-3]
    trainer        three losses 1.909360 2.167644 2.481691 against the oracle's 1.909363 2.167645 2.481688 (1.6e-6), idx equal at every
                   step (the oracle's top-2 gaps 0.2325 0.2972 0.2329 against the 0.1 they must exceed); after three steps
                   parameters 2.0e-7, support set 5.8e-5    [bar 1e-3]
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mocov3_ref as mr                  # noqa: E402
import nnclr_ref as nr                   # noqa: E402
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


def c_search_path(pkg, N, D, K, al):
    w, s = C.c_int32(-1), C.c_int32(-1)
    rc = pkg._hip.lib.gca_nnclr_search_path(N, D, K, int(al), C.addressof(w), C.addressof(s))
    return ('generic', 'fast')[rc] if rc in (0, 1) else rc, w.value, s.value


def c_bwd_path(pkg, N, D, al):
    w, s = C.c_int32(-1), C.c_int32(-1)
    rc = pkg._hip.lib.gca_nnclr_bwd_path(N, D, int(al), C.addressof(w), C.addressof(s))
    return ('generic', 'fast')[rc] if rc in (0, 1) else rc, w.value, s.value


def same_bits(got, want_np):
    """fp32 device tensor against an fp32 numpy array, bit for bit (NaN payloads included)."""
    return np.array_equal(got.detach().cpu().numpy().view(np.int32), np.ascontiguousarray(want_np, dtype=np.float32).view(np.int32))


# ----------------------------------------------------------------------------- 1. the search against the specification
def check_exact_search(pkg, N, D, K, path, nan=False):
    z1, z2, Q, plants = nr.exact_search_inputs(N, D, K, nan=nan)
    ref = nr.search(z1, z2, Q)
    zd1, zd2, Qd = dev(z1), dev(z2), dev(Q)
    want_path = nr.search_path(N, D, K, aligned(zd1, zd2, Qd))
    assert want_path[0] == path and c_search_path(pkg, N, D, K, aligned(zd1, zd2, Qd)) == want_path[:3]
    idx, sim, nn1, nn2 = pkg.engine.ops.nnclr_search(zd1, zd2, Qd)
    torch.cuda.synchronize()
    assert idx.dtype is torch.int32 and tuple(idx.shape) == (2, N) and tuple(sim.shape) == (2, N)
    got = idx.cpu().numpy().astype(np.int64)
    assert got.min() >= 0 and got.max() < K
    assert np.array_equal(got, np.stack(ref['idx'])), np.argwhere(got != np.stack(ref['idx']))[:8]
    assert same_bits(sim, np.stack(ref['sim']).astype(np.float32))
    assert same_bits(nn1, Q[got[0]]) and same_bits(nn2, Q[got[1]])
    for view, row, cols, want in plants:                                        # (their place and equality: test_nnclr_ref.py)
        assert got[view, row] == want
    return want_path


@pytest.mark.parametrize('case,path', list(zip(nr.SEARCH_EXACT_CASES, nr.SEARCH_EXACT_PATHS)),
                         ids=['N%d-D%d-K%d' % c for c in nr.SEARCH_EXACT_CASES])
def test_search_exact_inputs(pkg, case, path):
    check_exact_search(pkg, *case, path)


def test_search_nan_rows(pkg):
    """A NaN support row is never chosen; an all-NaN z row takes column 0 with sim = -inf (every key is -inf there)."""
    N, D, K = nr.NAN_CASE
    check_exact_search(pkg, N, D, K, 'fast', nan=True)
    z1, z2, Q, _ = nr.exact_search_inputs(N, D, K, nan=True)
    idx, sim, _, nn2 = pkg.engine.ops.nnclr_search(dev(z1), dev(z2), dev(Q))
    torch.cuda.synchronize()
    assert int(idx[1, 3]) == 0 and float(sim[1, 3]) == float('-inf') and not bool((idx == 5).any())
    assert same_bits(nn2[3], Q[0])


@pytest.mark.parametrize('N,D,K', nr.SEARCH_FLOAT_CASES)
def test_search_float_inputs(pkg, N, D, K):
    z1, z2, Q, _ = nr.float_search_inputs(N, D, K)
    ref = nr.search(z1, z2, Q)
    idx, sim, nn1, nn2 = pkg.engine.ops.nnclr_search(dev(z1), dev(z2), dev(Q))
    torch.cuda.synchronize()
    got = idx.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, np.stack(ref['idx']))                            # every row is clear: test_nnclr_ref.py
    e = rel(sim, t64(np.stack(ref['sim'])))
    print('MEASURED nnclr search unit N=%d D=%d K=%d (%s): rel_err sim %.3e' % (N, D, K, nr.search_path(N, D, K)[0], e))
    assert e <= BAR
    assert same_bits(nn1, Q[got[0]]) and same_bits(nn2, Q[got[1]])


# ----------------------------------------------------------------------------- 2. the backward against the specification
def fwd_lse(pkg, xd, inv_T):
    loss, lse, rank, _ = pkg.engine.ops.mocov3_fwd(*xd, inv_T, w=nr.W, want_rank=True)
    return loss, lse, rank


@pytest.mark.parametrize('case,path', list(zip(nr.BWD_EXACT_CASES, nr.BWD_EXACT_PATHS)), ids=['N%d-D%d' % c for c in nr.BWD_EXACT_CASES])
def test_backward_exact_inputs(pkg, case, path):
    N, D = case
    xs = nr.bwd_exact_inputs(N, D)
    ref = nr.nnclr(*xs, nr.EXACT_INV_T)
    xd = [dev(x) for x in xs]
    loss, lse, _ = fwd_lse(pkg, xd, nr.EXACT_INV_T)
    dp1 = torch.empty(N, D, device=DEV)
    dp2 = torch.empty(N, D, device=DEV)
    assert c_bwd_path(pkg, N, D, aligned(*xd, dp1, dp2)) == mr.mocov3_path(N, D, aligned(*xd, dp1, dp2)) and mr.mocov3_path(N, D)[0] == path
    dp1, dp2 = pkg.engine.ops.nnclr_bwd(*xd, lse, nr.EXACT_INV_T)
    torch.cuda.synchronize()
    smax = float(max(np.abs(s).max() for s in ref['s']))
    assert abs(float(loss[0]) - ref['loss']) <= BAR * smax
    if N == 1:
        assert float(loss[0]) == 0.0 and float(dp1.abs().max()) == 0.0 and float(dp2.abs().max()) == 0.0
    else:
        e = (rel(dp1, t64(ref['dp1'])), rel(dp2, t64(ref['dp2'])))
        print('MEASURED nnclr bwd exact N=%d D=%d: rel_err dp1 %.3e dp2 %.3e' % (N, D, e[0], e[1]))
        assert max(e) <= BAR, e


def float_bwd_case(pkg, xs, T, tag):
    inv_T = 1.0 / T
    ref = nr.nnclr(*xs, np.float32(inv_T))
    xd = [dev(x) for x in xs]
    loss, lse, _ = fwd_lse(pkg, xd, inv_T)
    dp1, dp2 = pkg.engine.ops.nnclr_bwd(*xd, lse, inv_T)
    torch.cuda.synchronize()
    e = dict(loss=abs(float(loss[0]) - ref['loss']) / abs(ref['loss']), dp1=rel(dp1, t64(ref['dp1'])), dp2=rel(dp2, t64(ref['dp2'])))
    print('MEASURED nnclr bwd %s T=%g: rel_err %s' % (tag, T, ' '.join('%s %.3e' % kv for kv in e.items())))
    assert max(e.values()) <= BAR, e


@pytest.mark.parametrize('T', nr.BWD_FLOAT_TS)
@pytest.mark.parametrize('N,D', nr.BWD_FLOAT_CASES)
def test_backward_float_inputs(pkg, N, D, T):
    assert mr.mocov3_path(N, D)[0] == 'fast'
    float_bwd_case(pkg, nr.bwd_float_inputs(N, D), T, 'unit N=%d D=%d' % (N, D))


@pytest.mark.parametrize('N,D,path', nr.HARD_CASES, ids=[c[2] for c in nr.HARD_CASES])
def test_backward_mistakes_that_must_show(pkg, N, D, path):
    """Row norms spread 4x, rows sharing a direction, one p row equal to its neighbour (properties: tests/test_nnclr_ref.py)."""
    assert mr.mocov3_path(N, D)[0] == path
    float_bwd_case(pkg, nr.bwd_float_inputs(N, D, hard=True), nr.HARD_T, 'hard N=%d D=%d' % (N, D))


# ----------------------------------------------------------------------------- 3. paths, determinism, scale, refusals, capture
def unaligned_copy(t):
    buf = torch.zeros(t.numel() + 1, device=DEV)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    return out


@pytest.mark.parametrize('which', [0, 2], ids=['z1', 'Q'])
def test_unaligned_search_takes_the_generic_path_to_the_same_idx(pkg, which):
    N, D, K = 33, 128, 100
    z1, z2, Q, _ = nr.float_search_inputs(N, D, K)
    ref = nr.search(z1, z2, Q)
    xd = [dev(z1), dev(z2), dev(Q)]
    xd[which] = unaligned_copy(xd[which])
    assert not aligned(*xd) and nr.search_path(N, D, K, aligned(*xd))[0] == 'generic'
    idx, sim, nn1, nn2 = pkg.engine.ops.nnclr_search(*xd)
    torch.cuda.synchronize()
    got = idx.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, np.stack(ref['idx'])) and rel(sim, t64(np.stack(ref['sim']))) <= BAR
    assert same_bits(nn1, Q[got[0]]) and same_bits(nn2, Q[got[1]])


@pytest.mark.parametrize('which', [0, 2], ids=['nn1', 'p1'])
def test_unaligned_backward_takes_the_generic_path_to_the_same_answer(pkg, which):
    N, D = 33, 128
    xs = nr.bwd_float_inputs(N, D)
    ref = nr.nnclr(*xs, np.float32(5.0))
    xd = [dev(x) for x in xs]
    xd[which] = unaligned_copy(xd[which])
    assert not aligned(*xd) and mr.mocov3_path(N, D, aligned(*xd))[0] == 'generic'
    _, lse, _ = fwd_lse(pkg, xd, 5.0)
    dp1, dp2 = pkg.engine.ops.nnclr_bwd(*xd, lse, 5.0)
    torch.cuda.synchronize()
    assert rel(dp1, t64(ref['dp1'])) <= BAR and rel(dp2, t64(ref['dp2'])) <= BAR


@pytest.mark.parametrize('N,D,K', [(33, 128, 100), (64, 256, 3075), (33, 130, 200)])
def test_deterministic(pkg, N, D, K):
    z1, z2, p1, p2, Q = (dev(x) for x in nr.step_inputs(N, D, K, seed=3))
    ops = pkg.engine.ops
    outs = []
    for _ in range(2):
        idx, sim, nn1, nn2 = ops.nnclr_search(z1, z2, Q)
        _, lse, _, _ = ops.mocov3_fwd(nn1, nn2, p1, p2, 5.0, w=nr.W)
        outs.append((idx, sim, nn1, nn2) + ops.nnclr_bwd(nn1, nn2, p1, p2, lse, 5.0))
    torch.cuda.synchronize()
    for a, b_ in zip(*outs):
        assert torch.equal(bits(a), bits(b_))


@pytest.mark.parametrize('N,D', [(33, 128), (257, 256), (33, 130)])
def test_gradient_scale(pkg, N, D):
    xd = [dev(x) for x in nr.bwd_float_inputs(N, D, seed=5)]
    ops = pkg.engine.ops
    _, lse, _ = fwd_lse(pkg, xd, 5.0)
    one = ops.nnclr_bwd(*xd, lse, 5.0)
    scaled = ops.nnclr_bwd(*xd, lse, 5.0, gscale_dev=torch.tensor([1024.0, 7.0], device=DEV))
    half = ops.nnclr_bwd(*xd, lse, 5.0, gscale_host=0.5)
    both = ops.nnclr_bwd(*xd, lse, 5.0, gscale_dev=torch.tensor([4.0], device=DEV), gscale_host=0.25)
    wide = ops.nnclr_bwd(*xd, lse, 5.0, w=1.0)
    torch.cuda.synchronize()
    for d in range(2):
        assert float(one[d].abs().max()) > 0
        assert torch.equal(bits(scaled[d]), bits(one[d] * 1024.0)) and torch.equal(bits(half[d]), bits(one[d] * 0.5))
        assert torch.equal(bits(both[d]), bits(one[d])) and torch.equal(bits(wide[d]), bits(one[d] * 2.0))


def test_refused_arguments_touch_nothing(pkg):
    lib, H = pkg._hip.lib, pkg._hip
    N, D, K = 8, 8, 12
    z1, z2, p1, p2, Q = (dev(x) for x in nr.step_inputs(N, D, K))
    SENT = 12345.0
    sim, nn1, nn2, dp1, dp2 = (torch.full((n,), SENT, device=DEV) for n in (2 * N + 1, N * D + 8, N * D + 8, N * D + 8, N * D + 8))
    idx = torch.full((2 * N + 1,), 777, dtype=torch.int32, device=DEV)
    lse = torch.zeros(2 * N, device=DEV)
    nb = max(lib.gca_nnclr_search_ws_bytes(N, D, K), lib.gca_nnclr_bwd_ws_bytes(N, D), 1 << 16)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    p = H.ptr
    nan, inf = float('nan'), float('inf')
    for bad in ((0, 8, 8), (65537, 1, 8), (8, 0, 8), (8, 8, 0), (8, 8, 2 ** 31), (65536, 32768, 8), (8, 32768, 65536), (-1, 8, 8)):
        assert lib.gca_nnclr_search_ws_bytes(*bad) == -1 and lib.gca_nnclr_search_path(*bad, 1, None, None) == EINVAL, bad
    assert lib.gca_nnclr_search_ws_bytes(1, 1, 1) > 0 and lib.gca_nnclr_bwd_ws_bytes(1, 1) > 0
    assert lib.gca_nnclr_bwd_ws_bytes(0, 8) == -1 and lib.gca_nnclr_bwd_ws_bytes(65536, 32768) == -1
    assert lib.gca_nnclr_bwd_path(0, 8, 1, None, None) == EINVAL

    def search(a=p(z1), b=p(z2), q=p(Q), N=N, D=D, K=K, ip=p(idx), sp=p(sim), n1=p(nn1), n2=p(nn2), wsp=p(ws), wb=nb):
        return lib.gca_nnclr_search(a, b, q, N, D, K, ip, sp, n1, n2, wsp, wb, H.stream())

    def bwd(a=p(nn1), b=p(nn2), c=p(p1), d=p(p2), N=N, D=D, inv_T=2.0, w=0.5, lp=p(lse), d1=p(dp1), d2=p(dp2), wsp=p(ws)):
        return lib.gca_nnclr_bwd(a, b, c, d, lp, N, D, inv_T, w, None, 1.0, d1, d2, wsp, H.stream())

    for kw in (dict(N=0), dict(N=-2), dict(N=65537, D=1), dict(D=0), dict(D=-1), dict(K=0), dict(K=-3), dict(K=2 ** 31),
               dict(N=65536, D=32768), dict(D=32768, K=65536), dict(a=None), dict(b=None), dict(q=None), dict(ip=None),
               dict(sp=None), dict(n1=None), dict(n2=None), dict(wsp=None), dict(wb=0), dict(wb=lib.gca_nnclr_search_ws_bytes(N, D, K) - 1),
               dict(n2=p(nn1)), dict(n2=p(nn1[4:])), dict(n1=p(Q)), dict(n2=p(Q[K - 1:])), dict(n1=p(z1)), dict(n2=p(z1)), dict(n1=p(z2)),
               dict(n2=p(z2))):
        assert search(**kw) == EINVAL, kw
    for kw in (dict(N=0), dict(N=65537, D=1), dict(D=0), dict(N=65536, D=32768), dict(inv_T=0.0), dict(inv_T=-1.0), dict(inv_T=inf),
               dict(inv_T=nan), dict(w=0.0), dict(w=-1.0), dict(w=inf), dict(w=nan), dict(a=None), dict(b=None), dict(c=None),
               dict(d=None), dict(lp=None), dict(d1=None), dict(d2=None), dict(wsp=None), dict(d1=p(p1)), dict(d2=p(p2)),
               dict(d1=p(nn1)), dict(d2=p(nn2)), dict(d2=p(dp1)), dict(d2=p(dp1[4:]))):
        assert bwd(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    for t in (sim, nn1, nn2, dp1, dp2):
        assert float(t.min()) == SENT == float(t.max())
    assert int(idx.min()) == 777 == int(idx.max())
    # the accepted calls write exactly their rows
    assert search() == 0
    _, lse2, _ = fwd_lse(pkg, [nn1[:N * D].view(N, D).clone(), nn2[:N * D].view(N, D).clone(), p1, p2], 2.0)
    lse.copy_(lse2)
    assert bwd() == 0
    torch.cuda.synchronize()
    assert int(idx[2 * N]) == 777 and int(idx[:2 * N].max()) < K and float(sim[2 * N]) == SENT and float(sim[:2 * N].max()) < SENT
    for t in (nn1, nn2, dp1, dp2):
        assert float(t[N * D:].min()) == SENT == float(t[N * D:].max()) and float(t[:N * D].abs().max()) < SENT


def test_ops_refuse_what_the_entries_refuse(pkg):
    ops = pkg.engine.ops
    z, Q = torch.zeros(4, 8, device=DEV), torch.zeros(6, 8, device=DEV)
    for args in ((z, torch.zeros(3, 8, device=DEV), Q), (z, z, torch.zeros(6, 9, device=DEV)), (z, z.double(), Q), (z, z, Q.double()),
                 (z[0], z[0], Q), (torch.zeros(0, 8, device=DEV), torch.zeros(0, 8, device=DEV), Q), (z, z, torch.zeros(0, 8, device=DEV))):
        with pytest.raises(ValueError, match='nnclr_search'):
            ops.nnclr_search(*args)
    for bad in (float('nan'), 0.0, -1.0, float('inf')):
        with pytest.raises(ValueError, match='nnclr_bwd'):
            ops.nnclr_bwd(z, z, z, z, torch.zeros(8, device=DEV), bad)
        with pytest.raises(ValueError, match='nnclr_bwd'):
            ops.nnclr_bwd(z, z, z, z, torch.zeros(8, device=DEV), 2.0, w=bad)
    with pytest.raises(ValueError, match='lse'):
        ops.nnclr_bwd(z, z, z, z, torch.zeros(4, device=DEV), 2.0)
    with pytest.raises(ValueError, match='gscale_host'):
        ops.nnclr_bwd(z, z, z, z, torch.zeros(8, device=DEV), 2.0, gscale_host=float('inf'))
    with pytest.raises(ValueError, match='nnclr_bwd'):
        ops.nnclr_bwd(z, z, z, torch.zeros(3, 8, device=DEV), torch.zeros(8, device=DEV), 2.0)
    assert ops.nnclr_weight() == 0.5


def eager_step(ops, z1, z2, p1, p2, Q, ptr_dev, K, inv_T):
    idx, sim, nn1, nn2 = ops.nnclr_search(z1, z2, Q)
    loss, lse, rank, _ = ops.mocov3_fwd(nn1, nn2, p1, p2, inv_T, w=nr.W, want_rank=True)
    dp1, dp2 = ops.nnclr_bwd(nn1, nn2, p1, p2, lse, inv_T)
    ops.queue_enqueue(Q, z1, 0, ptr_dev=ptr_dev)
    ops.queue_advance(ptr_dev, z1.shape[0], K)
    return idx, sim, loss, rank, dp1, dp2


def test_step_capturable_in_a_graph(pkg):
    """Search, mocov3_fwd, backward, enqueue and advance in ONE captured graph: three replays equal three eager steps bit for
    bit, the pointer wrap included (K = 10, N = 4: rows 0-3, 4-7, then 8, 9, 0, 1), and the specification step by step."""
    ops = pkg.engine.ops
    N, D, K, inv_T = 4, 32, 10, 5.0
    z1, z2, p1, p2, Q0 = (dev(x) for x in nr.step_inputs(N, D, K, seed=1))
    runs = {}
    for captured in (False, True):
        Q, ptr_dev = Q0.clone(), torch.zeros(1, dtype=torch.long, device=DEV)
        steps = []
        if captured:
            eager_step(ops, z1, z2, p1, p2, Q.clone(), ptr_dev.clone(), K, inv_T)          # workspaces exist before the capture
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                outs = eager_step(ops, z1, z2, p1, p2, Q, ptr_dev, K, inv_T)
        for _ in range(3):
            if captured:
                g.replay()
            else:
                outs = eager_step(ops, z1, z2, p1, p2, Q, ptr_dev, K, inv_T)
            torch.cuda.synchronize()
            steps.append(tuple(o.clone() for o in outs) + (Q.clone(), ptr_dev.clone()))
        runs[captured] = steps
        if captured:
            g.reset()
    for a, b_ in zip(runs[True], runs[False]):
        for x, y in zip(a, b_):
            assert torch.equal(bits(x) if x.is_floating_point() else x, bits(y) if y.is_floating_point() else y)
    Qn, index = Q0.cpu().numpy(), 0
    for k, st in enumerate(runs[True]):
        sr, ref, Qn, index = nr.module_step(z1.cpu().numpy(), z2.cpu().numpy(), p1.cpu().numpy(), p2.cpu().numpy(), Qn, index,
                                            np.float32(inv_T))
        assert np.array_equal(st[0].cpu().numpy().astype(np.int64), np.stack(sr['idx'])), k
        assert abs(float(st[2][0]) - ref['loss']) <= BAR * abs(ref['loss'])
        assert rel(st[4], t64(ref['dp1'])) <= BAR and rel(st[5], t64(ref['dp2'])) <= BAR
        assert same_bits(st[6], Qn) and int(st[7]) == index
    assert index == (3 * N) % K == 2


# ----------------------------------------------------------------------------- 4. the module
def test_module_forward_backward_and_queue(pkg):
    """Forward and backward against the specification; memory and index after three forwards with the wrap (K = 20, N = 8); the
    projections get no gradient."""
    import importlib
    NNCLRLoss = importlib.import_module(pkg.__name__ + '.lib.memory.nnclr').NNCLRLoss
    N, D, K, T = 8, 64, 20, 0.2
    z1n, z2n, p1n, p2n, Qn = nr.step_inputs(N, D, K, seed=2)
    crit = NNCLRLoss(D, K, T).to(DEV)
    crit.memory.copy_(dev(Qn))
    index = 0
    for k in range(3):
        sr, ref, Qn2, index2 = nr.module_step(z1n, z2n, p1n, p2n, Qn, index, np.float32(1.0 / T), g=3.0)
        z1, z2, p1, p2 = (dev(x).requires_grad_(True) for x in (z1n, z2n, p1n, p2n))
        loss = crit(z1, z2, p1, p2)
        assert loss.dim() == 0 and abs(float(loss.detach()) - ref['loss']) <= BAR * abs(ref['loss'])
        (loss * 3.0).backward()
        torch.cuda.synchronize()
        assert rel(p1.grad, t64(ref['dp1'])) <= BAR and rel(p2.grad, t64(ref['dp2'])) <= BAR
        assert z1.grad is None and z2.grad is None
        assert crit.idx.dtype is torch.int32 and tuple(crit.idx.shape) == (2, N) and tuple(crit.sim.shape) == (2, N)
        assert np.array_equal(crit.idx.cpu().numpy().astype(np.int64), np.stack(sr['idx'])), k
        assert rel(crit.sim, t64(np.stack(sr['sim']))) <= BAR
        assert crit.rank.dtype is torch.int32 and np.array_equal(crit.rank.cpu().numpy().astype(np.int64), np.stack(ref['rank']))
        assert abs(float(crit.l12) - ref['l'][0]) <= BAR * ref['l'][0] and abs(float(crit.l21) - ref['l'][1]) <= BAR * ref['l'][1]
        Qn, index = Qn2, index2
        assert crit.index == index and same_bits(crit.memory, Qn), k
    assert index == 4
    big = torch.zeros(K + 1, D, device=DEV)
    with pytest.raises(ValueError, match='cannot enqueue'):
        crit(big, big, big, big)
    assert crit.index == 4 and same_bits(crit.memory, Qn)


# ----------------------------------------------------------------------------- 5. model and trainer
def cpu_state(module):
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def test_model_against_the_fp64_oracle(pkg):
    import importlib
    import nnclr_model as nm
    from parity import check_grad_errors
    from test_nnclr_ref import nnclr_cfg
    NNCLRLoss = importlib.import_module(pkg.__name__ + '.lib.memory.nnclr').NNCLRLoss
    tr = pkg.NNCLRTrainer(nnclr_cfg(pkg), DEV, use_graph=False, seed=21)
    state = cpu_state(tr.model)
    x = nm.clip_batches(1, seed=31)[0]
    oracle = nm.oracle_nnclr('R2P1D10T', 8, nm.OUT, nm.HID, state)
    Q0 = nm.planted_queue(oracle, [x.double()], nm.LR, nm.TEMP, nm.QUEUE_K)
    want, rows, (idx64, gap) = nm.model_loss(oracle, x.double(), Q0.double(), nm.TEMP)
    assert float(gap.min()) > nm.GAP_BAR
    want.backward()
    crit = NNCLRLoss(nm.OUT, nm.QUEUE_K, nm.TEMP).to(DEV)
    crit.memory.copy_(Q0.to(DEV))
    tr.optimizer.zero_grad()
    m = tr.model.model
    x1, x2 = (v.contiguous() for v in torch.chunk(x.to(DEV), 2, dim=1))
    with torch.no_grad():
        tape_mod = importlib.import_module(pkg.__name__ + '.engine.tape')
        Tape, Var = tape_mod.Tape, tape_mod.Var
        z1, z2 = (m.fwd_zp(Tape(False), Var(v))[0].t for v in (x1, x2))
    p1, p2 = tr.model(x1), tr.model(x2)
    got = crit(z1, z2, p1, p2)
    got.backward()
    torch.cuda.synchronize()
    want = want.detach()
    e = dict(loss=abs(float(got.detach()) - float(want)) / abs(float(want)))
    for name, mine, ref in zip(('z1', 'z2', 'p1', 'p2'), (z1, z2, p1, p2), rows):
        e[name] = rel(mine, ref)
    print('MEASURED nnclr model loss %.6f vs oracle %.6f: rel err %s' % (float(got.detach()), float(want), ' '.join('%s %.3e' % kv for kv in e.items())))
    assert got.dim() == 0 and tuple(p1.shape) == (8, nm.OUT) and max(e.values()) < 1e-3, e
    assert torch.equal(crit.idx.cpu().long(), idx64)
    assert float((p1.detach().norm(dim=1) - 1).abs().max()) < 1e-5 and float((z1.norm(dim=1) - 1).abs().max()) < 1e-5
    g64 = {n: p.grad for n, p in oracle.named_parameters()}
    floor = 1e-9 * max(float(g.abs().max()) for g in g64.values() if g is not None)
    errs = {n: rel(p.grad, g64[n]) for n, p in tr.model.named_parameters() if g64[n] is not None and g64[n].abs().max() > floor}
    assert len(errs) > 40 and 'model.prediction.l2.weight' in errs and 'model.projection.l1.0.weight' in errs
    med, p95, worst = check_grad_errors(errs, 'nnclr parameter gradients')
    print('MEASURED nnclr model parameter gradients: median %.2e p95 %.2e worst %.2e over %d tensors' % (med, p95, worst, len(errs)))
    tr.close()


def test_trainer_graph_equals_eager_and_follows_the_oracle(pkg):
    """Three steps on three batches: the captured run equals the eager run bit for bit (losses, idx, parameters, support set,
    pointer), and idx exactly, losses, parameters and the support set within 1e-3 follow the fp64 step oracle -- whose own top-2
    gap on every row of every step is first shown to exceed 100x that bar."""
    import nnclr_model as nm
    from test_nnclr_ref import nnclr_cfg, oracle_run
    keys = ('loss', 'l12', 'l21', 'rank', 'idx', 'sim')
    runs, finals, run = {}, {}, None
    for use_graph in (True, False):
        tr = pkg.NNCLRTrainer(nnclr_cfg(pkg, WARMUP_FACTOR=1.0, BASE_LR=nm.LR), DEV, use_graph=use_graph, seed=nm.MODEL_SEED)
        if run is None:
            run = oracle_run(pkg, cpu_state(tr.model))
            assert min(run['gaps']) > nm.GAP_BAR, run['gaps']
        tr.contrast.memory.copy_(run['Q0'].to(DEV))
        outs = []
        for x in run['xs']:
            out = tr.train_step(x.to(DEV))
            torch.cuda.synchronize()
            assert set(out) >= set(keys) and out['idx'].dtype is torch.int32 and tuple(out['idx'].shape) == (2, 8)
            outs.append(tuple(out[k].detach().clone() for k in keys))
        assert (tr._segments[0].graph is not None) == use_graph
        assert int(tr.ptr_dev) == 24 == tr.contrast.index
        runs[use_graph] = outs
        finals[use_graph] = (tr.arena.flat.detach().clone(), tr.contrast.memory.detach().clone(), tr.ptr_dev.clone())
        state = cpu_state(tr.model)
        sd = tr.state_dict()
        assert list(sd['contrast']) == ['memory'] and sd['queue_index'] == 24
        tr.close()
    for ga, ea in zip(runs[True], runs[False]):
        for a, b_ in zip(ga, ea):
            assert torch.equal(bits(a) if a.is_floating_point() else a, bits(b_) if b_.is_floating_point() else b_)
    for a, b_ in zip(finals[True], finals[False]):
        assert torch.equal(bits(a) if a.is_floating_point() else a, bits(b_) if b_.is_floating_point() else b_)
    vals = [float(o[0]) for o in runs[False]]
    print('MEASURED nnclr trainer losses: %s  oracle: %s  top-2 gaps %s' % (' '.join('%.6f' % v for v in vals),
          ' '.join('%.6f' % v for v in run['losses']), ' '.join('%.4f' % g for g in run['gaps'])))
    for k, (o, idx64) in enumerate(zip(runs[False], run['idxs'])):
        assert torch.equal(o[4].cpu().long(), idx64), k
    for got, ref in zip(vals, run['losses']):
        assert abs(got - ref) <= 1e-3 * abs(ref), (vals, run['losses'])
    want = run['model'].state_dict()
    params = sorted(n for n, _ in run['model'].named_parameters())
    e_p = rel(torch.cat([state[k].reshape(-1) for k in params]), torch.cat([want[k].reshape(-1) for k in params]))
    e_q = rel(finals[False][1], run['Q'])
    print('MEASURED nnclr trainer after three steps: parameters %.2e support set %.2e' % (e_p, e_q))
    assert e_p <= 1e-3 and e_q <= 1e-3 and run['index'] == 24
    first = [float(v) for v in runs[False][0][:3]]
    assert abs(0.5 * (first[1] + first[2]) - first[0]) <= 1e-6 * abs(first[0])


def test_checkpoint_resume_is_exact_and_loads_downstream(pkg):
    """Save after step 2, resume in a fresh trainer built with another seed: step 3 is bitwise the uninterrupted run's (loss, idx,
    parameters, support set, device pointer)."""
    import copy
    import io
    import classify_model as cm
    import nnclr_model as nm
    from test_gpu_adam import action_cfg
    from test_nnclr_ref import nnclr_cfg
    cm.register()
    cfg = nnclr_cfg(pkg)
    cfg.CONTRAST.NCE_K = 20                                                    # 8 rows per step: the third step wraps
    xs = [x.to(DEV) for x in nm.clip_batches(3, seed=13)]
    a = pkg.NNCLRTrainer(cfg, DEV, use_graph=False, seed=5)
    for x in xs[:2]:
        a.train_step(x)
    sd = a.state_dict(epoch=7)
    assert set(sd) >= {'epoch', 'state_dict', 'optimizer', 'contrast', 'queue_index'} and sd['queue_index'] == 16
    buf = io.BytesIO()
    torch.save(sd, buf)
    b_ = pkg.NNCLRTrainer(cfg, DEV, use_graph=False, seed=99)
    assert b_.load_state_dict(torch.load(io.BytesIO(buf.getvalue()), map_location='cpu', weights_only=False)) == 7
    assert int(b_.ptr_dev) == 16 == b_.contrast.index and torch.equal(bits(b_.contrast.memory), bits(a.contrast.memory))
    oa, ob = a.train_step(xs[2]), b_.train_step(xs[2])
    torch.cuda.synchronize()
    assert torch.equal(bits(oa['loss']), bits(ob['loss'])) and torch.equal(oa['idx'], ob['idx']) and torch.equal(bits(oa['sim']), bits(ob['sim']))
    assert torch.equal(bits(a.arena.flat), bits(b_.arena.flat)) and torch.equal(bits(a.contrast.memory), bits(b_.contrast.memory))
    assert int(a.ptr_dev) == int(b_.ptr_dev) == 4 == a.contrast.index == b_.contrast.index
    sa, sb = a.model.state_dict(), b_.model.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.optimizer.buf, b_.optimizer.buf)
    assert all(k.startswith(('model.encoder.', 'model.projection.', 'model.prediction.')) for k in sd['state_dict'])
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


def test_trainer_refusals(pkg):
    import nnclr_model as nm
    from test_nnclr_ref import nnclr_cfg
    register_tiny(pkg)
    for mem in ('simsiam', 'moco', 'simclr', 'barlow', 'vicreg', 'swav', 'dino', 'mocov3'):
        with pytest.raises(ValueError, match='nnclr'):
            pkg.NNCLRTrainer(make_cfg(pkg, 'R2P1D10T', mem, 32, 16, 8), DEV)
    with pytest.raises(NotImplementedError, match='one GPU'):
        pkg.NNCLRTrainer(nnclr_cfg(pkg), DEV, ctx=pkg.parallel.DistCtx(force_active=True))
    for other in (pkg.SimCLRTrainer, pkg.MoCoV3Trainer, pkg.DINOTrainer):
        with pytest.raises(ValueError):
            other(nnclr_cfg(pkg), DEV)
    cfg = nnclr_cfg(pkg)
    cfg.CONTRAST.NCE_K = 6                                                     # N = 8 > K
    tr = pkg.NNCLRTrainer(cfg, DEV, use_graph=False, seed=3)
    mem = tr.contrast.memory.clone()
    with pytest.raises(ValueError, match='cannot enqueue'):
        tr.train_step(nm.clip_batches(1)[0].to(DEV))
    assert torch.equal(mem, tr.contrast.memory) and int(tr.ptr_dev) == 0 == tr.contrast.index
    tr.close()
