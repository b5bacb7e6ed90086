"""tests/nnclr_ref.py (the fp64 specification of the NNCLR kernels and module) held to torch's fp64 autograd of the literal loss, the
preconditions of the inputs that tests/test_gpu_nnclr.py relies on, the wrong variants that must miss the bar, the pointer wrap,
the dispatch rules against the library's, and the refusals and factories that need no GPU."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mocov3_ref as mr                  # noqa: E402
import nnclr_ref as nr                   # noqa: E402

BAR = 1e-5


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def chain64(z1, z2, p1, p2, Q, T):
    """torch fp64 autograd of torch_chain -> (loss, dp1, dp2, dz1, dz2)."""
    ts = [torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_(True) for x in (z1, z2, p1, p2)]
    loss = nr.torch_chain(*ts, torch.from_numpy(np.asarray(Q, dtype=np.float64)), T)
    loss.backward()
    return float(loss.detach()), ts[2].grad.numpy(), ts[3].grad.numpy(), ts[0].grad, ts[1].grad


# ----------------------------------------------------------------------------- the specification against autograd
@pytest.mark.parametrize('N,D,K', [(5, 32, 31), (33, 128, 100), (40, 130, 200)])
@pytest.mark.parametrize('T', nr.BWD_FLOAT_TS)
def test_specification_is_the_literal_loss(N, D, K, T):
    z1, z2, p1, p2, Q = nr.step_inputs(N, D, K)
    sr, ref, _, _ = nr.module_step(z1, z2, p1, p2, Q, 0, 1.0 / T)
    loss, dp1, dp2, dz1, dz2 = chain64(z1, z2, p1, p2, Q, T)
    assert abs(loss - ref['loss']) <= 1e-12 * abs(loss)
    assert rel(ref['dp1'], dp1) <= 1e-11 and rel(ref['dp2'], dp2) <= 1e-11
    assert dz1 is None and dz2 is None                                    # gradients to p only
    assert abs(ref['loss'] - nr.W * (ref['l'][0] + ref['l'][1])) <= 1e-15 * abs(loss)
    # the forward IS mocov3's with the roles (q1, q2, k1, k2) = (nn1, nn2, p1, p2) and w = 1/2
    m = mr.mocov3(sr['nn'][0], sr['nn'][1], p1, p2, 1.0 / T, w=nr.W)
    assert m['loss'] == ref['loss'] and np.array_equal(m['lse'][0], ref['lse'][0]) and np.array_equal(m['rank'][1], ref['rank'][1])


def test_search_specification_first_maximum_and_nan_key():
    Q = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [np.nan, 1.0]], dtype=np.float32)
    z = np.array([[1.0, 0.0], [0.0, 1.0], [0.5, 0.5], [np.nan, np.nan]], dtype=np.float32)
    r = nr.search_view(z, Q)
    # row 0: NaN * 0 is NaN, so column 3 is out; 0 and 2 tie -> 0.  row 1: column 1 (column 3 is NaN).  row 3: every key -inf -> 0
    assert r['idx'].tolist() == [0, 1, 0, 0] and r['sim'][:3].tolist() == [1.0, 1.0, 0.5] and r['sim'][3] == -np.inf
    assert nr.search_view(z, Q, last=True)['idx'].tolist() == [2, 1, 2, 3]
    assert np.array_equal(r['nn'][:3], Q[[0, 1, 0]])
    assert nr.top2_gap(r['s']).tolist()[:2] == [0.0, 1.0]


# ----------------------------------------------------------------------------- preconditions of the inputs
@pytest.mark.parametrize('case', nr.SEARCH_EXACT_CASES, ids=['N%d-D%d-K%d' % c for c in nr.SEARCH_EXACT_CASES])
def test_exact_scores_are_exact_in_fp32_under_any_order(case):
    N, D, K = case
    z1, z2, Q, _ = nr.exact_search_inputs(N, D, K)
    for z in (z1, z2):
        assert np.array_equal(z * 8, np.round(z * 8)) and np.abs(z).max() <= 1
        s64 = z.astype(np.float64) @ Q.astype(np.float64).T
        assert np.array_equal(s64 * 64, np.round(s64 * 64)) and np.abs(s64).max() <= D <= 2 ** 9
        # every partial sum of any order is a multiple of 1/64 below 2^9 in magnitude: 15 bits, exact in fp32 -- shown for three orders
        perm = np.random.RandomState(3).permutation(D)
        for order in (np.arange(D), np.arange(D)[::-1], perm):
            acc = np.zeros((z.shape[0], K), dtype=np.float32)
            for e in order:
                acc = acc + z[:, e:e + 1] * Q[None, :, e]
            assert np.array_equal(acc.astype(np.float64), s64)
    assert np.array_equal(Q * 8, np.round(Q * 8))


@pytest.mark.parametrize('case,path', list(zip(nr.SEARCH_EXACT_CASES, nr.SEARCH_EXACT_PATHS)),
                         ids=['N%d-D%d-K%d' % c for c in nr.SEARCH_EXACT_CASES])
def test_planted_ties_sit_where_the_gpu_tests_need_them(case, path):
    N, D, K = case
    z1, z2, Q, plants = nr.exact_search_inputs(N, D, K)
    name, waves, splits, tps = nr.search_path(N, D, K)
    assert name == path
    ref = nr.search(z1, z2, Q)
    bounds = nr.split_boundaries(N, D, K)
    assert bounds == [32 * tps * s for s in range(1, splits)] and all(b < K for b in bounds)
    seen = set()
    for view, row, cols, want in plants:
        s = ref['s'][view][row]
        assert all(s[c] == s.max() for c in cols) and ref['idx'][view][row] == want == min(cols)
        assert (s == s.max()).sum() == len(cols)                                  # nothing else reaches the planted maximum
        seen.add(cols)
    if D >= 32:
        if K >= 4 and N >= 2:
            assert (0, K - 1) in seen and (K - 1,) in seen                          # first / last column tie; a row whose maximum is its last column
            assert ref['idx'][1][N - 1] == K - 1
        if K >= 40 and N >= 2:
            assert (31, 32) in seen                                                 # across a tile edge
        for b in bounds:                                                            # both sides of EVERY split boundary
            assert (b - 1, b) in seen, b
        # the last-index rule would answer differently on every planted tie
        last = nr.search(z1, z2, Q, last=True)
        assert all(last['idx'][v][r] == max(c) for v, r, c, _ in plants)
    else:
        # small D: m / 8 values tie by themselves, in most rows
        ties = sum(int((ref['s'][v] == ref['s'][v].max(axis=1, keepdims=True)).sum(axis=1).max() > 1) for v in range(2))
        assert ties >= 1 or K == 1
    assert [c for c, p in zip(nr.SEARCH_EXACT_CASES, nr.SEARCH_EXACT_PATHS) if nr.search_path(*c)[2] >= 3].__len__() >= 2


def test_split_counts_of_the_search_cases():
    got = {c: nr.search_path(*c) for c in nr.SEARCH_EXACT_CASES}
    assert got[(33, 128, 100)] == ('fast', 4, 4, 1) and got[(64, 256, 3075)] == ('fast', 4, 97, 1)
    assert got[(33, 130, 200)] == ('generic', 1, 7, 1) and got[(4, 1, 40)] == ('generic', 1, 2, 1)
    assert got[(1, 8, 1)] == ('fast', 4, 1, 1) and got[(5, 32, 31)] == ('fast', 4, 1, 1)
    assert nr.search_path(64, 256, 65536) == ('fast', 4, 256, 8) and nr.search_path(64, 256, 98304) == ('fast', 4, 256, 12)
    assert nr.search_path(65, 256, 65536) == ('fast', 4, 128, 16)                 # three row tiles per view: two groups
    assert nr.search_path(64, 256, 65536, aligned=False) == ('generic', 1, 64, 32)
    assert nr.search_path(64, 260, 65536)[0] == 'generic' and nr.search_path(64, 254, 100)[0] == 'generic'
    assert nr.search_path(64, 256, 9600) == ('fast', 4, 150, 2)                   # 300 tiles: no empty split


def test_nan_case_inputs():
    N, D, K = nr.NAN_CASE
    z1, z2, Q, plants = nr.exact_search_inputs(N, D, K, nan=True)
    ref = nr.search(z1, z2, Q)
    assert np.isnan(Q[5]).all() and np.isnan(z2[3]).all() and not np.isnan(z1).any()
    assert ref['idx'][1][3] == 0 and ref['sim'][1][3] == -np.inf and not (np.stack(ref['idx']) == 5).any()
    assert len(plants) >= 4 and all(ref['idx'][v][r] == w for v, r, _, w in plants)


@pytest.mark.parametrize('N,D,K', nr.SEARCH_FLOAT_CASES + [(33, 128, 100)])
def test_every_float_row_is_clear(N, D, K):
    z1, z2, Q, des = nr.float_search_inputs(N, D, K)
    ref = nr.search(z1, z2, Q)
    for v, z in enumerate((z1, z2)):
        assert np.abs(np.linalg.norm(z.astype(np.float64), axis=1) - 1).max() < 1e-6
        smax = np.abs(ref['s'][v]).max()
        assert nr.top2_gap(ref['s'][v]).min() > 100 * nr.GAP * smax          # far above the condition the GPU comparison needs
        assert np.array_equal(ref['idx'][v], des[v])                           # the neighbour is the designated row
        assert 0.8 < ref['sim'][v].mean() < 0.97


def test_step_inputs_are_clear_at_every_step():
    """The inputs of the capture test (K = 10, N = 4) and of the module test (K = 20, N = 8), over three forwards with the wrap.  The
    same z1 is enqueued at every step, so from the third search on a row's maximum may be attained twice -- by bit-identical
    support rows, whose scores are the same number under any arithmetic that treats columns alike; everything else is far off."""
    for N, D, K, seed in ((4, 32, 10, 1), (8, 64, 20, 2)):
        z1, z2, p1, p2, Q = nr.step_inputs(N, D, K, seed=seed)
        index, tied = 0, 0
        for _ in range(3):
            sr, _, Q2, index2 = nr.module_step(z1, z2, p1, p2, Q, index, 5.0)
            for v in range(2):
                s = sr['s'][v]
                for i in range(N):
                    top = np.flatnonzero(s[i] == s[i].max())
                    assert all(np.array_equal(Q[j], Q[top[0]]) for j in top)
                    assert s[i].max() - s[i][s[i] < s[i].max()].max() > 100 * nr.GAP * np.abs(s).max()
                    tied += len(top) > 1
            Q, index = Q2, index2
        assert index == (3 * N) % K and tied > 0


def test_backward_input_properties():
    for N, D, _ in nr.HARD_CASES:
        nn1, nn2, p1, p2 = nr.bwd_float_inputs(N, D, hard=True)
        for x in (nn1, nn2, p1, p2):
            n = np.linalg.norm(x.astype(np.float64), axis=1)
            assert n.max() / n.min() > 3                                          # row norms spread (4x by construction)
        assert np.array_equal(nn1[0], p2[0]) and np.array_equal(nn2[0], p1[0])       # one p row equal to its neighbour
        u = nn1 / np.linalg.norm(nn1, axis=1, keepdims=True)
        assert np.abs(u @ u.T)[~np.eye(N, dtype=bool)].mean() > 0.3               # rows sharing a direction
    for N, D in nr.BWD_FLOAT_CASES:
        assert mr.mocov3_path(N, D)[0] == 'fast'
        nn1, nn2, p1, p2 = nr.bwd_float_inputs(N, D)
        for x in (nn1, nn2, p1, p2):
            assert np.abs(np.linalg.norm(x.astype(np.float64), axis=1) - 1).max() < 1e-6
        c = (nn1.astype(np.float64) * p2).sum(axis=1).mean()
        assert abs(c - nr.BWD_COS) < (0.2 if N == 5 else 0.08), (N, D, c)
    assert set(nr.BWD_FLOAT_TS) == {0.1, 0.2}


# ----------------------------------------------------------------------------- wrong variants must show
def _variants(kind, z1, z2, p1, p2, Q, index, inv_T):
    """-> (loss, dp1, new Q, idx) of a WRONG implementation."""
    sr, right, Q2, _ = nr.module_step(z1, z2, p1, p2, Q, index, inv_T)
    nn1, nn2 = sr['nn']
    N = z1.shape[0]
    coef = nr.W * inv_T
    if kind == 'softmax_over_rows':                 # the softmax over the neighbours instead of over the predictions
        m = mr.mocov3(p1, p2, nn1, nn2, inv_T, w=nr.W)               # rows p1 against columns nn2, rows p2 against columns nn1
        return m['loss'], m['dq'][0], Q2, sr['idx']
    if kind == 'gradient_to_rows':                  # mocov3's gradient (to the row operand), handed to p
        return right['loss'], right['dnn_rows'][1], Q2, sr['idx']
    if kind == 'post_enqueue_search':
        sr2 = nr.search(z1, z2, Q2)
        r = nr.nnclr(sr2['nn'][0], sr2['nn'][1], p1, p2, inv_T)
        return r['loss'], r['dp1'], Q2, sr2['idx']
    if kind == 'w_is_1':
        r = nr.nnclr(nn1, nn2, p1, p2, inv_T, w=1.0)
        return r['loss'], r['dp1'], Q2, sr['idx']
    if kind == 'enqueue_z2':
        return right['loss'], right['dp1'], nr.enqueue(Q, index, z2)[0], sr['idx']
    if kind == 'enqueue_p1':
        return right['loss'], right['dp1'], nr.enqueue(Q, index, p1)[0], sr['idx']
    raise KeyError(kind)


@pytest.mark.parametrize('kind', ['softmax_over_rows', 'gradient_to_rows', 'post_enqueue_search', 'w_is_1', 'enqueue_z2', 'enqueue_p1'])
@pytest.mark.parametrize('N,D,K', [(33, 128, 100), (40, 130, 200)])
def test_wrong_variants_miss_by_100_bars(N, D, K, kind):
    z1, z2, p1, p2, Q = nr.step_inputs(N, D, K)
    inv_T = 1.0 / nr.BWD_FLOAT_TS[0]
    _, right, Q2, _ = nr.module_step(z1, z2, p1, p2, Q, 3, inv_T)
    loss, dp1, Qw, idx = _variants(kind, z1, z2, p1, p2, Q, 3, inv_T)
    moved = max(abs(loss - right['loss']) / abs(right['loss']), rel(dp1, right['dp1']), rel(Qw, Q2))
    assert moved >= 100 * BAR, (kind, moved)


def test_last_index_tie_rule_shows_on_every_planted_tie():
    for case in nr.SEARCH_EXACT_CASES:
        z1, z2, Q, plants = nr.exact_search_inputs(*case)
        first, last = nr.search(z1, z2, Q), nr.search(z1, z2, Q, last=True)
        ties = [p for p in plants if len(p[2]) > 1]
        assert all(first['idx'][v][r] != last['idx'][v][r] for v, r, _, _ in ties)
        if case[1] >= 32 and case[2] >= 4 and case[0] >= 2:
            assert len(ties) >= 1


# ----------------------------------------------------------------------------- the pointer
def test_pointer_wrap():
    K, D = 10, 4
    Q = np.zeros((K, D), dtype=np.float32)
    rows = np.arange(1, 5, dtype=np.float32)[:, None] * np.ones((1, D), dtype=np.float32)
    index = 0
    for k in range(3):
        Q, index = nr.enqueue(Q, index, rows + 10 * k)
    assert index == 2 and Q[:, 0].tolist() == [23.0, 24.0, 3.0, 4.0, 11.0, 12.0, 13.0, 14.0, 21.0, 22.0]
    with pytest.raises(ValueError):
        nr.enqueue(Q, 0, np.zeros((11, D), dtype=np.float32))
    Q2, i2 = nr.enqueue(Q, 7, np.full((10, D), 5.0, dtype=np.float32))          # n == K: every row once
    assert i2 == 7 and (Q2 == 5.0).all()


# ----------------------------------------------------------------------------- dispatch
def test_dispatch_rules_are_the_librarys(pkg):
    import ctypes as C
    lib = pkg._hip.lib
    for N in (1, 31, 32, 33, 64, 65, 257, 4096, 65536):
        for D in (1, 4, 128, 130, 256, 260):
            for K in (1, 31, 32, 33, 100, 3075, 9600, 65536, 98304):
                if N * D >= 2 ** 31 or K * D >= 2 ** 31:
                    continue
                for al in (0, 1):
                    w, s = C.c_int32(-1), C.c_int32(-1)
                    rc = lib.gca_nnclr_search_path(N, D, K, al, C.addressof(w), C.addressof(s))
                    assert (('generic', 'fast')[rc], w.value, s.value) == nr.search_path(N, D, K, bool(al))[:3], (N, D, K, al)
                assert lib.gca_nnclr_search_ws_bytes(N, D, K) >= 16 * N * max(nr.search_path(N, D, K, a)[2] for a in (False, True))
            for al in (0, 1):
                w, s = C.c_int32(-1), C.c_int32(-1)
                rc = lib.gca_nnclr_bwd_path(N, D, al, C.addressof(w), C.addressof(s))
                assert (('generic', 'fast')[rc], w.value, s.value) == mr.mocov3_path(N, D, bool(al)), (N, D, al)
            assert lib.gca_nnclr_bwd_ws_bytes(N, D) > 0
    for N, D, K in ((0, 8, 8), (-1, 8, 8), (65537, 8, 8), (8, 0, 8), (8, 8, 0), (8, 8, 2 ** 31), (65536, 32768, 8), (8, 32768, 65536)):
        assert lib.gca_nnclr_search_path(N, D, K, 1, None, None) == -1 and lib.gca_nnclr_search_ws_bytes(N, D, K) == -1
    for N, D in ((0, 8), (65537, 8), (8, 0), (65536, 32768)):
        assert lib.gca_nnclr_bwd_path(N, D, 1, None, None) == -1 and lib.gca_nnclr_bwd_ws_bytes(N, D) == -1


def test_refused_entry_arguments_without_a_device(pkg):
    """The entries check sizes, NULLs, the workspace and overlaps before anything is launched: host pointers are enough."""
    import ctypes as C
    lib = pkg._hip.lib
    N, D, K = 4, 8, 6
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    z1, z2, Q, nn1, nn2, sim, idx, ws = (base + 4 * o for o in (0, 64, 128, 256, 320, 384, 448, 1024))
    nb = lib.gca_nnclr_search_ws_bytes(N, D, K)

    def search(**kw):
        a = dict(z1=z1, z2=z2, Q=Q, N=N, D=D, K=K, idx=idx, sim=sim, nn1=nn1, nn2=nn2, ws=ws, wb=nb)
        a.update(kw)
        return lib.gca_nnclr_search(a['z1'], a['z2'], a['Q'], a['N'], a['D'], a['K'], a['idx'], a['sim'], a['nn1'], a['nn2'], a['ws'],
                                    a['wb'], None)
    for kw in (dict(N=0), dict(N=65537), dict(D=0), dict(K=0), dict(K=2 ** 31), dict(z1=None), dict(z2=None), dict(Q=None),
               dict(idx=None), dict(sim=None), dict(nn1=None), dict(nn2=None), dict(ws=None), dict(wb=nb - 1), dict(nn2=nn1),
               dict(nn2=nn1 + 16), dict(nn1=Q + 4 * (K * D - 1)), dict(nn1=z1), dict(nn2=z2), dict(nn1=z2 + 4)):
        assert search(**kw) == -1, kw

    def bwd(**kw):
        a = dict(nn1=z1, nn2=z2, p1=Q, p2=Q + 256, lse=sim, N=N, D=D, inv_T=5.0, w=0.5, dp1=nn1, dp2=nn2, ws=ws)
        a.update(kw)
        return lib.gca_nnclr_bwd(a['nn1'], a['nn2'], a['p1'], a['p2'], a['lse'], a['N'], a['D'], a['inv_T'], a['w'], None, 1.0,
                                 a['dp1'], a['dp2'], a['ws'], None)
    for kw in (dict(N=0), dict(D=0), dict(N=65537), dict(inv_T=0.0), dict(inv_T=float('nan')), dict(inv_T=float('inf')), dict(w=0.0),
               dict(w=-0.5), dict(w=float('nan')), dict(nn1=None), dict(p2=None), dict(lse=None), dict(dp1=None), dict(dp2=None),
               dict(ws=None), dict(dp2=nn1), dict(dp2=nn1 + 4), dict(dp1=z1), dict(dp1=Q), dict(dp2=Q + 256), dict(dp2=z2 + 8)):
        assert bwd(**kw) == -1, kw


# ----------------------------------------------------------------------------- the host layers
def test_ops_refuse_before_any_device_is_touched(pkg):
    ops = pkg.engine.ops
    z, Q = torch.zeros(4, 8), torch.zeros(6, 8)
    for args in ((z, torch.zeros(3, 8), Q), (z, z, torch.zeros(6, 9)), (z.double(), z, Q), (z, z, Q.double()), (z[0], z[0], Q),
                 (z, z, Q[0]), (torch.zeros(0, 8), torch.zeros(0, 8), Q), (z, z, torch.zeros(0, 8)),
                 (torch.zeros(65537, 1), torch.zeros(65537, 1), torch.zeros(2, 1))):
        with pytest.raises(ValueError, match='nnclr_search'):
            ops.nnclr_search(*args)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.nnclr_search(z, z, Q)
    for bad in (0.0, -1.0, float('nan'), float('inf'), 1e39):
        with pytest.raises(ValueError, match='nnclr_bwd'):
            ops.nnclr_bwd(z, z, z, z, torch.zeros(8), bad)
        with pytest.raises(ValueError, match='nnclr_bwd'):
            ops.nnclr_bwd(z, z, z, z, torch.zeros(8), 5.0, w=bad)
    with pytest.raises(ValueError, match='nnclr_bwd'):
        ops.nnclr_bwd(z, z, z, torch.zeros(3, 8), torch.zeros(8), 5.0)
    with pytest.raises(ValueError, match='lse'):
        ops.nnclr_bwd(z, z, z, z, torch.zeros(4), 5.0)
    for gs in (float('inf'), float('nan'), 1e39):
        with pytest.raises(ValueError, match='gscale_host'):
            ops.nnclr_bwd(z, z, z, z, torch.zeros(8), 5.0, gscale_host=gs)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.nnclr_bwd(z, z, z, z, torch.zeros(8), 5.0)
    assert ops.nnclr_weight() == 0.5 == nr.W


def nnclr_cfg(pkg, **solver):
    from tests import parity
    import nnclr_model as nm
    parity.register_tiny(pkg)
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'nnclr', nm.OUT, nm.QUEUE_K, 8, **solver)
    cfg.CONTRAST.NCE_T = nm.TEMP
    cfg.CONTRAST.NN_HID = nm.HID
    return cfg


def test_factories(pkg):
    from tests import parity
    import nnclr_model as nm
    NNCLRLoss = importlib.import_module(pkg.__name__ + '.lib.memory.nnclr').NNCLRLoss
    build = importlib.import_module(pkg.__name__ + '.lib.modeling.build')
    gw = importlib.import_module(pkg.__name__ + '.lib.modeling.graph_wrappers')
    assert pkg.get_defaults().CONTRAST.NN_HID == 2048 and hasattr(pkg, 'NNCLRTrainer')
    cfg = nnclr_cfg(pkg)
    torch.manual_seed(3)
    c = pkg.create_contrast(cfg, 100)
    assert isinstance(c, NNCLRLoss) and c.T == nm.TEMP and c.K == nm.QUEUE_K and c.index == 0
    assert all(getattr(c, k) is None for k in ('idx', 'sim', 'rank', 'l12', 'l21'))
    assert list(c.state_dict()) == ['memory'] and tuple(c.memory.shape) == (nm.QUEUE_K, nm.OUT)
    assert float((c.memory.norm(dim=1) - 1).abs().max()) < 1e-6                 # normalised randn, as RGBMoCo's
    for bad in (0.0, -0.2, float('nan'), float('inf'), 1e-39):
        with pytest.raises(ValueError, match='NNCLRLoss'):
            NNCLRLoss(8, 16, bad)
    for bad in (dict(n_dim=0), dict(K=0), dict(K=2.5), dict(n_dim=True)):
        with pytest.raises(ValueError, match='NNCLRLoss'):
            NNCLRLoss(**{**dict(n_dim=8, K=16, T=0.1), **bad})
    z = torch.zeros(4, nm.OUT)
    for args in ((z, torch.zeros(4, 9), z, z), (z, z, torch.zeros(5, nm.OUT), z), (z, z, z, torch.zeros(4, 7)), (z[0], z[0], z[0], z[0])):
        with pytest.raises(ValueError, match='NNCLRLoss'):
            c(*args)
    big = torch.zeros(nm.QUEUE_K + 1, nm.OUT)
    with pytest.raises(ValueError, match='cannot enqueue'):                     # N > K, before any device is touched
        c(big, big, big, big)
    assert c.index == 0
    # the model factory: one model, no second one; SimSiam's names in MoCoV3's registration order
    torch.manual_seed(5)
    model, ema = build.create_visual_model(cfg)
    assert isinstance(model.model, gw.NNCLR) and ema is None
    assert [n for n, _ in model.model.named_children()] == ['encoder', 'projection', 'prediction']
    sk = list(model.state_dict())
    st = model.state_dict()
    assert tuple(st['model.projection.l1.0.weight'].shape) == (nm.HID, model.model.feature_dim)
    assert tuple(st['model.projection.l3.0.weight'].shape) == (nm.OUT, nm.HID)
    assert tuple(st['model.prediction.l1.0.weight'].shape) == (nm.HID, nm.OUT) and tuple(st['model.prediction.l2.weight'].shape) == (nm.OUT, nm.HID)
    assert {k[len('model.'):] for k in sk} == set(gw.SimSiam(build._encoder(cfg), nm.OUT).state_dict())
    v3 = parity.make_cfg(pkg, 'R2P1D10T', 'mocov3', nm.OUT, 16, 8)
    v3.CONTRAST.V3_HID = nm.HID
    assert list(build.create_visual_model(v3)[0].state_dict()) == sk                # MoCoV3's order
    for bad in (dict(out_dim=0), dict(hid_dim=0), dict(out_dim=2.5), dict(hid_dim=True)):
        with pytest.raises(ValueError, match='NNCLR'):
            gw.NNCLR(model.model.encoder, **{**dict(out_dim=32, hid_dim=48), **bad})
    # the oracle reads the same state
    nm.oracle_nnclr('R2P1D10T', 8, nm.OUT, nm.HID, {k: v.detach().clone() for k, v in st.items()})


def test_trainer_refusals_without_a_device(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    for mem in ('simsiam', 'moco', 'simclr', 'mocov3'):
        with pytest.raises(ValueError, match='nnclr'):
            pkg.NNCLRTrainer(parity.make_cfg(pkg, 'R2P1D10T', mem, 32, 16, 8), 'cpu')
    with pytest.raises(NotImplementedError, match='one GPU'):
        pkg.NNCLRTrainer(nnclr_cfg(pkg), 'cpu', ctx=pkg.parallel.DistCtx(force_active=True))
    for other in (pkg.SimCLRTrainer, pkg.DINOTrainer, pkg.MoCoV3Trainer):
        with pytest.raises(ValueError):
            other(nnclr_cfg(pkg), 'cpu')


# ----------------------------------------------------------------------------- the trainer test's oracle run
def oracle_run(pkg, state=None):
    """The three oracle steps the GPU trainer test follows -> (state, xs, Q0, losses, idxs, gaps, final Q, index, model)."""
    import nnclr_model as nm
    cfg = nnclr_cfg(pkg, WARMUP_FACTOR=1.0, BASE_LR=nm.LR)
    if state is None:                                                            # the trainer's own initialisation, on the CPU
        build = importlib.import_module(pkg.__name__ + '.lib.modeling.build')
        torch.manual_seed(nm.MODEL_SEED)
        state = {k: v.detach().clone() for k, v in build.create_visual_model(cfg)[0].state_dict().items()}
    xs = nm.clip_batches()
    x64 = [x.double() for x in xs]
    model = nm.oracle_nnclr('R2P1D10T', 8, nm.OUT, nm.HID, state)
    Q0 = nm.planted_queue(model, x64, nm.LR, nm.TEMP, nm.QUEUE_K)
    Q = Q0.double().clone()
    losses, idxs, gaps, _, index = nm.oracle_steps(model, Q, 0, x64, nm.LR, nm.TEMP)
    return dict(cfg=cfg, state=state, xs=xs, Q0=Q0, losses=losses, idxs=idxs, gaps=gaps, Q=Q, index=index, model=model)


def test_the_oracles_neighbours_are_clear_at_every_step(pkg):
    import nnclr_model as nm
    run = oracle_run(pkg)
    print('MEASURED nnclr oracle top-2 gaps per step: %s (bar %.1e)' % (' '.join('%.4f' % g for g in run['gaps']), nm.GAP_BAR))
    assert min(run['gaps']) > nm.GAP_BAR                                         # 100x the 1e-3 feature bar
    assert run['index'] == 24 and all(np.isfinite(run['losses']))
    assert float((run['Q0'].norm(dim=1) - 1).abs().max()) < 1e-6


# ----------------------------------------------------------------------------- what fp32 arithmetic alone costs
def test_fp32_cpu_chain_leaves_room_under_the_bar():
    worst = dict(loss=(0.0, None), dp=(0.0, None))
    cases = [(nr.bwd_float_inputs(N, D), T, 'unit N=%d D=%d T=%g' % (N, D, T)) for N, D in nr.BWD_FLOAT_CASES for T in nr.BWD_FLOAT_TS]
    cases += [(nr.bwd_float_inputs(N, D, hard=True), nr.HARD_T, 'hard N=%d D=%d' % (N, D)) for N, D, _ in nr.HARD_CASES]
    for xs, T, tag in cases:
        ref = nr.nnclr(*xs, np.float32(1.0 / T))
        nn1, nn2 = (torch.from_numpy(x) for x in xs[:2])
        p1, p2 = (torch.from_numpy(x).requires_grad_(True) for x in xs[2:])
        target = torch.arange(nn1.shape[0])
        F = torch.nn.functional
        loss = 0.5 * (F.cross_entropy(nn1 @ p2.t() / T, target) + F.cross_entropy(nn2 @ p1.t() / T, target))
        loss.backward()
        e_l = abs(float(loss.detach()) - ref['loss']) / abs(ref['loss'])
        e_d = max(rel(p1.grad.numpy(), ref['dp1']), rel(p2.grad.numpy(), ref['dp2']))
        if e_l > worst['loss'][0]:
            worst['loss'] = (e_l, tag)
        if e_d > worst['dp'][0]:
            worst['dp'] = (e_d, tag)
    print('MEASURED nnclr cpu chain (fp32 torch ops against fp64): loss %.3e (%s)  dp %.3e (%s)  [bar %.0e]'
          % (worst['loss'][0], worst['loss'][1], worst['dp'][0], worst['dp'][1], BAR))
    assert worst['loss'][0] <= BAR / 4 and worst['dp'][0] <= BAR / 4
