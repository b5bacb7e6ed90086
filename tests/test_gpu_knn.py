"""gca_knn_vote / ops.knn_vote, lib.evaluation.knn and the staged feature pass on the device, against tests/knn_ref.py.

Uniform weights: scores, pred and rank must be the bits of the order32 specification (sums of ones are exact; class ties go
to the lower index).  Exp weights: scores within rtol 2e-5 of the fp64 specification on the same fp32 distances -- at most 64
positive terms: summation 63 * 2^-24, the rounded product |dist / T| * 2^-24 <= 40 * 2^-24, expf <= 3 ulp, together about
6.3e-6, the bar about three times that -- and pred / rank exact, which tests/test_knn_ref.py makes sound by asserting a
relative gap of 1e-3 around every compared score of these seeded inputs.

Measured on an MI355X (printed by test_exp_weights_float_cases), max |score - fp64| / fp64 per temperature over all cases:
    T = 0.05  1.95e-6 (k = 64)     T = 0.07  9.51e-7 (k = 63)     T = 1.0  1.35e-7 (k = 63)     [bar 2e-5]
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_cases as kc                   # noqa: E402
import knn_ref as kr                     # noqa: E402
import retrieval_cases as rcases         # noqa: E402
import retrieval_ref as rref             # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
RTOL = 2e-5
EINVAL = -1


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def run(pkg, c, kvote=None, weighting='exp', T=0.07, scores=True, labelled=True):
    """ops.knn_vote on a case of knn_cases -> numpy (scores | None, pred, rank | None)."""
    ql = dev(c['q_label']) if labelled else None
    pred, rank, s = pkg.engine.ops.knn_vote(dev(c['idx']), dev(c['dist']), dev(c['g_label']), c['C'], kvote=kvote, q_label=ql,
                                            self_base=c.get('self_base', -1), weighting=weighting, T=T, want_scores=scores)
    nq = c['idx'].shape[0]
    assert pred.dtype is torch.int32 and tuple(pred.shape) == (nq,)
    assert (rank is None) == (not labelled) and (s is None) == (not scores)
    assert rank is None or (rank.dtype is torch.int32 and tuple(rank.shape) == (nq,))
    assert s is None or (s.dtype is torch.float32 and tuple(s.shape) == (nq, c['C']))
    return (None if s is None else s.cpu().numpy(), pred.cpu().numpy(), None if rank is None else rank.cpu().numpy())


def spec(c, kvote, weighting, T=0.07, order32=False):
    return kr.vote(c['idx'], c['dist'], c['g_label'], c['C'], kvote, c['q_label'], c.get('self_base', -1), weighting, T, order32)


def assert_bits(got, want):
    (s, p, r), (ws, wp, wr) = got, want
    assert np.array_equal(p, wp) and np.array_equal(r, wr)
    assert s.dtype == ws.dtype == np.float32 and np.array_equal(s.view(np.uint32), ws.view(np.uint32))


# ----------------------------------------------------------------------------- uniform weights: the specification's bits
@pytest.mark.parametrize('name', ['content', 'distinct', 'loo'])
def test_uniform_weights_content_cases(pkg, name):
    c = {'content': kc.content_case, 'distinct': kc.distinct_classes_case, 'loo': kc.loo_case}[name]()
    for kv in kc.kvotes(c['idx'].shape[1]) + ([3] if name == 'loo' else []):
        assert_bits(run(pkg, c, kv, 'uniform'), spec(c, kv, 'uniform', order32=True))


@pytest.mark.parametrize('case', kc.FLOAT_CASES, ids=lambda s: 'nq%d-k%d-C%d' % s[:3])
def test_uniform_weights_shapes(pkg, case):
    c = kc.float_case(*case)
    for kv in kc.kvotes(case[1]):
        assert_bits(run(pkg, c, kv, 'uniform'), spec(c, kv, 'uniform', order32=True))


# ----------------------------------------------------------------------------- exp weights
@pytest.mark.parametrize('T', kc.TS)
@pytest.mark.parametrize('case', kc.FLOAT_CASES, ids=lambda s: 'nq%d-k%d-C%d' % s[:3])
def test_exp_weights_float_cases(pkg, case, T):
    c = kc.float_case(*case)
    worst = 0.0
    for kv in kc.kvotes(case[1]):
        s, p, r = run(pkg, c, kv, 'exp', T)
        ws, wp, wr = spec(c, kv, 'exp', T)
        voted = ws > 0
        assert not s[~voted].any()                                       # a class without voters is exactly 0
        err = np.abs(s[voted].astype(np.float64) - ws[voted]) / ws[voted]
        worst = max(worst, float(err.max()) if err.size else 0.0)
        print('knn exp %r T=%g kvote=%d: max |score - fp64| / fp64 = %.3e (bar %.1e)' % (case[:3], T, kv, err.max() if err.size else 0, RTOL))
        assert (err <= RTOL).all()
        assert np.array_equal(p, wp) and np.array_equal(r, wr)          # exact: the gaps are asserted in test_knn_ref.py
    assert worst <= RTOL


@pytest.mark.parametrize('T', kc.TS)
def test_exp_weights_content_case(pkg, T):
    """Tail, NaN, +inf (weight 0), dist = 0 (weight 1) and dist = 2 slots under exp weights; rows without voters."""
    c = kc.content_case()
    for kv in kc.kvotes(8):
        s, p, r = run(pkg, c, kv, 'exp', T)
        ws, wp, wr = spec(c, kv, 'exp', T)
        assert np.isfinite(s).all() and np.array_equal(s == 0, ws == 0)
        assert np.allclose(s, ws, rtol=RTOL, atol=0)
        assert np.array_equal(p == -1, wp == -1) and np.array_equal(r[wp == -1], wr[wp == -1])
    i = c['what'].index('dist 0 and 2')
    s = run(pkg, c, None, 'exp', T)[0]
    assert s[i, 2] == 2.0                                                # two voters at distance 0: weight exactly 1 each


def test_repeated_calls_give_the_same_bits(pkg):
    c = kc.float_case(9, 64, 101, 0)
    a, b = run(pkg, c, 63, 'exp'), run(pkg, c, 63, 'exp')
    assert_bits(a, b)


def test_without_scores_and_without_query_labels(pkg):
    for c in (kc.float_case(9, 64, 101, 0), kc.content_case()):
        full = run(pkg, c, None, 'exp')
        s, p, r = run(pkg, c, None, 'exp', scores=False)
        assert s is None and np.array_equal(p, full[1]) and np.array_equal(r, full[2])
        s, p, r = run(pkg, c, None, 'exp', labelled=False)
        assert r is None and np.array_equal(p, full[1]) and np.array_equal(s.view(np.uint32), full[0].view(np.uint32))
        s, p, r = run(pkg, c, None, 'exp', scores=False, labelled=False)
        assert s is None and r is None and np.array_equal(p, full[1])


# ----------------------------------------------------------------------------- the entry's refusals
def test_invalid_arguments_launch_nothing(pkg):
    H = pkg._hip
    c = kc.float_case(5, 63, 2, 0)
    nq, k, C, ng = 5, 63, 2, c['ng']
    idx, dist, gl, ql = dev(c['idx']), dev(c['dist']), dev(c['g_label']), dev(c['q_label'])
    scores = torch.full((nq, C), 77.0, device=DEV)
    pred = torch.full((nq,), 77, dtype=torch.int32, device=DEV)
    rank = torch.full((nq,), 77, dtype=torch.int32, device=DEV)
    base = dict(idx=idx, dist=dist, nq=nq, k=k, kvote=k, gl=gl, ng=ng, ql=ql, self_base=-1, C=C, weighting=1, inv_T=1.0,
                scores=scores, pred=pred, rank=rank)

    def entry(**kw):
        a = dict(base, **kw)
        p = lambda t: None if t is None else t.data_ptr()               # noqa: E731
        return H.lib.gca_knn_vote(p(a['idx']), p(a['dist']), a['nq'], a['k'], a['kvote'], p(a['gl']), a['ng'], p(a['ql']),
                                  a['self_base'], a['C'], a['weighting'], a['inv_T'], p(a['scores']), p(a['pred']), p(a['rank']),
                                  H.stream())
    torch.cuda.synchronize()
    refused = [dict(k=0, kvote=0), dict(k=0, kvote=1), dict(k=65, kvote=1), dict(k=-1), dict(kvote=0), dict(kvote=k + 1), dict(kvote=-1),
               dict(C=0), dict(C=-1), dict(nq=-1), dict(ng=-1), dict(ng=2 ** 31), dict(C=2 ** 31 // nq + 1),      # nq * C >= 2^31
               dict(nq=2 ** 31 // C), dict(weighting=2), dict(weighting=-1), dict(inv_T=-1.0), dict(inv_T=float('inf')),
               dict(inv_T=float('nan')), dict(ql=None), dict(idx=None), dict(dist=None), dict(gl=None), dict(pred=None)]
    for kw in refused:
        assert entry(**kw) == EINVAL, kw
    assert entry(nq=0) == 0                                              # nothing to do, nothing launched
    assert entry(nq=0, idx=None, dist=None, gl=None, pred=None, scores=None, rank=None, ql=None) == 0
    torch.cuda.synchronize()
    assert bool((scores == 77.0).all()) and bool((pred == 77).all()) and bool((rank == 77).all())
    assert entry(C=2 ** 31 // nq + 1, scores=None) == 0                  # without scores C has no such limit
    torch.cuda.synchronize()
    assert bool((scores == 77.0).all())
    assert entry() == 0
    torch.cuda.synchronize()
    ws, wp, wr = spec(c, k, 'exp', 1.0)
    assert np.array_equal(pred.cpu().numpy(), wp) and np.array_equal(rank.cpu().numpy(), wr)
    assert np.allclose(scores.cpu().numpy(), ws, rtol=RTOL, atol=0)


def test_no_queries(pkg):
    ops = pkg.engine.ops
    gl = torch.zeros(9, dtype=torch.int64, device=DEV)
    pred, rank, s = ops.knn_vote(torch.empty(0, 5, dtype=torch.int32, device=DEV), torch.empty(0, 5, device=DEV), gl, 4,
                                 q_label=torch.empty(0, dtype=torch.int64, device=DEV), want_scores=True)
    assert tuple(pred.shape) == (0,) and tuple(rank.shape) == (0,) and tuple(s.shape) == (0, 4)


# ----------------------------------------------------------------------------- end to end on exact operands
def _counts(rank):
    return {'top1': int((rank < 1).sum()), 'top5': int((rank < 5).sum())}


def test_knn_classify_equals_search_then_vote_specification(pkg):
    """retrieval_cases.cosine_case: the search is bit-exact on these operands, so under uniform weights the counts are exact."""
    K = pkg.lib.evaluation.knn
    q, g = rcases.cosine_case()
    rs = np.random.RandomState(17)
    gl, ql, C = rs.randint(0, 9, size=len(g)), rs.randint(0, 9, size=len(q)), 9
    ks = (1, 5, 20, 64)
    idx, dist, _ = rref.topk(q, g, 64, 'cosine', dtype=np.float32)
    want = {k: _counts(kr.vote(idx, dist, gl, C, k, ql, weighting='uniform')[2]) for k in ks}
    got, total = K.knn_classify(g, gl, q, ql, ks=ks, weighting='uniform', device=DEV)
    assert total == len(q) and got == want
    assert K.knn_classify(torch.from_numpy(g).to(DEV), gl, torch.from_numpy(q).to(DEV), ql, num_class=C, ks=ks, weighting='uniform')[0] == want
    pred = K.knn_predict(g, gl, q, C, k=20, weighting='uniform', device=DEV)
    assert np.array_equal(pred.cpu().numpy(), kr.vote(idx, dist, gl, C, 20, weighting='uniform')[1])
    # exp weights: the counts of the fp64 vote wherever its gaps carry the comparison
    s64, _, r64 = kr.vote(idx, dist, gl, C, 20, ql, weighting='exp', T=0.07)
    if kr.gaps(s64, ql).min() >= kc.GAP:
        assert K.knn_classify(g, gl, q, ql, ks=(20,), T=0.07, device=DEV)[0] == {20: _counts(r64)}


def test_leave_one_out_equals_specification_for_two_chunk_sizes(pkg):
    K = pkg.lib.evaluation.knn
    _, g = rcases.cosine_case()
    gl, C = np.random.RandomState(18).randint(0, 9, size=len(g)), 9
    ks = (1, 5, 20, 63)
    idx, dist, _ = rref.topk(g, g, 64, 'cosine', dtype=np.float32)
    assert (idx[:, 0] != np.arange(len(g))).any()                       # duplicated rows: a row is not always its own nearest
    want = {k: _counts(kr.vote(idx, dist, gl, C, k, gl, self_base=0, weighting='uniform')[2]) for k in ks}
    a, n = K.knn_classify_loo(g, gl, ks=ks, weighting='uniform', chunk=4096, device=DEV)
    b, _ = K.knn_classify_loo(g, gl, ks=ks, weighting='uniform', chunk=130, device=DEV)
    assert n == len(g) and a == want and b == want


# ----------------------------------------------------------------------------- plumbing on the tiny backbone
T_CLIP, SIZE = 8, 48
BANK_C, QUERY_C, NUM_CLASS = [0, 1, 2, 3, 4, 5], [2, 0, 7, 5], 8


@pytest.fixture(scope='module')
def tiny(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    return parity


def _trainer(pkg, tiny, seed=5):
    return pkg.MoCoTrainer(tiny.make_cfg(pkg, 'R2P1D10T', 'moco', 32, 20, T_CLIP), DEV, use_graph=False, seed=seed)


def _step_input(seed):
    return torch.randn(8, 6, T_CLIP, SIZE, SIZE, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _batches(seed, classes):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(2, 3, T_CLIP, SIZE, SIZE, generator=gen), torch.tensor(classes[i:i + 2])) for i in range(0, len(classes), 2)]


def test_monitor_equals_knn_classify_on_extracted_features(pkg, tiny):
    E = pkg.lib.evaluation
    trainer = _trainer(pkg, tiny)
    trainer.train_step(_step_input(3))
    bank, query = _batches(31, BANK_C), _batches(32, QUERY_C)
    mon = E.KNNMonitor(trainer.cfg, bank, query, NUM_CLASS, k=4, T=0.07, device=DEV)
    res = mon.evaluate(trainer)
    enc = E.load_encoder(trainer.state_dict(), 'R2P1D10T', T_CLIP).to(DEV)
    g = torch.cat([E.extract_feature_single(enc, d.to(DEV), 1, T_CLIP) for d, _ in bank])
    q = torch.cat([E.extract_feature_single(enc, d.to(DEV), 1, T_CLIP) for d, _ in query])
    counts, total = E.knn_classify(g, BANK_C, q, QUERY_C, num_class=NUM_CLASS, ks=(4,), T=0.07)
    r1, _ = E.topk_retrieval(g.cpu().numpy(), np.array(BANK_C), q.cpu().numpy(), np.array(QUERY_C), ks=(1,), device=DEV)
    assert res == dict(top1=100.0 * counts[4]['top1'] / 4, top5=100.0 * counts[4]['top5'] / 4, r1=100.0 * r1[1] / 4, count=4)
    assert total == 4 and not mon.encoder.training and trainer.model.training
    sd = trainer.state_dict(epoch=1)
    assert mon.evaluate({'state_dict': sd['state_dict']}) == res         # a checkpoint dict works like the trainer
    f, cl = E.features_of(enc, bank, 1, T_CLIP, DEV)
    assert f.is_cuda and cl.is_cuda and torch.equal(f, g) and cl.tolist() == BANK_C


def test_staged_batches_give_the_features_of_their_views(pkg, tiny):
    E, inp = pkg.lib.evaluation, pkg.engine.input
    trainer = _trainer(pkg, tiny)
    enc = E.load_encoder(trainer.state_dict(), 'R2P1D10T', T_CLIP).to(DEV)
    B, crops, clips, Hs, Ws = 2, 3, 2, 56, 72
    frames = np.random.RandomState(51).randint(0, 256, size=(B, clips * T_CLIP, Hs, Ws, 3)).astype(np.uint8)
    stage = inp.ActionInputStage(B, clips * T_CLIP, (Hs, Ws), SIZE, DEV, mode='test', scale_size=(52, 64), test_crops=crops,
                                 test_clips=clips)
    views = stage.views
    assert views == crops * clips
    x = stage.prepare(stage.stage(frames), torch.empty(stage.out_shape(), device=DEV))           # (B * views, 3, T, S, S)
    data = x.reshape(B, views, 3, T_CLIP, SIZE, SIZE).permute(0, 2, 1, 3, 4, 5).reshape(B, 3, views * T_CLIP, SIZE, SIZE).contiguous()
    want = E.extract_feature_single(enc, data, crops, T_CLIP)
    buf = torch.empty(stage.out_shape(), device=DEV)
    got = E.extract_feature_single(enc, stage.stage(frames), crops, T_CLIP, views_buf=buf)
    assert got.shape == (B, enc.feature_dim) and torch.equal(got, want) and torch.equal(buf, x)
    assert torch.equal(E.extract_feature_single(enc, stage.stage(frames), crops, T_CLIP), want)   # a buffer of its own
    f, cl = E.features_of(enc, ((stage.stage(frames), torch.tensor([4, 1])) for _ in range(3)), crops, T_CLIP, DEV)
    assert torch.equal(f, torch.cat([want] * 3)) and cl.tolist() == [4, 1] * 3
    with pytest.raises(ValueError):
        E.extract_feature_single(enc, stage.stage(frames), crops, T_CLIP + 1)
    with pytest.raises(ValueError):
        E.extract_feature_single(enc, stage.stage(frames), crops, T_CLIP, views_buf=buf[:1])


def test_monitor_takes_staged_batches(pkg, tiny, tmp_path):
    E, inp = pkg.lib.evaluation, pkg.engine.input
    trainer = _trainer(pkg, tiny)
    rs = np.random.RandomState(52)
    frames = [rs.randint(0, 256, size=(2, T_CLIP, 56, 64, 3)).astype(np.uint8) for _ in range(5)]
    stage = inp.ActionInputStage(2, T_CLIP, (56, 64), SIZE, DEV, mode='test', scale_size=(52, 60), test_crops=1, test_clips=1)
    labels = [torch.tensor(BANK_C[i:i + 2]) for i in (0, 2, 4)] + [torch.tensor(QUERY_C[i:i + 2]) for i in (0, 2)]
    bank = lambda: ((stage.stage(frames[i]), labels[i]) for i in range(3))                      # noqa: E731
    query = lambda: ((stage.stage(frames[i]), labels[i]) for i in (3, 4))                       # noqa: E731
    res = E.KNNMonitor(trainer.cfg, bank, query, NUM_CLASS, k=4, device=DEV).evaluate(trainer)
    views = [stage.prepare(stage.stage(f), torch.empty(stage.out_shape(), device=DEV)) for f in frames]
    tens = [(v, l) for v, l in zip(views, labels)]
    assert E.KNNMonitor(trainer.cfg, tens[:3], tens[3:], NUM_CLASS, k=4, device=DEV).evaluate(trainer) == res
    assert res['count'] == 4
    # extract_features passes staged batches through as well; its files are what they were
    enc = E.load_encoder(trainer.state_dict(), 'R2P1D10T', T_CLIP).to(DEV)
    a = E.extract_features(enc, bank(), 1, T_CLIP, str(tmp_path), 'staged', device=DEV)
    b = E.extract_features(enc, tens[:3], 1, T_CLIP, str(tmp_path), 'tensor', device=DEV)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].dtype == np.float32


def test_monitor_leaves_the_training_run_alone(pkg, tiny):
    """Two identically seeded runs, one with a monitor call between the steps: the same bits after the second step."""
    E = pkg.lib.evaluation
    bank, query = _batches(31, BANK_C), _batches(32, QUERY_C)
    runs = []
    for watched in (False, True):
        trainer = _trainer(pkg, tiny, seed=9)
        mon = E.KNNMonitor(trainer.cfg, bank, query, NUM_CLASS, k=4, device=DEV) if watched else None
        losses = [trainer.train_step(_step_input(3))['loss'].clone()]
        if watched:
            res = mon.evaluate(trainer)
            assert res['count'] == 4 and trainer.model.training
        losses.append(trainer.train_step(_step_input(4))['loss'].clone())
        torch.cuda.synchronize()
        state = {k: v.detach().clone() for k, v in trainer.model.state_dict().items()}
        state.update({'ema.' + k: v.detach().clone() for k, v in trainer.model_ema.state_dict().items()})
        state['queue'] = trainer.contrast.memory.detach().clone()
        runs.append((losses, state))
    (la, sa), (lb, sb) = runs
    assert all(torch.equal(x, y) for x, y in zip(la, lb)) and bool(torch.isfinite(la[1]).all())
    assert sa.keys() == sb.keys() and any('running_mean' in k for k in sa) and len(sa) > 100
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
