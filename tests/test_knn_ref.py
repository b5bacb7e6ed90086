"""CPU tests of the k-NN vote's specification (tests/knn_ref.py), of the preconditions the GPU tests rest on, and of the
host layers that need no device: ops.knn_vote's argument checks, knn_classify's counting, tools/knn_eval.py."""
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_cases as kc                   # noqa: E402
import knn_ref as kr                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plain_vote(idx, dist, g_label, C, kvote, q_label, self_base, weight):
    """An independent statement with dictionaries and sorted(): -> (score dicts, pred, rank)."""
    scores, pred, rank = [], [], []
    for i in range(len(idx)):
        tally, used = {}, 0
        for j in range(len(idx[i])):
            gi = int(idx[i][j])
            if used == kvote or gi < 0 or gi >= len(g_label) or dist[i][j] != dist[i][j]:
                continue
            if self_base >= 0 and gi == self_base + i:
                continue
            c = int(g_label[gi])
            if c < 0 or c >= C:
                continue
            tally[c] = tally.get(c, 0.0) + weight(float(dist[i][j]))
            used += 1
        scores.append(tally)
        if not used:
            pred.append(-1)
            rank.append(C)
            continue
        t = int(q_label[i])
        order = sorted(range(C), key=lambda c: (-tally.get(c, 0.0), c))
        pred.append(order[0])
        rank.append(sum(1 for c in order[:order.index(t)] if c != t))
    return scores, np.array(pred), np.array(rank)


def all_small_cases():
    out = [(n, kc.content_case()) for n in ('content',)] + [('distinct', kc.distinct_classes_case()), ('loo', kc.loo_case())]
    out += [('float%r' % (spec,), kc.float_case(*spec)) for spec in kc.FLOAT_CASES if spec[2] <= 101]
    return out


@pytest.mark.parametrize('weighting', kr.WEIGHTINGS)
def test_specification_against_a_plain_loop(weighting):
    T = 0.07
    weight = (lambda d: 1.0) if weighting == 'uniform' else (lambda d: float(np.exp(-(np.float64(np.float32(d)) * np.float64(kr.inv_T32(T))))))
    for name, c in all_small_cases():
        k = c['idx'].shape[1]
        for kv in kc.kvotes(k):
            sb = c.get('self_base', -1)
            s, p, r = kr.vote(c['idx'], c['dist'], c['g_label'], c['C'], kv, c['q_label'], sb, weighting, T)
            ps, pp, pr = plain_vote(c['idx'], c['dist'], c['g_label'], c['C'], kv, c['q_label'], sb, weight)
            assert np.array_equal(p, pp) and np.array_equal(r, pr), (name, kv)
            for i, tally in enumerate(ps):
                dense = np.zeros(c['C'])
                for cls, v in tally.items():
                    dense[cls] = v
                assert np.allclose(s[i], dense, rtol=1e-12, atol=0), (name, kv, i)
            assert np.array_equal(r == 0, p == c['q_label']), (name, kv)          # rank == 0 iff pred == label


def test_exp_weight_ranks_like_instdisc():
    """exp(-dist / T) = exp(sim / T) / exp(1 / T) for dist = 1 - sim: the same prediction and rank, in fp64."""
    for spec in kc.FLOAT_CASES:
        if spec[2] > 101:
            continue
        c = kc.float_case(*spec)
        sim = 1.0 - c['dist'].astype(np.float64)
        for T in (0.07, 1.0):            # (exp(1 / 0.05) scales the gaps of T = 0.05 too, but 0.07 is the protocol's value)
            _, p, r = kr.vote(c['idx'], c['dist'], c['g_label'], c['C'], None, c['q_label'], weighting='exp', T=T)
            _, pp, pr = plain_vote(c['idx'], c['dist'], c['g_label'], c['C'], c['idx'].shape[1], c['q_label'], -1,
                                   lambda d, T=T: float(np.exp((1.0 - np.float64(np.float32(d))) / T)))
            assert np.array_equal(p, pp) and np.array_equal(r, pr), (spec, T)
        assert sim.max() <= 1.0


def test_rules_on_the_content_case():
    c = kc.content_case()
    what = c['what']
    s, p, r = kr.vote(c['idx'], c['dist'], c['g_label'], c['C'], None, c['q_label'], weighting='uniform', order32=True)
    assert s.dtype == np.float32 and p.dtype == np.int32 and r.dtype == np.int32
    row = {w: i for i, w in enumerate(what)}
    i = row['all neighbours in one class']
    assert p[i] == 0 and r[i] == 0 and s[i, 0] == 8 and s[i].sum() == 8
    i = row['target class absent, unvoted classes 0 and 4 below it']
    assert (s[i, 1], s[i, 2], s[i, 3]) == (3, 3, 2) and p[i] == 1 and r[i] == 3 + 2
    i = row['target score 0 far up: every unvoted class below counts']
    assert r[i] == 3 + 97
    i = row['target score 0 at class 0: only the voted classes come first']
    assert r[i] == 3
    i = row['tail slots']
    assert s[i].sum() == 2 and s[i, 5] == 2 and p[i] == 5 and r[i] == 0
    i = row['idx >= ng and negative idx']
    assert s[i].sum() == 3 and (s[i, 3], s[i, 4]) == (2, 1) and p[i] == 3 and r[i] == 1
    i = row['labels outside [0, C): only 67 (class 100), 4 and 11 vote']
    assert s[i].sum() == 3 and s[i, 100] == 1 and s[i, 4] == 2 and p[i] == 4 and r[i] == 1
    i = row['NaN slots skipped, +inf slots vote']
    assert s[i].sum() == 6 and (s[i, 6], s[i, 5]) == (5, 1) and p[i] == 6     # rows 13 and 5 (NaN) are out, the +inf ones in
    i = row['no valid slot']
    assert p[i] == -1 and r[i] == c['C'] and not s[i].any()
    i = row['no valid slot: labels and indices out of range']
    assert p[i] == -1 and r[i] == c['C'] and not s[i].any()
    i = row['classes 3 and 1 tie at three voters: the lower class comes first']
    assert s[i, 1] == s[i, 3] == 3 and p[i] == 1 and r[i] == 2      # classes 1 and 3 before class 0 (two voters)
    i = row['the same tie met in the other order']
    assert p[i] == 1 and r[i] == 1
    # exp weights: a +inf distance votes with weight 0, dist = 0 with weight 1
    s, p, r = kr.vote(c['idx'], c['dist'], c['g_label'], c['C'], None, c['q_label'], weighting='exp', T=0.07, order32=True)
    i = row['dist 0 and 2']
    assert (s[i, 2], s[i, 3]) == (2.0, 1.0 + np.float32(np.exp(-np.float64(np.float32(2.0) * kr.inv_T32(0.07)))))
    # kvote: the first kvote VALID slots vote
    s, p, r = kr.vote(c['idx'], c['dist'], c['g_label'], c['C'], 2, c['q_label'], weighting='uniform')
    i = row['idx >= ng and negative idx']
    assert (s[i, 3], s[i, 4]) == (1, 1) and s[i].sum() == 2         # gallery rows 3 and 4, past five invalid slots
    i = row['NaN slots skipped, +inf slots vote']
    assert s[i].sum() == 2


def test_leave_one_out_and_kvote_promotion():
    c = kc.loo_case()
    base = c['self_base']
    assert c['idx'][0, 0] == base and c['idx'][1, 2] == base + 1 and c['idx'][3, 5] == base + 3 and base + 2 not in c['idx'][2]
    s, p, r = kr.vote(c['idx'], c['dist'], c['g_label'], c['C'], 3, c['q_label'], base, 'uniform')
    gl = c['g_label']
    for i, slots in enumerate(([1, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2])):
        want = np.zeros(c['C'])
        for j in slots:
            want[gl[c['idx'][i, j]]] += 1
        assert np.array_equal(s[i], want), i
    s_all = kr.vote(c['idx'], c['dist'], c['g_label'], c['C'], 3, c['q_label'], -1, 'uniform')[0]
    assert not np.array_equal(s_all[0], s[0]) and not np.array_equal(s_all[1], s[1]) and np.array_equal(s_all[2:], s[2:])


def test_preconditions_of_the_gpu_float_cases():
    """Every nq / k / C of the issue's lists occurs, and for every kvote and T the fp64 scores of every row keep the relative
    gap GAP between the best two classes and around the target: fp32 sums (error < 2e-5) cannot reorder them."""
    assert {s[0] for s in kc.FLOAT_CASES} == set(kc.NQS) and {s[1] for s in kc.FLOAT_CASES} == set(kc.KS)
    assert {s[2] for s in kc.FLOAT_CASES} == set(kc.CS)
    for spec in kc.FLOAT_CASES:
        c = kc.float_case(*spec)
        assert (c['dist'][:, 1:] >= c['dist'][:, :-1]).all() and c['dist'][np.isfinite(c['dist'])].max() <= 2.0
        for kv in kc.kvotes(spec[1]):
            for T in kc.TS:
                s, p, r = kr.vote(c['idx'], c['dist'], c['g_label'], c['C'], kv, c['q_label'], weighting='exp', T=T)
                assert kr.gaps(s, c['q_label']).min() >= kc.GAP, (spec, kv, T)
                assert (p >= 0).all()


def test_gaps_sees_ties():
    s = np.array([[3.0, 3.0, 1.0], [3.0, 2.0, 2.0], [3.0, 2.0, 0.0], [0.0, 2.0, 0.0]])
    g = kr.gaps(s, np.array([2, 1, 2, 0]))
    assert g[0] == 0 and g[1] == 0 and g[2] == pytest.approx(1 / 3) and g[3] == 1.0


# ----------------------------------------------------------------------------- host layers
def fake_ops(monkeypatch, pkg):
    """retrieval_topk / knn_vote of engine.ops replaced by the numpy specifications, on host tensors."""
    import retrieval_ref as rr
    ops = pkg.engine.ops

    def topk(q, g, k, metric='cosine', q_label=None, g_label=None, slabs=0):
        idx, dist, hit = rr.topk(q.numpy(), g.numpy(), k, metric, None if q_label is None else q_label.numpy(),
                                 None if g_label is None else g_label.numpy())
        return torch.from_numpy(idx), torch.from_numpy(dist), None if hit is None else torch.from_numpy(hit)

    def vote(idx, dist, g_label, num_class, kvote=None, q_label=None, self_base=-1, weighting='exp', T=0.07, want_scores=False):
        s, p, r = kr.vote(idx.numpy(), dist.numpy(), g_label.numpy(), num_class, kvote, None if q_label is None else q_label.numpy(),
                          self_base, weighting, T)
        return torch.from_numpy(p), None if r is None else torch.from_numpy(r), torch.from_numpy(s) if want_scores else None
    monkeypatch.setattr(ops, 'retrieval_topk', topk)
    monkeypatch.setattr(ops, 'knn_vote', vote)


def test_knn_classify_counts_a_hand_made_case(pkg, monkeypatch):
    fake_ops(monkeypatch, pkg)
    K = pkg.lib.evaluation.knn
    cpu = torch.device('cpu')
    # bank on the plane: three rows of class 0 around angle 0, two of class 1 around 90 degrees, one of class 6 at 180 degrees
    ang = np.deg2rad([0.0, 5.0, -5.0, 90.0, 80.0, 180.0])
    train = np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)
    train_c = np.array([0, 0, 0, 1, 1, 6])
    qang = np.deg2rad([2.0, 85.0, 60.0, 170.0, 44.0])
    val = np.stack([np.cos(qang), np.sin(qang)], 1).astype(np.float32)
    # the third: nearest are the two of class 1; the fourth: its class has no bank row and sits behind 6, 0, 1, 2, 3, 4 or
    # 1, 6, 0, 2, 3, 4; the fifth: nearest is 80 degrees (class 1), then 5 and 0 degrees (class 0)
    val_c = np.array([0, 1, 0, 5, 0])
    correct, total = K.knn_classify(train, train_c, val, val_c, ks=(1, 3, 6), T=0.07, weighting='uniform', device=cpu)
    assert total == 5 and list(correct) == [1, 3, 6]
    assert correct[1] == {'top1': 2, 'top5': 4}    # rows 1, 2 right; rows 3, 5 vote class 1, their own at rank 1; row 4 at rank 5
    assert correct[3] == {'top1': 3, 'top5': 4}    # row 5 now has two votes for class 0
    assert correct[6] == {'top1': 3, 'top5': 4}    # all six vote: class 0 wins everywhere (rows 1, 3, 5), class 1 has rank 1
    assert K.knn_classify(train, train_c, val, val_c, num_class=7, ks=(6,), weighting='uniform', device=cpu)[0] == {6: correct[6]}
    pred = K.knn_predict(torch.from_numpy(train), train_c, torch.from_numpy(val), 7, k=3, weighting='uniform', device=cpu)
    assert pred.tolist() == [0, 1, 1, 1, 0]
    loo, n = K.knn_classify_loo(train, train_c, ks=(1, 2), weighting='uniform', chunk=4, device=cpu)
    assert n == 6 and loo[1] == {'top1': 5, 'top5': 5} and K.knn_classify_loo(train, train_c, ks=(1, 2), weighting='uniform',
                                                                                 chunk=1, device=cpu)[0] == loo
    for bad in (dict(ks=(0,)), dict(ks=(65,)), dict(ks=()), dict(num_class=6), dict(weighting='gauss')):
        with pytest.raises(ValueError):
            K.knn_classify(train, train_c, val, val_c, device=cpu, **bad)
    with pytest.raises(ValueError):
        K.knn_classify(train, np.array([0, 0, 0, 1, 1, -1]), val, val_c, device=cpu)
    with pytest.raises(ValueError):
        K.knn_classify(train, train_c[:5], val, val_c, device=cpu)
    with pytest.raises(ValueError):
        K.knn_classify(train, train_c, val, val_c[:4], device=cpu)
    with pytest.raises(ValueError):
        K.knn_classify_loo(train, train_c, ks=(64,), device=cpu)
    with pytest.raises(ValueError):
        K.knn_predict(train, train_c, val, 7, metric='euclidean', device=cpu)                  # exp weights need cosine distances
    with pytest.raises(ValueError):
        K.knn_predict(train, train_c, val, 7, k=65, device=cpu)


def test_ops_knn_vote_refuses_before_it_looks_for_a_device(pkg):
    ops = pkg.engine.ops
    idx = torch.zeros(3, 4, dtype=torch.int32)
    dist = torch.zeros(3, 4)
    gl, ql = torch.zeros(9, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    for args, kw in [((idx, dist, gl, 5), dict(kvote=0)), ((idx, dist, gl, 5), dict(kvote=5)), ((idx, dist, gl, 0), {}),
                     ((idx, dist, gl, 5), dict(weighting='gauss')), ((idx, dist, gl, 5), dict(T=0.0)),
                     ((idx, dist, gl, 5), dict(T=-1.0)), ((idx, dist, gl, 5), dict(T=float('nan'))),
                     ((idx, dist, gl, 5), dict(T=1e-40)),                                       # 1 / T overflows fp32
                     ((idx.long(), dist, gl, 5), {}), ((idx, dist.double(), gl, 5), {}), ((idx, dist[:, :3], gl, 5), {}),
                     ((idx[0], dist[0], gl, 5), {}), ((idx, dist, gl.int(), 5), {}), ((idx, dist, gl[None], 5), {}),
                     ((idx, dist, gl, 5), dict(q_label=ql[:2])), ((idx, dist, gl, 5), dict(q_label=ql.int())),
                     ((torch.zeros(3, 65, dtype=torch.int32), torch.zeros(3, 65), gl, 5), {}),
                     ((torch.zeros(3, 0, dtype=torch.int32), torch.zeros(3, 0), gl, 5), {}),
                     ((idx, dist, gl, 2 ** 30), dict(want_scores=True))]:
        with pytest.raises(ValueError):
            ops.knn_vote(*args, **kw)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.knn_vote(idx, dist, gl, 5, q_label=ql)


def test_abi_and_build_lists_name_the_kernel(pkg):
    assert 'gca_knn_vote' in pkg._hip.SIGNATURES and len(pkg._hip.SIGNATURES['gca_knn_vote'][1]) == 16
    entry = importlib.import_module('__graft_entry__')
    assert 'knn' in entry.SOURCES
    sh = open(os.path.join(ROOT, 'build_hip.sh')).read()
    assert ' knn;' in sh and 'knn.o' in sh


def test_knn_eval_parser_and_json(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    tool = importlib.import_module('knn_eval')
    base = ['--train_feature_path', 'a', '--train_classes_path', 'b', '--val_feature_path', 'c', '--val_classes_path', 'd']
    a = tool.get_parser().parse_args(base)
    assert tool.ks_of(a) == (1, 5, 10, 20) and a.temperature == 0.07 and a.weighting == 'exp' and a.num_class is None
    a = tool.get_parser().parse_args(base + ['--k', '20', '--k', '5', '--temperature', '0.1', '--weighting', 'uniform',
                                             '--num_class', '101', '--save_scores', str(tmp_path)])
    assert tool.ks_of(a) == (20, 5) and a.temperature == 0.1 and a.weighting == 'uniform' and a.num_class == 101
    with pytest.raises(SystemExit):
        tool.get_parser().parse_args(base + ['--weighting', 'gauss'])
    with pytest.raises(SystemExit):
        tool.get_parser().parse_args(base[2:])
    correct = {20: {'top1': 7, 'top5': np.int64(9)}, 5: {'top1': 6, 'top5': 9}}
    rep = json.loads(json.dumps(tool.report(correct, 10, 0.1, 'uniform')))
    assert rep == {'total': 10, 'temperature': 0.1, 'weighting': 'uniform',
                   'k': {'20': {'top1': 7, 'top5': 9}, '5': {'top1': 6, 'top5': 9}}}
    assert tool.lines(correct, 10)[0] == 'k = 20: top-1 correct = 7, top-5 correct = 9, total = 10, top-1 = 0.700, top-5 = 0.900'
