"""CPU checks of the retrieval feature: the numpy specification (tests/retrieval_ref.py) against the sklearn functions the
reference calls, the preconditions under which tests/test_gpu_retrieval.py may demand the specification's bits from the
kernel, the recall arithmetic and file formats of lib/evaluation/retrieval.py, tools/retrieval_eval.py with the search
replaced by the specification, and the argument checks of the C entry (they return before any launch)."""
import importlib.util
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retrieval_cases as cases          # noqa: E402
import retrieval_ref as ref              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ----------------------------------------------------------------------------- specification
@pytest.mark.parametrize('metric', ref.METRICS)
def test_spec_equals_sklearn(metric):
    """Distances to 1e-12 on fp64 inputs, and the same top-k as np.argsort(kind='stable') of sklearn's own matrix."""
    pairwise = pytest.importorskip('sklearn.metrics.pairwise')
    rs = np.random.RandomState(3)
    q, g = rs.standard_normal((23, 16)), rs.standard_normal((211, 16))
    g[17] = 0.0                                                    # sklearn's normalize leaves an all-zero row alone
    q[5] = 0.0
    theirs = (pairwise.cosine_distances if metric == 'cosine' else pairwise.euclidean_distances)(q, g)
    key = ref.keys64(q, g, metric)
    assert np.abs(ref.dist_of_key(key, metric) - theirs).max() <= 1e-12
    idx, dist, _ = ref.topk(q, g, 50, metric, dtype=np.float64)
    want = np.argsort(theirs, axis=1, kind='stable')[:, :50]
    zero_row = np.zeros(23, bool)
    zero_row[5] = metric == 'cosine'      # every distance of a zero query is exactly 1 here, clipped 1 +- ulp there: all ties
    assert np.array_equal(idx[~zero_row], want[~zero_row])
    assert np.abs(dist - np.take_along_axis(theirs, want, 1))[~zero_row].max() <= 1e-12
    assert np.array_equal(idx[5], np.arange(50)) or metric != 'cosine'


def test_spec_order_is_the_k_smallest_words():
    """(key, index) order, NaN after +inf, -0 == +0: argsort(kind='stable') and 'the k smallest packed words' agree."""
    key = np.array([[0.0, -0.0, np.nan, np.inf, -np.inf, 1.5, 1.5, -2.0, -np.nan, 1e-40, -1e-40, 0.0]], dtype=F32)
    words = ref.order_words(key)
    by_words = np.argsort(words, axis=1)
    canon = key + F32(0)
    by_sort = np.argsort(canon, axis=1, kind='stable')
    assert np.array_equal(by_words[:, :10], by_sort[:, :10])       # the two NaNs come last, in index order
    assert list(by_words[0, 10:]) == [2, 8] and list(by_words[0, :3]) == [4, 7, 10]
    assert len(np.unique(words)) == words.size
    assert words.max() < np.uint64(0xFFFFFFFFFFFFFFFF)              # the tail word is never a candidate


def test_spec_tails_labels_and_zero_rows():
    q = np.array([[1, 0], [0, 0], [0, 2]], dtype=F32)
    g = np.array([[2, 0], [0, 0], [0, 1], [1, 1]], dtype=F32)
    idx, dist, hit = ref.topk(q, g, 6, 'cosine', np.array([7, 7, 9]), np.array([1, 7, 9, 7]))
    assert idx.shape == (3, 6) and (idx[:, 4:] == -1).all() and np.isinf(dist[:, 4:]).all()
    assert list(idx[0, :4]) == [0, 3, 1, 2] and list(idx[1, :4]) == [0, 1, 2, 3]      # zero rows: distance exactly 1
    assert dist[0, 0] == 0 and dist[0, 2] == 1 and (dist[1, :4] == 1).all()
    assert list(hit) == [2, 2, 1]
    assert list(ref.topk(q, g, 2, 'euclidean', np.array([5, 5, 5]), np.array([1, 2, 3, 4]))[2]) == [3, 3, 3]
    e = ref.topk(q, np.zeros((0, 2), F32), 3, 'euclidean', np.array([1, 2, 3]), np.zeros(0, np.int64))
    assert (e[0] == -1).all() and np.isinf(e[1]).all() and list(e[2]) == [4, 4, 4]
    gn = g.copy()
    gn[1] = np.nan
    idx, dist, _ = ref.topk(q, gn, 4, 'euclidean')
    assert (idx[:, 3] == 1).all() and np.isnan(dist[:, 3]).all() and not np.isnan(dist[:, :3]).any()


# ----------------------------------------------------------------------------- preconditions of the exact GPU cases
def chain32(q, g, metric):
    """The kernel's arithmetic after the dot products, one fp32 rounding per operation.  The dot products and squared
    norms themselves are taken exact: the caller asserts sum |a b| < 2^24 on integer-valued operands, under which every
    partial sum of every summation order is an integer below 2^24."""
    q64, g64 = q.astype(np.float64), g.astype(np.float64)
    s = (q64 @ g64.T).astype(F32)
    n2q, n2g = (q64 * q64).sum(1).astype(F32), (g64 * g64).sum(1).astype(F32)
    with np.errstate(all='ignore'):
        if metric == 'cosine':
            rq = np.where(n2q == 0, F32(0), F32(1) / np.sqrt(n2q)).astype(F32)
            rg = np.where(n2g == 0, F32(0), F32(1) / np.sqrt(n2g)).astype(F32)
            return F32(1) - (s * rq[:, None]) * rg[None, :]
        d2 = (n2q[:, None] + n2g[None, :]) - F32(2) * s
        return np.where(d2 < 0, F32(0), d2)


def assert_exact(q, g, metric, rows=None):
    """Every partial sum is an integer below 2^24 and every later operation is exact, on gallery rows `rows` (all)."""
    g = g if rows is None else g[rows]
    assert np.array_equal(q, np.round(q)) and np.array_equal(g, np.round(g))
    assert (np.abs(q).astype(np.float64) @ np.abs(g).astype(np.float64).T).max() < 2 ** 24
    assert max((q.astype(np.float64) ** 2).sum(1).max(), (g.astype(np.float64) ** 2).sum(1).max()) < 2 ** 24
    key32, key64 = chain32(q, g, metric), ref.keys64(q, g, metric)
    assert key32.dtype == F32 and np.array_equal(key32.astype(np.float64), key64)
    if metric == 'cosine':
        n2 = np.concatenate([(q.astype(np.float64) ** 2).sum(1), (g.astype(np.float64) ** 2).sum(1)])
        r = F32(1) / np.sqrt(n2[n2 > 0].astype(F32))
        assert np.array_equal(r.astype(np.float64) ** 2 * n2[n2 > 0], np.ones(len(r)))       # 1 / sqrt(n2) is exact
        unit = 2.0 ** -24
        assert np.array_equal(key64 / unit, np.round(key64 / unit)) and np.abs(key64 / unit).max() <= 2 ** 25
    else:
        assert key64.max() < 2 ** 24


def has_tie_across_slabs(q, g, k, metric, slabs):
    """Some query's result holds two rows of equal key that lie in different slabs."""
    idx, dist, _ = ref.topk(q, g, k, metric)
    where = cases.slab_of(np.maximum(idx, 0), len(q), len(g), slabs)
    for i in range(len(q)):
        for d in np.unique(dist[i][idx[i] >= 0]):
            if len(set(where[i][(dist[i] == d) & (idx[i] >= 0)])) > 1:
                return True
    return False


def test_slab_arithmetic_matches_the_library(pkg):
    """cases.slab_count restates make_plan: the workspace size is norms + nq * S * k * 8."""
    ws = pkg._hip.lib.gca_retrieval_ws_bytes
    for nq, ng, slabs in [(33, 700, 0), (33, 700, 3), (33, 700, 1), (70, 1000, 0), (5, 4096, 0), (5, 4096, 3), (130, 2049, 0),
                          (3783, 9537, 0), (4096, 240000, 0), (1, 1, 0), (5, 300, 3), (20000, 240000, 0), (33, 700, 100)]:
        S, per = cases.slab_count(nq, ng, slabs)
        assert ws(nq, ng, 64, 50, slabs) == -(-(nq + ng) * 4 // 16) * 16 + nq * S * 50 * 8, (nq, ng, slabs)
        assert S * per >= ng > (S - 1) * per
    assert cases.slab_count(33, 700, 3) == (3, 256) and cases.slab_count(33, 700, 0) == (6, 128)
    assert cases.slab_count(3783, 9537, 0)[0] == 9 and cases.slab_count(4096, 240000, 0)[0] == 8


@pytest.mark.parametrize('name', ['cosine', 'euclidean', 'all_equal'])
def test_exact_cases_are_exact_and_tied(name):
    q, g = {'cosine': cases.cosine_case, 'euclidean': cases.euclidean_case, 'all_equal': cases.all_equal_case}[name]()
    metrics = {'cosine': ['cosine'], 'euclidean': ['euclidean'], 'all_equal': list(ref.METRICS)}[name]
    for metric in metrics:
        assert_exact(q, g, metric)
        for k in ((1, 50, 64) if name == 'cosine' else (64,) if name == 'all_equal' else (50,)):
            idx, dist, _ = ref.topk(q, g, k, metric)
            if k > 1:
                assert (dist[:, 1:] == dist[:, :-1]).any()                   # ties inside a result
                for slabs in (3, 0):
                    assert cases.slab_count(len(q), len(g), slabs)[0] > 1
                    if name == 'all_equal':      # every row of every slab ties; the result is the k lowest indices, all of slab 0
                        assert (ref.keys64(q, g, metric) == ref.keys64(q, g, metric)[:, :1]).all()
                    else:
                        assert has_tie_across_slabs(q, g, k, metric, slabs), (metric, k, slabs)
    if name == 'cosine':                 # rows equal to a query (distance 0) and duplicated rows
        idx, dist, _ = ref.topk(q, g, 50, 'cosine')
        assert list(idx[0, :4]) == [100, 130, 300, 600] and (dist[0, :4] == 0).all()
        assert np.array_equal(g[400], g[20]) and np.array_equal(g[650], g[20])
    if name == 'all_equal':
        assert np.array_equal(ref.topk(q, g, 64, 'cosine')[0], np.tile(np.arange(64, dtype=np.int32), (5, 1)))


@pytest.mark.parametrize('descending', [True, False])
def test_ramp_cases_are_exact_where_it_matters(descending):
    """Rows |v| < 4096 (v^2 < 2^24) are exact.  The 105 longer rows are not (v^2 needs up to 25 bits): they are the farthest
    rows, and their keys -- rounded the way the kernel rounds them -- stay above every key of a result, so they order the
    kernel's intermediate lists only and the result is still the specification's, bit for bit."""
    q, g = cases.ramp_case(descending)
    small = np.abs(g[:, 0]) < 4096
    assert small.sum() == 4096 - 105
    assert_exact(q, g, 'euclidean', rows=small)
    idx, dist, _ = ref.topk(q, g, 64, 'euclidean')
    assert small[idx].all()
    kth = (dist[:, -1].astype(np.float64)) ** 2
    assert (chain32(q, g[~small], 'euclidean').min(1) > kth).all()
    assert (dist[:, 1:] > dist[:, :-1]).all()                                # no ties: a strict ramp
    want = np.arange(4095, 4031, -1) if descending else np.arange(64)        # the nearest rows are the 64 shortest
    assert np.array_equal(idx[0], want.astype(np.int32))


@pytest.mark.parametrize('metric', ref.METRICS)
def test_shape_cases_are_exact(metric):
    for nq, ng, D in [(1, 1, 1), (31, 33, 3), (33, 31, 6), (130, 2049, 65), (33, 2049, 130), (33, 700, 1024)]:
        q, g = cases.shape_case(nq, ng, D, metric)
        assert q.shape == (nq, D) and g.shape == (ng, D)
        assert_exact(q, g, metric)


# ----------------------------------------------------------------------------- recall arithmetic and file formats
def test_recall_counts_from_first_hit(pkg):
    R = pkg.lib.evaluation.retrieval
    first_hit = np.array([1, 1, 2, 5, 6, 10, 11, 20, 50, 51, 51], dtype=np.int32)       # 51 = no hit within k = 50
    assert R.recall_counts(first_hit) == {1: 2, 5: 4, 10: 6, 20: 8, 50: 9}
    assert R.recall_counts(first_hit, ks=(3,)) == {3: 3}
    assert pkg.lib.evaluation.topk_retrieval is R.topk_retrieval


def spec_search(val_features, val_classes, train_features, train_classes, k, metric, norm=False, device=None):
    """lib.evaluation.retrieval.search_first_hit on the specification instead of the device."""
    q, g = np.asarray(val_features, F32), np.asarray(train_features, F32)
    if norm:
        q = torch.nn.functional.normalize(torch.from_numpy(q), dim=1).numpy()
        g = torch.nn.functional.normalize(torch.from_numpy(g), dim=1).numpy()
    return ref.topk(q, g, k, metric, np.asarray(val_classes), np.asarray(train_classes))[2]


def reference_counts(train_f, train_c, val_f, val_c, ks):
    """The counting loop of the reference (tools/video_retrieval.py:189-197) on a stable argsort of the spec's keys."""
    order = np.argsort(ref.keys64(val_f, train_f, 'cosine').astype(F32), axis=1, kind='stable')
    return {k: int(sum(c in train_c[o[:k]] for o, c in zip(order, val_c))) for k in ks}


def test_topk_retrieval_counts_like_the_reference(pkg, monkeypatch):
    R = pkg.lib.evaluation.retrieval
    monkeypatch.setattr(R, 'search_first_hit', spec_search)
    rs = np.random.RandomState(5)
    train_f, val_f = rs.standard_normal((300, 12)).astype(F32), rs.standard_normal((40, 12)).astype(F32)
    train_c, val_c = rs.randint(0, 30, 300), rs.randint(0, 30, 40)
    correct, total = R.topk_retrieval(train_f, train_c, val_f, val_c)
    assert total == 40 and list(correct) == [1, 5, 10, 20, 50]
    assert correct == reference_counts(train_f, train_c, val_f, val_c, (1, 5, 10, 20, 50))
    assert 0 < correct[1] < correct[50] <= 40
    with pytest.raises(ValueError):
        R.topk_retrieval(train_f, train_c, val_f, val_c, ks=(1, 65))
    with pytest.raises(ValueError):
        R.topk_retrieval(train_f, train_c[:-1], val_f, val_c)


def test_extract_features_writes_the_reference_pickles(pkg, monkeypatch, tmp_path):
    R = pkg.lib.evaluation.retrieval
    monkeypatch.setattr(R, 'extract_feature_single',
                        lambda model, data, crops, T, softmax=False: data.reshape(data.shape[0], -1)[:, :4] * (2.0 if softmax else 1.0))
    batches = [(torch.arange(2 * 3 * 4 * 2 * 2, dtype=torch.float32).reshape(2, 3, 4, 2, 2), torch.tensor([4, 9])),
               (torch.ones(1, 3, 4, 2, 2), torch.tensor([1]))]
    feats, classes = R.extract_features(None, batches, 1, 4, str(tmp_path), 'val', device=torch.device('cpu'))
    fpath, cpath = tmp_path / 'val_features.pkl', tmp_path / 'val_classes.pkl'
    assert fpath.exists() and cpath.exists()
    with open(fpath, 'rb') as fh:
        f2 = pickle.load(fh)
    with open(cpath, 'rb') as fh:
        c2 = pickle.load(fh)
    assert isinstance(f2, np.ndarray) and f2.dtype == F32 and f2.shape == (3, 4) and np.array_equal(f2, feats)
    assert isinstance(c2, np.ndarray) and c2.dtype == np.int64 and list(c2) == [4, 9, 1] and np.array_equal(c2, classes)
    assert list(f2[1]) == [48, 49, 50, 51] and list(f2[2]) == [1, 1, 1, 1]


def test_split_views_follows_the_reference_layout(pkg):
    """dim 2 = clips x crops x T; view (clip c, crop i) is frames [(c * crops + i) * T, +T) (tools/video_retrieval.py:105-109)."""
    R = pkg.lib.evaluation.retrieval
    B, crops, clips, T = 2, 3, 2, 4
    data = torch.arange(B * 3 * clips * crops * T * 2 * 2, dtype=torch.float32).reshape(B, 3, clips * crops * T, 2, 2)
    v = R.split_views(data, crops, T)
    assert v.shape == (B, clips * crops, 3, T, 2, 2)
    theirs = []
    for clip in data.split(crops * T, dim=2):
        clip = clip.view((-1, 3, crops, T) + clip.shape[-2:]).contiguous()
        theirs.extend(clip[:, :, i, :] for i in range(crops))
    assert torch.equal(v, torch.stack(theirs, 1))
    with pytest.raises(ValueError):
        R.split_views(data[:, :, :-1], crops, T)


def test_load_encoder_filters_and_strips_keys(pkg):
    sys.path.insert(0, ROOT)
    from tests import parity
    R = pkg.lib.evaluation.retrieval
    sd = {'model.encoder.base_model.conv1.weight': 1, 'model.proj_head.fc.weight': 2, 'module.model.encoder.base_model.bn.bias': 3,
          'model.proj_head.encoder.x': 4}
    assert R.encoder_state_dict(sd) == {'base_model.conv1.weight': 1, 'base_model.bn.bias': 3}
    parity.register_tiny(pkg)
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'moco', 32, 20, 8)
    torch.manual_seed(4)
    model, _ = pkg.create_visual_model(cfg)
    ckpt = {'epoch': 1, 'state_dict': {k: v.clone() for k, v in model.state_dict().items()}}
    assert any('proj_head' in k for k in ckpt['state_dict']) and all(k.startswith('model.') for k in ckpt['state_dict'])
    enc = R.load_encoder(ckpt, 'R2P1D10T', 8)
    assert not enc.training and enc.feature_dim == model.model.encoder.feature_dim
    want = model.model.encoder.state_dict()
    got = enc.state_dict()
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    import io
    buf = io.BytesIO()
    torch.save(ckpt, buf)
    ckpt2 = torch.load(io.BytesIO(buf.getvalue()), map_location='cpu', weights_only=False)
    assert all(torch.equal(R.load_encoder(ckpt2, 'R2P1D10T', 8).state_dict()[k], want[k]) for k in want)


def test_retrieval_eval_tool(pkg, monkeypatch, tmp_path):
    """Argument names of the reference's search mode, topk_correct.json as it writes it; the search itself is the spec."""
    R = pkg.lib.evaluation.retrieval
    monkeypatch.setattr(R, 'search_first_hit', spec_search)
    spec = importlib.util.spec_from_file_location('retrieval_eval', os.path.join(ROOT, 'tools', 'retrieval_eval.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rs = np.random.RandomState(6)
    arrays = {'train_features': rs.standard_normal((120, 8)).astype(F32), 'train_classes': rs.randint(0, 10, 120),
              'val_features': rs.standard_normal((25, 8)).astype(F32) * 3, 'val_classes': rs.randint(0, 10, 25)}
    for name, arr in arrays.items():
        with open(tmp_path / (name + '.pkl'), 'wb') as fh:
            pickle.dump(arr, fh, protocol=pickle.HIGHEST_PROTOCOL)
    argv = ['--train_feature_path', str(tmp_path / 'train_features.pkl'), '--train_classes_path', str(tmp_path / 'train_classes.pkl'),
            '--val_feature_path', str(tmp_path / 'val_features.pkl'), '--val_classes_path', str(tmp_path / 'val_classes.pkl'),
            '--save_scores', str(tmp_path / 'out')]
    a = tool.get_parser().parse_args(argv)
    assert a.distance_metric == 'cosine' and a.norm is False
    out = tool.main(argv)
    assert out == str(tmp_path / 'out' / 'topk_correct.json')
    got = json.load(open(out))
    want = reference_counts(arrays['train_features'], arrays['train_classes'], arrays['val_features'], arrays['val_classes'],
                            (1, 5, 10, 20, 50))
    assert got == {str(k): v for k, v in want.items()}
    tool.main(argv + ['--distance_metric', 'euclidean', '--norm'])
    q = arrays['val_features'] / np.linalg.norm(arrays['val_features'], axis=1, keepdims=True)
    g = arrays['train_features'] / np.linalg.norm(arrays['train_features'], axis=1, keepdims=True)
    hit = ref.topk(q.astype(F32), g.astype(F32), 50, 'euclidean', arrays['val_classes'], arrays['train_classes'])[2]
    assert json.load(open(out)) == {str(k): int((hit <= k).sum()) for k in (1, 5, 10, 20, 50)}
    with pytest.raises(SystemExit):
        tool.get_parser().parse_args(argv + ['--distance_metric', 'manhattan'])


# ----------------------------------------------------------------------------- argument checks of the C entry
def test_entry_refuses_bad_arguments_before_any_launch(pkg):
    """Invariant (c): each of these returns GCA_EINVAL; no pointer is touched and nothing is launched (this runs without a
    GPU).  nq = 0 / ng = 0 with good arguments return GCA_OK, also without a launch."""
    lib = pkg._hip.lib
    big = 1 << 40

    def call(nq=4, ng=9, D=8, k=5, metric=0, ql=None, gl=None, slabs=0, ws_bytes=big, hit=None):
        return lib.gca_retrieval_topk(None, None, nq, ng, D, k, metric, ql, gl, slabs, None, None, hit, None, ws_bytes, None)

    bad = [dict(k=0), dict(k=65), dict(k=-3), dict(D=0), dict(D=-1), dict(nq=-1), dict(ng=-1), dict(slabs=-1), dict(metric=2),
           dict(metric=-1), dict(ql=8), dict(gl=8), dict(ql=8, gl=8), dict(ng=1 << 31),
           dict(ws_bytes=lib.gca_retrieval_ws_bytes(4, 9, 8, 5, 0) - 1), dict(ws_bytes=0)]
    for kw in bad:
        assert call(**kw) == -1, kw
    for kw in [dict(k=0), dict(k=65), dict(D=0), dict(nq=-1), dict(ng=-1), dict(slabs=-1), dict(ng=1 << 31)]:
        args = dict(nq=4, ng=9, D=8, k=5, slabs=0)
        args.update(kw)
        assert lib.gca_retrieval_ws_bytes(args['nq'], args['ng'], args['D'], args['k'], args['slabs']) == -1, kw
    assert call(nq=0) == 0 and call(ng=0) == 0 and call(nq=0, ng=0, ql=8, gl=8, hit=8) == 0
    assert lib.gca_retrieval_ws_bytes(4, 9, 8, 5, 0) == 64 + 4 * 1 * 5 * 8
    ops = pkg.engine.ops
    x = torch.zeros(4, 8)
    for kw in [dict(k=0), dict(k=65), dict(k=5, metric='manhattan'), dict(k=5, slabs=-1), dict(k=5, q_label=torch.zeros(4, dtype=torch.int64))]:
        with pytest.raises(ValueError):
            ops.retrieval_topk(x, torch.zeros(9, 8), **kw)
    with pytest.raises(ValueError):
        ops.retrieval_topk(x, torch.zeros(9, 7), 5)
