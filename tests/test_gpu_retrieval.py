"""gca_retrieval_topk / ops.retrieval_topk and the retrieval feature pass on the device, against tests/retrieval_ref.py.

Every search runs with slabs in {1, 3, 0} and the three outputs must agree bit for bit.  On operands that are exact in fp32
(tests/test_retrieval_ref.py asserts the preconditions) idx, dist and first_hit must be the specification's bits.  On float
operands the returned distances are held to the fp64 distance of the returned rows, and the ranking to the fp64 order
statistics; indices are NOT compared with an fp64 argsort (near-ties legitimately order differently in fp32).

Measured on an MI355X (maxima over queries and ranks, printed by test_float_operands; the bars in brackets):
    cosine     |dist - d64|                      D=65 1.70e-7   D=512 1.78e-7   D=1024 1.70e-7   D=2048 2.27e-7   [2e-6]
    euclidean  |dist^2 - d2_64| / (n2_q + n2_g)  D=65 2.50e-7   D=512 2.25e-7   D=1024 2.31e-7   D=2048 2.11e-7   [8e-6]
    rank error / bar: 0.031 at cosine D=2048 (one near-tie ordered differently in fp32), 0 everywhere else   [2]
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retrieval_cases as cases          # noqa: E402
import retrieval_ref as ref              # noqa: E402
from conftest import rel_err             # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def search(pkg, q, g, k, metric, q_label=None, g_label=None):
    """ops.retrieval_topk with every slab count of cases.SLABS, bitwise equal across them -> numpy (idx, dist, first_hit)."""
    qd, gd = torch.from_numpy(q).to(DEV), torch.from_numpy(g).to(DEV)
    ql = None if q_label is None else torch.from_numpy(np.asarray(q_label, dtype=np.int64)).to(DEV)
    gl = None if g_label is None else torch.from_numpy(np.asarray(g_label, dtype=np.int64)).to(DEV)
    outs = [pkg.engine.ops.retrieval_topk(qd, gd, k, metric, ql, gl, slabs) for slabs in cases.SLABS]
    for slabs, o in zip(cases.SLABS[1:], outs[1:]):
        assert torch.equal(o[0], outs[0][0]), ('idx', slabs)
        assert torch.equal(o[1].view(torch.int32), outs[0][1].view(torch.int32)), ('dist', slabs)
        assert (o[2] is None) == (outs[0][2] is None) and (o[2] is None or torch.equal(o[2], outs[0][2])), ('first_hit', slabs)
    idx, dist, hit = outs[0]
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and idx.shape == dist.shape == (len(q), k)
    return idx.cpu().numpy(), dist.cpu().numpy(), None if hit is None else hit.cpu().numpy()


def assert_spec_bits(got, q, g, k, metric, q_label=None, g_label=None):
    idx, dist, hit = got
    ridx, rdist, rhit = ref.topk(q, g, k, metric, q_label, g_label)
    assert np.array_equal(idx, ridx)
    nan = np.isnan(rdist)
    assert np.array_equal(np.isnan(dist), nan)
    assert np.array_equal(dist.view(np.uint32)[~nan], rdist.view(np.uint32)[~nan])
    assert (hit is None) == (rhit is None) and (hit is None or (hit.dtype == np.int32 and np.array_equal(hit, rhit)))
    for row in idx:                                                     # invariant (b)
        assert len(set(row[row >= 0])) == (row >= 0).sum()


# ----------------------------------------------------------------------------- exact operands
@pytest.mark.parametrize('k', [1, 50, 64])
def test_exact_cosine(pkg, k):
    q, g = cases.cosine_case()
    labels = (np.arange(33) % 7, np.arange(700) % 7)
    assert_spec_bits(search(pkg, q, g, k, 'cosine', *labels), q, g, k, 'cosine', *labels)


def test_exact_euclidean(pkg):
    q, g = cases.euclidean_case()
    labels = (np.arange(70) % 11, (np.arange(1000) * 7) % 11)
    assert_spec_bits(search(pkg, q, g, 50, 'euclidean', *labels), q, g, 50, 'euclidean', *labels)


@pytest.mark.parametrize('descending', [True, False])
def test_candidate_buffer_worst_cases(pkg, descending):
    """Descending: every later gallery row beats every threshold, so the candidate buffers fill and are re-selected all the
    way through.  Ascending: nothing after the first k passes."""
    q, g = cases.ramp_case(descending)
    got = search(pkg, q, g, 64, 'euclidean')
    assert_spec_bits(got, q, g, 64, 'euclidean')
    want = np.arange(4095, 4031, -1) if descending else np.arange(64)
    assert np.array_equal(got[0][0], want)


@pytest.mark.parametrize('metric', ref.METRICS)
def test_all_equal_gallery(pkg, metric):
    q, g = cases.all_equal_case()
    got = search(pkg, q, g, 64, metric)
    assert np.array_equal(got[0], np.tile(np.arange(64, dtype=np.int32), (5, 1)))
    assert_spec_bits(got, q, g, 64, metric)


@pytest.mark.parametrize('ng', [1, 31, 33, 2049])
@pytest.mark.parametrize('nq', [1, 31, 33, 130])
def test_shapes(pkg, nq, ng):
    """Sizes around the 32-row MFMA tile and the 128-row workgroup tile, more than one query tile and gallery tile, feature
    counts that are no multiple of 4 (scalar staging) or of the 32-feature chunk; ng < k leaves tails."""
    for D in (1, 3, 6, 65, 130):
        for metric in ref.METRICS:
            q, g = cases.shape_case(nq, ng, D, metric)
            labels = (np.arange(nq) % 5, (np.arange(ng) * 3) % 5)
            assert_spec_bits(search(pkg, q, g, 50, metric, *labels), q, g, 50, metric, *labels)


@pytest.mark.parametrize('metric', ref.METRICS)
def test_long_features(pkg, metric):
    q, g = cases.shape_case(33, 700, 1024, metric)
    assert_spec_bits(search(pkg, q, g, 50, metric), q, g, 50, metric)


def test_short_gallery_tails(pkg):
    q, g = cases.shape_case(33, 7, 6, 'euclidean')
    labels = (np.zeros(33, np.int64), np.arange(7) + 1)
    idx, dist, hit = got = search(pkg, q, g, 50, 'euclidean', *labels)
    assert (idx[:, 7:] == -1).all() and np.isposinf(dist[:, 7:]).all() and (idx[:, :7] >= 0).all() and (hit == 51).all()
    assert_spec_bits(got, q, g, 50, 'euclidean', *labels)


def test_empty_gallery_and_empty_queries(pkg):
    ops = pkg.engine.ops
    q = torch.ones(5, 6, device=DEV)
    for slabs in cases.SLABS:
        idx, dist, hit = ops.retrieval_topk(q, torch.empty(0, 6, device=DEV), 4, 'cosine', torch.zeros(5, dtype=torch.int64, device=DEV),
                                            torch.zeros(0, dtype=torch.int64, device=DEV), slabs)
        assert (idx == -1).all() and torch.isposinf(dist).all() and (hit == 5).all() and idx.shape == (5, 4)
        idx, dist, hit = ops.retrieval_topk(torch.empty(0, 6, device=DEV), q, 4, 'euclidean', slabs=slabs)
        assert idx.shape == (0, 4) and dist.shape == (0, 4) and hit is None


def test_zero_rows_under_cosine(pkg):
    q, g = cases.shape_case(33, 300, 16, 'cosine')
    q[4] = 0
    g[[0, 150, 299]] = 0
    got = search(pkg, q, g, 50, 'cosine')
    assert_spec_bits(got, q, g, 50, 'cosine')
    assert np.array_equal(got[0][4], np.arange(50)) and (got[1][4] == 1).all()            # a zero query: every distance is 1


@pytest.mark.parametrize('metric', ref.METRICS)
def test_nan_gallery_row_comes_last(pkg, metric):
    q, g = cases.shape_case(33, 300, 16, metric)
    clean = search(pkg, q, g, 50, metric)
    g2 = g.copy()
    g2[137] = np.nan
    got = search(pkg, q, g2, 50, metric)
    assert_spec_bits(got, q, g2, 50, metric)
    assert not (got[0] == 137).any()                                    # 299 other rows: it is not among the nearest 50
    for i in range(33):                                                 # and the other rows keep their order
        want = [j for j in ref.topk(q[i:i + 1], g, 51, metric)[0][0] if j != 137][:50]
        assert list(got[0][i]) == want
    assert clean[0].shape == got[0].shape
    few = search(pkg, q, g2[130:140], 50, metric)                       # a short gallery: the NaN row is the last real entry
    assert (few[0][:, 9] == 7).all() and np.isnan(few[1][:, 9]).all() and (few[0][:, 10:] == -1).all()
    assert_spec_bits(few, q, g2[130:140], 50, metric)


def test_first_hit(pkg):
    q, g = cases.euclidean_case()
    k = 50
    idx = ref.topk(q, g, k, 'euclidean')[0]
    ql = np.arange(70, dtype=np.int64)
    gl = np.full(1000, -1, dtype=np.int64)                              # no match anywhere
    assert (search(pkg, q, g, k, 'euclidean', ql, gl)[2] == k + 1).all()
    want = np.full(70, k + 1)
    for i, rank in [(0, 1), (1, k), (2, 7)]:                            # a match at rank 1, only at rank k, in between
        gl[idx[i, rank - 1]] = ql[i]
        want[i] = rank
    assert len({idx[0, 0], idx[1, k - 1], idx[2, 6]}) == 3
    got = search(pkg, q, g, k, 'euclidean', ql, gl)
    assert np.array_equal(got[2], ref.topk(q, g, k, 'euclidean', ql, gl)[2]) and np.array_equal(got[2], want)
    assert search(pkg, q, g, k, 'euclidean')[2] is None                 # without labels there is no first_hit
    # ... and the C entry leaves a first_hit pointer alone when it gets no labels
    H, ops = pkg._hip, pkg.engine.ops
    qd, gd = torch.from_numpy(q).to(DEV), torch.from_numpy(g).to(DEV)
    hit = torch.full((70,), 12345, dtype=torch.int32, device=DEV)
    oi, od = torch.empty(70, k, dtype=torch.int32, device=DEV), torch.empty(70, k, device=DEV)
    nbytes = H.lib.gca_retrieval_ws_bytes(70, 1000, 48, k, 0)
    ws = ops.WS.get(nbytes, DEV)
    assert H.lib.gca_retrieval_topk(H.ptr(qd), H.ptr(gd), 70, 1000, 48, k, 1, None, None, 0, H.ptr(oi), H.ptr(od), H.ptr(hit),
                                    H.ptr(ws), nbytes, H.stream()) == 0
    torch.cuda.synchronize()
    assert (hit == 12345).all() and np.array_equal(oi.cpu().numpy(), idx)


# ----------------------------------------------------------------------------- float operands
@pytest.mark.parametrize('metric', ref.METRICS)
@pytest.mark.parametrize('D', [65, 512, 1024, 2048])
def test_float_operands(pkg, D, metric):
    """Bars: the fp32-MFMA chain is bounded by 0.75-1.5e-7 sum|a b| for K <= 1024 and sum|a b| <= |a||b|; a sequential
    non-fused fp32 emulation of these very inputs gave 2.3e-7 (cosine) and 1.8e-6 relative (euclidean, D = 2048); the bars
    are 4-9x that.  cosine: |dist - d64| <= 2e-6; euclidean: |dist^2 - d2_64| <= 8e-6 (n2_q + n2_g)."""
    q, g = cases.float_case(D)
    k = 50
    idx, dist, _ = search(pkg, q, g, k, metric)
    key64 = ref.keys64(q, g, metric)                                    # cosine distance / squared euclidean distance
    assert (idx >= 0).all()
    got64 = np.take_along_axis(key64, idx.astype(np.int64), 1)
    if metric == 'cosine':
        bar = np.full(idx.shape, 2e-6)
        mine = dist.astype(np.float64)
    else:
        n2q, n2g = (q.astype(np.float64) ** 2).sum(1), (g.astype(np.float64) ** 2).sum(1)
        bar = 8e-6 * (n2q[:, None] + n2g[idx])
        mine = dist.astype(np.float64) ** 2
    err = np.abs(mine - got64)
    rank_err = np.abs(got64 - np.sort(key64, axis=1)[:, :k])
    print('retrieval float %s D=%d: max |dist - fp64| / bar unit = %.3e (bar %.1e), max rank error / bar = %.3f'
          % (metric, D, (err / bar).max() * (2e-6 if metric == 'cosine' else 8e-6), 2e-6 if metric == 'cosine' else 8e-6,
             (rank_err / bar).max()))
    assert (err <= bar).all()
    assert (rank_err <= 2 * bar).all()                                  # a lost or misplaced candidate shows here
    for row in idx:
        assert len(set(row)) == k
    assert (dist[:, 1:] >= dist[:, :-1]).all()


def test_repeated_calls_give_the_same_bits(pkg):
    q, g = cases.float_case(512)
    a, b = search(pkg, q, g, 50, 'cosine'), search(pkg, q, g, 50, 'cosine')
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ----------------------------------------------------------------------------- errors
def test_invalid_arguments_raise_and_launch_nothing(pkg):
    ops = pkg.engine.ops
    q, g = torch.ones(4, 8, device=DEV), torch.ones(9, 8, device=DEV)
    lab = torch.zeros(4, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    for kw in [dict(k=0), dict(k=65), dict(k=-1), dict(k=5, slabs=-1), dict(k=5, metric='manhattan'), dict(k=5, q_label=lab),
               dict(k=5, g_label=torch.zeros(9, dtype=torch.int64, device=DEV))]:
        with pytest.raises(ValueError):
            ops.retrieval_topk(q, g, **kw)
    with pytest.raises(ValueError):
        ops.retrieval_topk(torch.ones(4, 0, device=DEV), torch.ones(9, 0, device=DEV), 5)          # D < 1
    # the C entry itself: a workspace one byte short, labels on one side; outputs stay untouched
    H = pkg._hip
    idx, dist = torch.full((4, 5), 77, dtype=torch.int32, device=DEV), torch.full((4, 5), 77.0, device=DEV)
    nbytes = H.lib.gca_retrieval_ws_bytes(4, 9, 8, 5, 0)
    ws = ops.WS.get(nbytes, DEV)

    def entry(ws_bytes=nbytes, ql=None, gl=None, k=5, D=8):
        return H.lib.gca_retrieval_topk(H.ptr(q), H.ptr(g), 4, 9, D, k, 1, ql, gl, 0, H.ptr(idx), H.ptr(dist), None, H.ptr(ws),
                                        ws_bytes, H.stream())
    assert entry(ws_bytes=nbytes - 1) == -1 and entry(ql=H.ptr(lab)) == -1 and entry(k=65) == -1 and entry(D=0) == -1
    torch.cuda.synchronize()
    assert (idx == 77).all() and (dist == 77.0).all()
    assert entry() == 0
    torch.cuda.synchronize()
    assert (idx[:, 0] == 0).all() and (dist == 0).all()                 # (all-ones rows: distance 0, ties by index)


# ----------------------------------------------------------------------------- feature pass
@pytest.fixture(scope='module')
def checkpoint(pkg):
    """A checkpoint dict as the MoCo trainer writes it, after one step (so the BatchNorm running statistics have moved)."""
    from tests import parity
    parity.register_tiny(pkg)
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'moco', 32, 20, 8)
    trainer = pkg.MoCoTrainer(cfg, DEV, use_graph=False, seed=5)
    trainer.train_step(torch.randn(8, 6, 8, 48, 48, generator=torch.Generator().manual_seed(3)).to(DEV))
    sd = trainer.state_dict(epoch=1)
    return {k: ({n: t.detach().cpu().clone() for n, t in v.items()} if k == 'state_dict' else v) for k, v in sd.items()
            if k in ('epoch', 'state_dict')}


def oracle_encoder(pkg, checkpoint):
    from oracle import wrappers as owrap
    enc = owrap.VisualModelWrapper(8, 'R2P1D10T')
    enc.load_state_dict(pkg.lib.evaluation.encoder_state_dict(checkpoint['state_dict']))
    return enc.double().eval()


def test_extract_feature_single_vs_oracle(pkg, checkpoint):
    """B = 2, crops = 3, clips = 2, T = 8, 48 x 48: the mean over the six views of the fp64 oracle's eval-mode forward on the
    same weights, at the model bar of 1e-3; with softmax=True the softmax of that mean."""
    R = pkg.lib.evaluation.retrieval
    enc = R.load_encoder(checkpoint, 'R2P1D10T', 8).to(DEV)
    assert not enc.training
    ref_enc = oracle_encoder(pkg, checkpoint)
    B, crops, clips, T = 2, 3, 2, 8
    data = torch.randn(B, 3, clips * crops * T, 48, 48, generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        views = [ref_enc(data[:, :, v * T:(v + 1) * T].double()) for v in range(clips * crops)]
        want = torch.stack(views, 1).mean(1)
    got = R.extract_feature_single(enc, data.to(DEV), crops, T)
    assert got.shape == want.shape == (B, enc.feature_dim)
    assert rel_err(got, want) < 1e-3
    got_sm = R.extract_feature_single(enc, data.to(DEV), crops, T, softmax=True)
    assert rel_err(got_sm, torch.softmax(want, dim=-1)) < 1e-3
    assert float((views[0] - views[1]).abs().max()) > 1e-3 * float(want.abs().max())       # the views do differ
    enc.train()
    with pytest.raises(RuntimeError):
        R.extract_feature_single(enc, data.to(DEV), crops, T)


def test_checkpoint_to_recall_end_to_end(pkg, checkpoint, tmp_path):
    """load_encoder -> extract_features (the reference's pickles) -> topk_retrieval == the specification on those features."""
    import pickle
    R = pkg.lib.evaluation.retrieval
    enc = R.load_encoder(checkpoint, 'R2P1D10T', 8).to(DEV)
    gen = torch.Generator().manual_seed(21)
    crops, clips, T = 3, 2, 8

    def batches(n, classes):
        return [(torch.randn(2, 3, clips * crops * T, 48, 48, generator=gen), torch.tensor(classes[2 * i:2 * i + 2])) for i in range(n)]
    train_c, val_c = [0, 1, 2, 0, 1, 2], [2, 0, 1, 1]
    R.extract_features(enc, batches(3, train_c), crops, T, str(tmp_path), 'train', device=DEV)
    R.extract_features(enc, batches(2, val_c), crops, T, str(tmp_path), 'val', device=DEV)
    loaded = {}
    for split in ('train', 'val'):
        for path, kind in zip(R.feature_files(str(tmp_path), split), ('features', 'classes')):
            with open(path, 'rb') as fh:
                loaded[split, kind] = pickle.load(fh)
    assert loaded['train', 'features'].shape == (6, enc.feature_dim) and list(loaded['val', 'classes']) == val_c
    for metric in ref.METRICS:
        for norm in (False, True):
            correct, total = R.topk_retrieval(loaded['train', 'features'], loaded['train', 'classes'], loaded['val', 'features'],
                                              loaded['val', 'classes'], metric=metric, norm=norm, device=DEV)
            q, g = loaded['val', 'features'], loaded['train', 'features']
            if norm:
                q = torch.nn.functional.normalize(torch.from_numpy(q), dim=1).numpy()
                g = torch.nn.functional.normalize(torch.from_numpy(g), dim=1).numpy()
            hit = ref.topk(q, g, 50, metric, loaded['val', 'classes'], loaded['train', 'classes'])[2]
            assert total == 4 and correct == R.recall_counts(hit), (metric, norm)
            assert correct[50] == 4 and list(correct) == [1, 5, 10, 20, 50]
