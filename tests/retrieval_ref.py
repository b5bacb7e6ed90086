"""Numpy specification of gca_retrieval_topk (csrc/retrieval.hip): what tools/video_retrieval.py:174-197 of the reference
computes with sklearn's cosine_distances / euclidean_distances and np.argsort, with the points it leaves open fixed.

    s       = q . g                                    here in fp64 from the given inputs (the kernel: fp32 matrix cores)
    n2      = |row|^2
    cosine:    r = 1 / sqrt(n2), 0 for an all-zero row (sklearn's normalize leaves such a row alone);
               key = dist = 1 - (s r_q) r_g
    euclidean: key = d2 = max(0, (n2_q + n2_g) - 2 s), NaN kept;  dist = sqrt(d2)
    order:     ascending by (key, gallery index) = np.argsort(kind='stable'); a NaN key sorts after +inf, -0 counts as +0
    tails:     ng < k  ->  idx = -1, dist = +inf
    first_hit: 1-based rank of the first returned row whose label equals the query's, k + 1 if there is none

`dtype` is the format the keys are rounded to before they are ordered: float32 is the kernel's contract (on operands whose
scores, norms and keys are exact in fp32 the kernel returns these very bits), float64 leaves them as computed (the
comparison with sklearn, and the yardstick of the float-data tests)."""
import numpy as np

METRICS = ('cosine', 'euclidean')


def keys64(q, g, metric):
    """(nq, ng) fp64 ranking keys: the cosine distance, or the squared euclidean distance."""
    q, g = np.asarray(q, dtype=np.float64), np.asarray(g, dtype=np.float64)
    with np.errstate(all='ignore'):
        s = q @ g.T
        n2q, n2g = (q * q).sum(1), (g * g).sum(1)
        if metric == 'cosine':
            rq = np.where(n2q == 0, 0.0, 1.0 / np.sqrt(np.where(n2q == 0, 1.0, n2q)))
            rg = np.where(n2g == 0, 0.0, 1.0 / np.sqrt(np.where(n2g == 0, 1.0, n2g)))
            return 1.0 - (s * rq[:, None]) * rg[None, :]
        if metric == 'euclidean':
            d2 = (n2q[:, None] + n2g[None, :]) - 2.0 * s
            return np.where(d2 < 0, 0.0, d2)
    raise ValueError(metric)


def dist_of_key(key, metric):
    with np.errstate(all='ignore'):
        return np.sqrt(key) if metric == 'euclidean' else key


def order_words(key32):
    """fp32 keys (nq, ng) -> uint64 words (order-preserving u32 of the key) << 32 | gallery index: the k smallest words of
    a row are its result."""
    key32 = np.ascontiguousarray(key32, dtype=np.float32) + np.float32(0)          # -0 -> +0
    u = key32.view(np.uint32).astype(np.uint64)
    u = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    u = np.where(np.isnan(key32), np.uint64(0xFFFFFFFF), u).astype(np.uint64)
    return (u << np.uint64(32)) | np.arange(key32.shape[1], dtype=np.uint64)[None, :]


def first_hit_of(idx, q_label, g_label, k):
    g_label = np.asarray(g_label)
    hit = np.zeros(idx.shape, dtype=bool)
    valid = idx >= 0
    hit[valid] = (g_label[idx[valid]] == np.broadcast_to(np.asarray(q_label)[:, None], idx.shape)[valid])
    return np.where(hit.any(1), hit.argmax(1) + 1, k + 1).astype(np.int32)


def topk(q, g, k, metric='cosine', q_label=None, g_label=None, dtype=np.float32):
    """-> (idx (nq, k) int32, dist (nq, k) dtype, first_hit (nq,) int32 or None)."""
    assert metric in METRICS and k >= 1
    q, g = np.asarray(q), np.asarray(g)
    nq, ng = q.shape[0], g.shape[0]
    key = keys64(q, g, metric).astype(dtype) + dtype(0) if ng else np.zeros((nq, 0), dtype)
    # NaN last, then key, then index: argsort puts NaN last already and 'stable' keeps equal keys in index order
    order = np.argsort(key, axis=1, kind='stable')[:, :k]
    m = order.shape[1]
    idx = np.full((nq, k), -1, dtype=np.int32)
    dist = np.full((nq, k), np.inf, dtype=dtype)
    idx[:, :m] = order
    dist[:, :m] = dist_of_key(np.take_along_axis(key, order, 1), metric)
    hit = None
    if q_label is not None:
        hit = first_hit_of(idx, q_label, g_label, k)
    return idx, dist, hit
