"""Inputs of the k-NN vote tests, shared by tests/test_knn_ref.py (which asserts the preconditions) and
tests/test_gpu_knn.py (which then compares exactly): hand-built (idx, dist, labels) as gca_retrieval_topk would write them."""
import functools

import numpy as np

NQS = (1, 3, 4, 5, 9)                 # four queries per workgroup: partial and several workgroups
KS = (1, 2, 63, 64)
CS = (1, 2, 101, 100000)
TS = (0.05, 0.07, 1.0)
GAP = 1e-3                            # least fp64 relative gap the exact pred / rank comparison of a float case rests on


def kvotes(k):
    return sorted({1, max(1, k - 1), k})


def random_case(nq, k, C, seed, ng=300, tails=True):
    """Rows of distinct gallery indices with ascending distances in [0, 2], labels in [0, C), query labels that occur among
    the neighbours for even rows and are arbitrary for odd rows; when `tails`, the last row ends in tail slots."""
    rs = np.random.RandomState(seed)
    idx = np.stack([rs.permutation(ng)[:k] for _ in range(nq)]).astype(np.int32)
    dist = np.sort(rs.uniform(0.0, 2.0, size=(nq, k)), axis=1).astype(np.float32)
    g_label = rs.randint(0, min(C, 40), size=ng).astype(np.int64) * max(1, C // 40) % C      # spread over [0, C), few distinct
    q_label = np.where(np.arange(nq) % 2 == 0, g_label[idx[:, k // 2]], rs.randint(0, C, size=nq)).astype(np.int64)
    if tails and k > 2:
        idx[-1, k - k // 3:] = -1
        dist[-1, k - k // 3:] = np.inf
    return dict(idx=idx, dist=dist, g_label=g_label, q_label=q_label, C=C, ng=ng)


# (nq, k, C, seed): every nq / k / C of the lists above occurs; the seeds are those for which test_knn_ref's precondition
# holds for every kvote of kvotes(k) and every T of TS (found by trying seeds upwards from 0)
FLOAT_CASES = ((1, 64, 2, 0), (3, 63, 101, 0), (4, 2, 101, 0), (5, 1, 1, 0), (9, 64, 101, 0), (9, 64, 100000, 0), (5, 63, 2, 0),
               (4, 1, 100000, 0))


@functools.lru_cache(maxsize=None)
def float_case(nq, k, C, seed):
    return random_case(nq, k, C, 7000 + seed)


def content_case():
    """k = 8, ng = 80, C = 101: one row per rule of the specification.  g_label[j] = j % 7 for j < 64, then entries outside
    [0, C) and the largest class."""
    k, ng, C = 8, 80, 101
    g_label = np.arange(ng, dtype=np.int64) % 7
    g_label[64:70] = [-1, 101, 2 ** 40, 100, -2 ** 40, 2 ** 31]
    inf, nan = np.inf, np.nan
    ramp = [0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0]
    rows = [
        # (idx, dist, q_label, what)
        ([0, 7, 14, 21, 28, 35, 42, 49], ramp, 0, 'all neighbours in one class'),
        ([1, 2, 3, 8, 9, 10, 15, 16], ramp, 5, 'target class absent, unvoted classes 0 and 4 below it'),
        ([1, 2, 3, 8, 9, 10, 15, 16], ramp, 100, 'target score 0 far up: every unvoted class below counts'),
        ([1, 2, 3, 8, 9, 10, 15, 16], ramp, 0, 'target score 0 at class 0: only the voted classes come first'),
        ([5, 12, -1, -1, -1, -1, -1, -1], [0.5, 0.75] + [inf] * 6, 5, 'tail slots'),
        ([80, 200, 2 ** 31 - 1, 3, -7, 81, 4, 10], ramp, 4, 'idx >= ng and negative idx'),
        ([64, 65, 66, 67, 68, 69, 4, 11], ramp, 100, 'labels outside [0, C): only 67 (class 100), 4 and 11 vote'),
        ([6, 13, 20, 27, 5, 33, 34, 41], [0.125, nan, inf, 0.5, nan, 0.75, inf, inf], 6, 'NaN slots skipped, +inf slots vote'),
        ([2, 9, 3, 10, 4, 11, 5, 12], [0.0, 0.0, 0.0, 2.0, 2.0, 2.0, 2.0, 2.0], 3, 'dist 0 and 2'),
        ([-1] * 8, [inf] * 8, 3, 'no valid slot'),
        ([64, 65, 66, 68, 69, 90, -1, -1], ramp, 3, 'no valid slot: labels and indices out of range'),
        ([3, 1, 10, 8, 17, 15, 0, 7], [0.5] * 8, 0, 'classes 3 and 1 tie at three voters: the lower class comes first'),
        ([1, 3, 8, 10, 15, 17, 0, 7], [0.5] * 8, 3, 'the same tie met in the other order'),
    ]
    idx = np.array([r[0] for r in rows], dtype=np.int64).astype(np.int32)
    dist = np.array([r[1] for r in rows], dtype=np.float32)
    q_label = np.array([r[2] for r in rows], dtype=np.int64)
    return dict(idx=idx, dist=dist, g_label=g_label, q_label=q_label, C=C, ng=ng, what=[r[3] for r in rows])


def distinct_classes_case():
    """64 neighbours in 64 distinct classes (every lane leads its own class), equal weights: class order decides."""
    k, ng, C = 64, 64, 101
    rs = np.random.RandomState(5)
    g_label = (rs.permutation(C)[:ng]).astype(np.int64)
    idx = np.stack([rs.permutation(ng) for _ in range(5)]).astype(np.int32)
    dist = np.full((5, k), 0.5, dtype=np.float32)
    q_label = np.array([g_label.min(), g_label.max(), sorted(g_label)[30], min(set(range(C)) - set(g_label)), 100], dtype=np.int64)
    return dict(idx=idx, dist=dist, g_label=g_label, q_label=q_label, C=C, ng=ng)


def loo_case():
    """Leave-one-out with self_base = 40, k = 6: row 0 meets itself in slot 0, row 1 in slot 2 (with kvote = 3 the slot
    of rank 3 is promoted into the vote), row 2 not at all, row 3 in the last slot."""
    base, k, ng, C = 40, 6, 60, 7
    g_label = np.arange(ng, dtype=np.int64) % C
    idx = np.array([[40, 1, 2, 3, 4, 5], [8, 15, 41, 9, 22, 10], [42 + 7, 1, 8, 2, 9, 3], [0, 7, 14, 1, 2, 43]], dtype=np.int32)
    dist = np.tile(np.array([0.0, 0.25, 0.5, 0.75, 1.0, 1.25], dtype=np.float32), (4, 1))
    q_label = g_label[base + np.arange(4)]
    return dict(idx=idx, dist=dist, g_label=g_label, q_label=q_label, C=C, ng=ng, self_base=base)
