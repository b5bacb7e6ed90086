"""Numpy specification of gca_knn_vote (csrc/knn.hip): the weighted k-NN vote of InstDisc / MoCo / SimSiam evaluations on
the (idx, dist) lists of gca_retrieval_topk.

    valid slot j of query i:  0 <= idx[i,j] < ng,  idx[i,j] != self_base + i (self_base >= 0: leave-one-out),
                              g_label[idx[i,j]] in [0, C),  dist[i,j] not NaN
    voters:      the first kvote valid slots in rank order
    weight:      'uniform' 1;  'exp' exp(-(dist * inv_T)), inv_T the fp32 value of 1 / T
    score[c]:    sum of the weights of class c's voters, in rank order; 0 for a class without voters
    order:       score descending, then class index ascending, over all C classes
    pred:        the first class of that order;  rank: the number of classes other than q_label before q_label
    no voter:    pred = -1, rank = C

vote() computes in fp64 from the given fp32 distances (the yardstick of the float cases); order32=True rounds as the kernel
does -- the product to fp32, the weight to fp32, the sum in fp32 in rank order -- with numpy's exp in place of the device
expf, so it states the kernel's bits wherever the weights are exact (uniform weights; dist = 0)."""
import numpy as np

WEIGHTINGS = ('uniform', 'exp')


def inv_T32(T):
    """What ops.knn_vote hands the kernel: the fp32 rounding of the fp64 quotient 1 / T."""
    return np.float32(1.0 / float(T))


def voters(idx, dist, g_label, C, kvote, self_base=-1):
    """-> list over queries of [(slot, class)] in rank order."""
    idx, dist, g_label = np.asarray(idx), np.asarray(dist), np.asarray(g_label)
    out = []
    for i in range(idx.shape[0]):
        row = []
        for j in range(idx.shape[1]):
            gi = int(idx[i, j])
            if len(row) == kvote:
                break
            if gi < 0 or gi >= len(g_label) or (self_base >= 0 and gi == self_base + i) or np.isnan(dist[i, j]):
                continue
            c = int(g_label[gi])
            if 0 <= c < C:
                row.append((j, c))
        out.append(row)
    return out


def weights(dist, weighting, T, order32=False):
    assert weighting in WEIGHTINGS
    dist = np.asarray(dist, dtype=np.float32)
    if weighting == 'uniform':
        return np.ones(dist.shape, dtype=np.float32 if order32 else np.float64)
    with np.errstate(all='ignore'):
        if order32:
            t = (dist * inv_T32(T)).astype(np.float32)                    # one fp32 rounding of the product
            return np.exp(-t.astype(np.float64)).astype(np.float32)
        return np.exp(-(dist.astype(np.float64) * np.float64(inv_T32(T))))


def order_of(scores_row):
    """Class indices of one score row, score descending then class ascending."""
    return np.lexsort((np.arange(len(scores_row)), -scores_row))


def vote(idx, dist, g_label, C, kvote=None, q_label=None, self_base=-1, weighting='exp', T=0.07, order32=False):
    """-> (scores (nq, C) fp64 or fp32, pred (nq,) int32, rank (nq,) int32 or None)."""
    idx = np.asarray(idx)
    nq, k = idx.shape
    kvote = k if kvote is None else kvote
    assert 1 <= kvote <= k
    dt = np.float32 if order32 else np.float64
    w = weights(dist, weighting, T, order32)
    scores = np.zeros((nq, C), dtype=dt)
    pred = np.full(nq, -1, dtype=np.int32)
    rank = None if q_label is None else np.full(nq, C, dtype=np.int32)
    for i, row in enumerate(voters(idx, dist, g_label, C, kvote, self_base)):
        for j, c in row:
            scores[i, c] = dt(scores[i, c] + w[i, j])                      # rank order, one rounding per addition
        if not row:
            continue
        order = order_of(scores[i])
        pred[i] = order[0]
        if q_label is not None:
            t = int(q_label[i])
            rank[i] = int(np.nonzero(order == t)[0][0])                    # classes before t are all != t
    return scores, pred, rank


def gaps(scores, q_label):
    """Smallest relative gap of every row that the exact comparison of pred / rank rests on: between the best and the
    second-best class score, and between the target's score and its neighbours in the order (relative to the larger of the
    two; rows where both are 0 -- unvoted classes, ordered by index -- do not count)."""
    out = np.full(scores.shape[0], np.inf)
    for i in range(scores.shape[0]):
        s = np.sort(scores[i])[::-1]
        pairs = [(s[0], s[1])] if len(s) > 1 else []
        t = scores[i, int(q_label[i])]
        above, below = scores[i][scores[i] > t], scores[i][scores[i] < t]
        others = np.delete(scores[i], int(q_label[i]))
        if (others == t).any() and t > 0:
            pairs.append((t, t))
        if above.size:
            pairs.append((above.min(), t))
        if below.size:
            pairs.append((t, below.max()))
        for a, b in pairs:
            if a > 0:
                out[i] = min(out[i], (a - b) / a)
    return out
