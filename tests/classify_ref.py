"""fp64 specification of gca_classifier_fwd / gca_classifier_bwd (csrc/classifier.hip) and of the video-level metrics of
lib/evaluation/classify.py.  tests/test_classify_ref.py holds it to torch autograd, ref64.rank_ge and sklearn on the CPU;
tests/test_gpu_classify.py holds the kernels to it.

    logits[i,j] = (sum_d x[i,d] w[j,d]) + bias[j]
    row_lse[i]  = m_i + log sum_j exp(logits[i,j] - m_i),  m_i = max_j logits[i,j]
    loss        = (1/b) sum_i (row_lse[i] - logits[i,target[i]])
    rank_ge[i]  = #{ j != target[i] : logits[i,j] >= logits[i,target[i]] }
    g[i,j]      = s (exp(logits[i,j] - row_lse[i]) - [j == target[i]]),  s = gscale / b
    dw = g^T x,  dbias = sum_i g[i,:],  dx = g w
"""
import numpy as np
import torch


def _d(t):
    return torch.as_tensor(t).detach().cpu().double()


def logits(x, w, bias=None):
    out = _d(x) @ _d(w).t()
    return out if bias is None else out + _d(bias)


def row_lse(lg):
    lg = _d(lg)
    m = lg.max(dim=1, keepdim=True).values
    return (m + (lg - m).exp().sum(dim=1, keepdim=True).log()).reshape(-1)


def loss(lg, target):
    lg, t = _d(lg), torch.as_tensor(target).cpu().long()
    return (row_lse(lg) - lg.gather(1, t[:, None]).reshape(-1)).sum() / lg.shape[0]


def rank_ge(lg, target):
    lg, t = _d(lg), torch.as_tensor(target).cpu().long()
    ref = lg.gather(1, t[:, None])
    other = torch.arange(lg.shape[1])[None, :] != t[:, None]
    return ((lg >= ref) & other).sum(1).to(torch.int32)


def forward(x, w, bias, target):
    """-> (logits, row_lse, loss, rank_ge), all from the fp64 logits."""
    lg = logits(x, w, bias)
    return lg, row_lse(lg), loss(lg, target), rank_ge(lg, target)


def backward(x, w, lg, lse, target, gscale=1.0):
    """-> (dw, dbias, dx) of gscale * loss."""
    x, w, lg, lse = _d(x), _d(w), _d(lg), _d(lse)
    t = torch.as_tensor(target).cpu().long()
    g = (lg - lse[:, None]).exp()
    g[torch.arange(lg.shape[0]), t] -= 1.0
    g *= float(gscale) / lg.shape[0]
    return g.t() @ x, g.sum(0), g @ w


def confusion(labels, pred, num_class):
    """(C, C) counts: row = label, column = prediction."""
    cf = np.zeros((num_class, num_class), dtype=np.int64)
    for t, p in zip(np.asarray(labels).reshape(-1), np.asarray(pred).reshape(-1)):
        cf[int(t), int(p)] += 1
    return cf


def mean_class_acc(cf):
    """Mean of hits / count over the classes that occur as a label."""
    cf = np.asarray(cf, dtype=np.float64)
    accs = [cf[c, c] / cf[c].sum() for c in range(cf.shape[0]) if cf[c].sum() > 0]
    return float(np.mean(accs))
