"""Numpy (fp64) specification of gca_mocov3_fwd / gca_mocov3_bwd (csrc/mocov3.hip): MoCo v3's symmetrised cross-view InfoNCE
(Chen, Xie, He 2021, Algorithm 1).

    q1, q2 (N, D): the student's predictor outputs of the two views;  k1, k2 (N, D): the momentum teacher's projector outputs
    direction 0 pairs (q, k) = (q1, k2), direction 1 pairs (q2, k1);  inv_T = 1 / CONTRAST.NCE_T;  per direction d:
    s[i,j]  = (sum_e q[i,e] * k[j,e]) * inv_T
    lse[i]  = m_i + log sum_j exp(s[i,j] - m_i),   m_i = max_j s[i,j]          (ALL j, the diagonal included)
    sp[i]   = s[i,i]
    l_d     = (1/N) sum_i (lse[i] - sp[i])
    rank[i] = #{ j != i : s[i,j] >= sp[i] }                                   (top-k hit iff rank < k)
    P[i,j]  = exp(s[i,j] - lse[i])
    dq[i,:] = g * w * inv_T / N * ( sum_j P[i,j] k[j,:] - k[i,:] )            (nothing flows to k)
    loss    = w * (l_0 + l_1),   w = 2 T as the host rounds it to fp32

Dispatch of the kernels (mocov3_path; T = ceil(N / 32) tiles of 32 rows):
    fast     D <= 256, D % 4 == 0 and every pointer 16-byte aligned: 4 waves per workgroup, features in chunks of 128
    generic  otherwise: 1 wave per workgroup, features in chunks of 128
    splits   clamp(ceil(256 / T), 1, ceil(T / waves)) slices of the streamed tiles per direction, folded in order

Inputs of the tests live here too, so the CPU tests can assert the properties the GPU tests rely on."""
import numpy as np

EXACT_INV_T = 16.0
EXACT_CASES = [(1, 8), (2, 8), (5, 32), (32, 128), (33, 128), (64, 256), (97, 256), (33, 130), (4, 1)]      # (N, D)
EXACT_PATHS = ['fast', 'fast', 'fast', 'fast', 'fast', 'fast', 'fast', 'generic', 'generic']
FLOAT_CASES = [(5, 32), (33, 128), (100, 256), (257, 256)]
FLOAT_TS = (0.2, 0.5)
HARD_CASES = [(33, 256, 'fast'), (40, 130, 'generic')]                   # at T = 0.5
HARD_T = 0.5
FAST_MAX_D = 256
RANK_MARGIN = 1e-5               # rank is compared on rows with no other column within RANK_MARGIN * max|s| of the positive


def weight(inv_T):
    """2 T as the host rounds it to fp32."""
    return float(np.float32(2.0 / float(inv_T)))


def direction(q, k, inv_T, coef):
    q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
    N = q.shape[0]
    s = (q @ k.T) * float(inv_T)
    m = s.max(axis=1)
    lse = m + np.log(np.exp(s - m[:, None]).sum(axis=1))
    sp = np.diagonal(s).copy()
    off = ~np.eye(N, dtype=bool)
    rank = (off & (s >= sp[:, None])).sum(axis=1).astype(np.int64)
    P = np.exp(s - lse[:, None])
    dq = coef / N * (P @ k - k)
    return dict(s=s, lse=lse, sp=sp, l=float((lse - sp).mean()), rank=rank, P=P, dq=dq)


def mocov3(q1, q2, k1, k2, inv_T, w=None, g=1.0):
    """-> dict(s, lse, sp, l, rank, P, dq: [direction 0, direction 1] each; loss), everything in fp64 from the given values."""
    w = weight(inv_T) if w is None else float(w)
    coef = float(g) * w * float(inv_T)
    d = [direction(q1, k2, inv_T, coef), direction(q2, k1, inv_T, coef)]
    out = {key: [d[0][key], d[1][key]] for key in d[0]}
    out['loss'] = w * (d[0]['l'] + d[1]['l'])
    return out


def rank_by_sort(s):
    """rank through a sort of each row's other columns: how many come before-or-level-with the positive in descending order."""
    N = s.shape[0]
    out = np.zeros(N, dtype=np.int64)
    for i in range(N):
        others = np.sort(np.delete(s[i], i))                             # ascending
        out[i] = len(others) - np.searchsorted(others, s[i, i], side='left')
    return out


def clear_rows(s, margin=RANK_MARGIN):
    """Rows whose rank no error below margin * max|s| can change: no other column that close to the positive."""
    N = s.shape[0]
    gap = np.abs(s - np.diagonal(s)[:, None])
    gap[np.arange(N), np.arange(N)] = np.inf
    return gap.min(axis=1, initial=np.inf) > margin * np.abs(s).max()


def mocov3_path(N, D, aligned=True):
    """The path gca_mocov3_fwd / _bwd take from their arguments alone -> (name, waves per workgroup, splits)."""
    fast = D <= FAST_MAX_D and D % 4 == 0 and aligned
    waves = 4 if fast else 1
    tiles = -(-N // 32)
    splits = min(max(-(-256 // tiles), 1), -(-tiles // waves))
    return ('fast' if fast else 'generic', waves, splits)


def _exact_pair(rng, N, D):
    # sparse random rows: their logits stay around |s| <= 20, where the fp32 row_lse that the backward pass reads resolves
    # exp(s - lse) to well under the bar (at |s| ~ 250, dense rows, its rounding alone costs 7e-6 of dq); the planted rows
    # below are dense and carry the large logits, each with ONE dominant column, whose lse is a representable number
    dens = 1.0 if D < 8 else np.sqrt(0.6 / D)
    q = (rng.randint(-8, 9, size=(N, D)) * (rng.rand(N, D) < dens)).astype(np.float32) / np.float32(8)
    k = (rng.randint(-8, 9, size=(N, D)) * (rng.rand(N, D) < dens)).astype(np.float32) / np.float32(8)
    q[0] = 1.0
    k[0] = 1.0                           # s[0,0] = 16 D: for D >= 8 above 88, exp overflows fp32 without the max subtraction
    if N >= 2:
        k[1] = 1.0                       # column 0 ties with the positive of row 1 ...
        if D >= 3:                       # ... through another key (equal keys would make dq vanish for N = 2), at |s| <= 18,
            k[1, 0] = k[1, 1] = 0.5      # where an fp32 lse still resolves the softmax of a tie to the bar
            q[1] = 0.0
            q[1, 0], q[1, 1], q[1, 2] = 0.5, -0.5, 0.125
    if N >= 5:
        q[2, 0] = 1.0
        k[3] = np.sign(q[2])             # the largest s row 2 can reach ...
        k[2] = k[3] / np.float32(2)      # ... and its positive at half of it: column 3 beats the positive of row 2
    return q, k


def exact_inputs(N, D, seed=0):
    """(q1, q2, k1, k2) fp32 with entries m / 8 in [-1, 1]: with inv_T = 16 every s[i,j] is a multiple of 1/4 of magnitude at
    most 16 D <= 2^12, the same number in fp32 and fp64 under any order of summation.  In both directions: row 0 of q and of k is all
    ones (s[0,0] = 16 D > 88 for D >= 8); (N >= 2) column 0 scores exactly what the positive of row 1 does, a tie, through a
    different key for D >= 3; (N >= 5) column 3 scores twice the positive of row 2."""
    rng = np.random.RandomState(1000 * N + D + seed)
    q1, k2 = _exact_pair(rng, N, D)
    q2, k1 = _exact_pair(rng, N, D)
    return q1, q2, k1, k2


def float_inputs(N, D, seed=0, hard=False):
    """(q1, q2, k1, k2) fp32.  Unit rows, each a perturbed copy of its clip's direction, so cos(q[i], k[i]) is about 0.9 as at
    the start of training (the teacher is a copy of the student).  hard: the clips share a direction, the row norms of q and of
    k are spread over [0.5, 2] (4x) independently, and row 0 of each q equals its key."""
    rng = np.random.RandomState(77 * N + D + seed)
    base = rng.randn(N, D)
    if hard:
        base += 1.5 * rng.randn(1, D)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    out = []
    for _ in range(4):
        x = base + rng.randn(N, D) * np.sqrt(0.11 / D)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        if hard:
            x *= np.exp(rng.uniform(np.log(0.5), np.log(2.0), size=(N, 1)))
        out.append(x)
    q1, q2, k1, k2 = out
    if hard:
        q1[0] = k2[0]
        q2[0] = k1[0]
    return tuple(x.astype(np.float32) for x in (q1, q2, k1, k2))


def torch_chain(q1, q2, k1, k2, T):
    """The literal loss of Algorithm 1 as a chain of torch ops (the comparator of tools/mocov3_micro.py and test_mocov3_ref.py)."""
    import torch
    import torch.nn.functional as F
    target = torch.arange(q1.shape[0], device=q1.device)
    return 2 * T * (F.cross_entropy(q1 @ k2.t() / T, target) + F.cross_entropy(q2 @ k1.t() / T, target))
