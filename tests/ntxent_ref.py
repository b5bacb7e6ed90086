"""Numpy (fp64) specification of gca_ntxent_fwd / gca_ntxent_bwd (csrc/ntxent.hip): NT-Xent, SimCLR's in-batch contrastive loss.

    z (N, D), N = 2b: rows 0..b-1 are view 1, rows b..2b-1 view 2;  pos(i) = (i + b) mod N;  inv_T = 1 / CONTRAST.NCE_T
    s[i,j]  = (sum_d z[i,d] * z[j,d]) * inv_T
    lse[i]  = m_i + log sum_{j != i} exp(s[i,j] - m_i),   m_i = max_{j != i} s[i,j]        (rows need not be unit-norm)
    sp[i]   = s[i, pos(i)]
    loss    = (1/N) sum_i (lse[i] - sp[i])
    rank[i] = #{ j : j != i, j != pos(i), s[i,j] >= sp[i] }                                 (top-k hit iff rank < k)
    P[i,j]  = exp(s[i,j] - lse[i]) for j != i, 0 on the diagonal
    dz[i,:] = g * inv_T / N * ( sum_j (P[i,j] + P[j,i]) z[j,:] - 2 z[pos(i),:] )

Dispatch of the kernels (ntxent_path; T = ceil(N / 32) tiles of 32 rows):
    fast     D <= 128, D % 4 == 0 and z / dz / workspace 16-byte aligned: 4 waves per workgroup
    generic  otherwise: 1 wave per workgroup, features in chunks of 128
    splits   clamp(ceil(256 / T), 1, ceil(T / waves)) slices of the streamed tiles, folded in order, in both directions

Inputs of the tests live here too, so the CPU tests can assert the properties the GPU tests rely on."""
import numpy as np

EXACT_INV_T = 16.0
EXACT_CASES = [(1, 8), (2, 8), (5, 32), (16, 128), (17, 128), (33, 128), (48, 64), (33, 130), (4, 1)]      # (b, D)
EXACT_PATHS = ['fast', 'fast', 'fast', 'fast', 'fast', 'fast', 'fast', 'generic', 'generic']
FLOAT_CASES = [(5, 32), (33, 128), (100, 128), (256, 128)]
FLOAT_TS = (0.07, 0.5)


def pos_index(N):
    return (np.arange(N) + N // 2) % N


def ntxent(z, inv_T, g=1.0):
    """-> dict(s, lse, sp, loss, rank, P, dz), everything in fp64 from the given values."""
    z = np.asarray(z, dtype=np.float64)
    N = z.shape[0]
    if N < 2 or N % 2:
        raise ValueError('N must be even and >= 2')
    pos = pos_index(N)
    s = (z @ z.T) * float(inv_T)
    off = ~np.eye(N, dtype=bool)
    sm = np.where(off, s, -np.inf)
    m = sm.max(axis=1)
    e = np.where(off, np.exp(sm - m[:, None]), 0.0)
    lse = m + np.log(e.sum(axis=1))
    sp = s[np.arange(N), pos]
    neg = off.copy()
    neg[np.arange(N), pos] = False
    rank = (neg & (s >= sp[:, None])).sum(axis=1).astype(np.int64)
    P = np.where(off, np.exp(sm - lse[:, None]), 0.0)
    dz = float(g) * float(inv_T) / N * ((P + P.T) @ z - 2.0 * z[pos])
    return dict(s=s, lse=lse, sp=sp, loss=float((lse - sp).mean()), rank=rank, P=P, dz=dz)


def rank_by_sort(s, N):
    """rank through a sort of each row's negatives: how many come before-or-level-with the positive in descending order."""
    pos = pos_index(N)
    out = np.zeros(N, dtype=np.int64)
    for i in range(N):
        negs = np.sort(np.array([s[i, j] for j in range(N) if j != i and j != pos[i]]))       # ascending
        out[i] = len(negs) - np.searchsorted(negs, s[i, pos[i]], side='left')
    return out


def ntxent_path(N, D, aligned=True):
    """The path gca_ntxent_fwd / _bwd take from their arguments alone -> (name, waves per workgroup, splits)."""
    fast = D <= 128 and D % 4 == 0 and aligned
    waves = 4 if fast else 1
    tiles = -(-N // 32)
    splits = min(max(-(-256 // tiles), 1), -(-tiles // waves))
    return ('fast' if fast else 'generic', waves, splits)


def exact_inputs(b, D, seed=0):
    """z (2b, D) fp32 with entries k / 8 in [-1, 1]: with inv_T = 16 every s[i,j] is a multiple of 1/4 below 2^12, the same
    number in fp32 and fp64 under any order of summation.  Row 0 is all ones and (b >= 2) row 1 repeats it, so s[0,1] =
    s[0,0] = 16 D: a tie with the diagonal and, for D >= 8, |s| > 88 -- exp overflows fp32 without the max subtraction.
    (b >= 2) the last row repeats row b = pos(0): s[i,N-1] = s[i,b] for every i, a tie with the positive of row 0."""
    rng = np.random.RandomState(1000 * b + D + seed)
    N = 2 * b
    z = rng.randint(-8, 9, size=(N, D)).astype(np.float32) / np.float32(8)
    z[0] = 1.0
    if b >= 2:
        z[1] = z[0]
        z[N - 1] = z[b]
    if b >= 5:
        z[b + 3] = z[2]                  # pos(2) = b + 2 sits next to a copy of row 2 itself
    return z


def float_inputs(b, D, seed=0, hard=False):
    """Unit rows (what the projection head's Normalize produces).  hard: rows that share a direction (cosines around 0.7)
    with norms spread over [0.5, 2] (4x), so the log-sum-exps differ from row to row and P != P^T by a wide margin, and row 0
    equal to its positive."""
    rng = np.random.RandomState(77 * b + D + seed)
    N = 2 * b
    z = rng.randn(N, D)
    if hard:
        z += 1.5 * rng.randn(1, D)
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    if hard:
        z *= np.exp(rng.uniform(np.log(0.5), np.log(2.0), size=(N, 1)))
        z[0] = z[b]
    return z.astype(np.float32)


def torch_chain(z, inv_T):
    """The same loss as a chain of torch ops (the comparator of tools/ntxent_micro.py and of test_ntxent_ref.py)."""
    import torch
    import torch.nn.functional as F
    N = z.shape[0]
    s = (z @ z.t()) * inv_T
    s = s.masked_fill(torch.eye(N, dtype=torch.bool, device=z.device), float('-inf'))
    target = (torch.arange(N, device=z.device) + N // 2) % N
    return F.cross_entropy(s, target)
