"""ReSSL's relational loss (Zheng et al. 2021), the fp64 statement of gca_ressl_fwd / gca_ressl_bwd (csrc/ressl.hip), the inputs
of its tests, the wrong variants those inputs must expose, and the dispatch rule of the kernels restated in Python.

    s[i,j] = inv_Ts q_i . Q_j            t[i,j] = inv_Tt k_i . Q_j
    lse_s[i] = logsumexp_j s[i,:]        lse_t[i] = logsumexp_j t[i,:]       Ps = exp(s - lse_s)     Pt = exp(t - lse_t)
    O_s = Ps Q                           O_t = Pt Q
    loss_i = lse_s[i] - sum_j Pt[i,j] s[i,j]  ( = lse_s[i] - inv_Ts q_i . O_t[i] )      loss = mean_i loss_i
    ent_i  = lse_t[i] - sum_j Pt[i,j] t[i,j]                                            ent  = mean_i ent_i
    dq[i]  = g inv_Ts / N (O_s[i] - O_t[i])

which is the gradient of the literal -(softmax(t) * log_softmax(s)).sum(1).mean() to q (torch_chain; tests/test_ressl_ref.py
holds the two together at 1e-12).  Every function takes the fp32 inputs the device sees and computes in fp64."""
import numpy as np

BAR = 1e-5                                       # the suite's per-op bar, on the logit scale (tests/test_gpu_mocov3.py: BAR)
SPEC_CASES = [(1, 8, 1), (5, 32, 7), (33, 128, 100), (64, 128, 3075), (40, 130, 200), (97, 256, 1000)]
FLOAT_CASES = [(5, 32, 7), (33, 128, 100), (64, 128, 3075), (97, 256, 1000), (33, 130, 200), (1, 128, 65)]
FLOAT_PATHS = ['fast', 'fast', 'fast', 'fast', 'generic', 'fast']
TEMPS = [(0.1, 0.04), (0.2, 0.2)]                # (Ts, Tt): the paper's pair, and equal temperatures
KINDS = ['easy', 'hard', 'overflow']
REPEAT_CASES = [(33, 128, 100), (64, 256, 3075), (33, 130, 200)]


def _lse(x):
    m = x.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]


def ressl(q, k, Q, inv_Ts, inv_Tt, g=1.0):
    """-> dict: lse_s, lse_t, row_loss, row_ent (N,), loss, ent, dq, Os, Ot (N, D), coef, smax = max(|s|, |t|), and
    oscale = coef * max(|O_s|inf, |O_t|inf), the scale the gradient bar is taken on."""
    q, k, Q = (np.asarray(a, dtype=np.float64) for a in (q, k, Q))
    inv_Ts, inv_Tt, g = float(inv_Ts), float(inv_Tt), float(g)
    N = q.shape[0]
    s, t = inv_Ts * (q @ Q.T), inv_Tt * (k @ Q.T)
    lse_s, lse_t = _lse(s), _lse(t)
    Ps, Pt = np.exp(s - lse_s[:, None]), np.exp(t - lse_t[:, None])
    Os, Ot = Ps @ Q, Pt @ Q
    row_loss = lse_s - (Pt * s).sum(axis=1)
    row_ent = lse_t - (Pt * t).sum(axis=1)
    coef = g * inv_Ts / N
    return dict(lse_s=lse_s, lse_t=lse_t, row_loss=row_loss, row_ent=row_ent, loss=float(row_loss.mean()),
                ent=float(row_ent.mean()), dq=coef * (Os - Ot), Os=Os, Ot=Ot, coef=coef,
                smax=float(max(np.abs(s).max(), np.abs(t).max())), tmax=float(np.abs(t).max()),
                oscale=abs(coef) * float(max(np.abs(Os).max(), np.abs(Ot).max())))


def torch_chain(q, k, Q, Ts, Tt):
    """The literal loss on torch tensors (autograd flows to q only)."""
    import torch
    s = q @ Q.t() / Ts
    t = k.detach() @ Q.t() / Tt
    return -(torch.softmax(t, dim=1) * torch.log_softmax(s, dim=1)).sum(dim=1).mean()


def ressl_f32(q, k, Q, inv_Ts, inv_Tt, g=1.0):
    """The same formulas in plain fp32 numpy (what fp32 arithmetic alone costs) -> dict(lse_s, lse_t, row_loss, loss, ent, dq)."""
    f = np.float32
    q, k, Q = (np.asarray(a, dtype=f) for a in (q, k, Q))
    N = q.shape[0]
    s, t = f(inv_Ts) * (q @ Q.T), f(inv_Tt) * (k @ Q.T)
    lse_s, lse_t = _lse(s), _lse(t)
    Ps, Pt = np.exp(s - lse_s[:, None]), np.exp(t - lse_t[:, None])
    row_loss = lse_s - (Pt * s).sum(axis=1)
    row_ent = lse_t - (Pt * t).sum(axis=1)
    coef = f(g) * f(inv_Ts) / f(N)
    return dict(lse_s=lse_s, lse_t=lse_t, row_loss=row_loss, loss=row_loss.mean(dtype=f), ent=row_ent.mean(dtype=f),
                dq=coef * (Ps @ Q - Pt @ Q))


# ----------------------------------------------------------------------------- inputs
def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def inputs(kind, N, D, K, seed=0):
    """-> q, k (N, D), Q (K, D) fp32.
    easy      unit rows; k_i is a noisy copy of q_i (two views of one clip), Q random.
    hard      rows of norm 2.5; near-copies of the teacher rows are planted in Q (row i at column (7 i + 3) % K while K > i), so
              the teacher's softmax is one-hot to 1e-3 nats at either temperature; q_i is orthogonal to k_i, so the student is NOT
              peaked on the same column and O_s - O_t does not cancel.
    overflow  as hard with rows of norm 3: t reaches 225 at Tt = 0.04, where exp without the max subtraction is inf."""
    rng = np.random.RandomState(1000 * seed + 7 * N + 3 * D + K + {'easy': 0, 'hard': 1, 'overflow': 2}[kind])
    q = _unit(rng.randn(N, D))
    Q = _unit(rng.randn(K, D))
    if kind == 'easy':
        k = _unit(q + 0.5 * _unit(rng.randn(N, D)))
    else:
        k = _unit(rng.randn(N, D))
        q = _unit(q - (q * k).sum(axis=1, keepdims=True) * k)                   # q_i orthogonal to k_i: the student looks elsewhere
        for i in range(min(N, K)):
            Q[(7 * i + 3) % K if K > 7 else i] = _unit((k[i] + 0.02 * _unit(rng.randn(1, D))[0])[None])[0]
        r = 2.5 if kind == 'hard' else 3.0
        q, k, Q = r * q, r * k, r * Q
    return q.astype(np.float32), k.astype(np.float32), Q.astype(np.float32)


def step_inputs(N, D, K, seed=0):
    """q, k, all_k (N, D) and a queue (K, D) of unit rows for the enqueue / graph / module tests."""
    q, k, Q = inputs('easy', N, D, K, seed)
    rng = np.random.RandomState(77 + seed)
    return q, k, k[rng.permutation(N)].copy(), Q


def enqueue(Q, rows, index):
    """RGBMoCo's update: rows at (index + i) % K -> (new queue, new index)."""
    Q = Q.copy()
    K = Q.shape[0]
    for i in range(rows.shape[0]):
        Q[(index + i) % K] = rows[i]
    return Q, (index + rows.shape[0]) % K


# ----------------------------------------------------------------------------- wrong variants
def wrong_variants(q, k, Q, inv_Ts, inv_Tt, g, index=0):
    """name -> dict(loss, dq) of a plausible wrong kernel on the same inputs."""
    N, K = q.shape[0], Q.shape[0]
    out = {}
    out['temperatures swapped'] = ressl(q, k, Q, inv_Tt, inv_Ts, g)
    out['teacher at the student temperature'] = ressl(q, k, Q, inv_Ts, inv_Ts, g)
    out['post-enqueue queue'] = ressl(q, k, enqueue(np.asarray(Q), np.asarray(k), index)[0], inv_Ts, inv_Tt, g)
    r = ressl(q, k, Q, inv_Ts, inv_Tt, g)
    out['1/N missing'] = dict(loss=r['loss'] * N, dq=r['dq'] * N)
    pad = (-K) % 32
    Qp = np.concatenate([np.asarray(Q, dtype=np.float64), np.zeros((pad, Q.shape[1]))])
    out['padded columns scored 0'] = ressl(q, k, Qp, inv_Ts, inv_Tt, g)
    out['gradient scale missing'] = dict(loss=r['loss'], dq=r['dq'] / g)          # (shows in dq alone)
    return out


# ----------------------------------------------------------------------------- dispatch, as csrc/ressl.hip decides it
def _cdiv(a, b):
    return -(-a // b)


def sizes_ok(N, D, K):
    return 1 <= N <= 65536 and D >= 1 and 1 <= K < 2 ** 31 and N * D < 2 ** 31 and K * D < 2 ** 31


def path(N, D, K, aligned=True, sides=1):
    """-> ('fast' | 'generic', waves per workgroup, K-splits, tiles per split).  sides: 1 forward, 2 backward."""
    fast = D <= 256 and D % 4 == 0 and bool(aligned)
    waves = 4 if fast else 1
    kt = _cdiv(K, 32)
    want = min(max(_cdiv(256, _cdiv(N, 32) * sides), 1), _cdiv(kt, waves))
    tps = _cdiv(kt, want)
    return ('fast' if fast else 'generic'), waves, _cdiv(kt, tps), tps
