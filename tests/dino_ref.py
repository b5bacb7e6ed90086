"""The arithmetic of DINO's centred-teacher self-distillation loss (csrc/dino.hip, ops.dino_fwd / dino_bwd,
lib.memory.dino.DINOLoss) in fp64 numpy, and the seeded inputs and case lists of tests/test_dino_ref.py (CPU) and
tests/test_gpu_dino.py.

    student zs1, zs2 (N, D), Cs (K, D); teacher zt1, zt2 (N, D), Ct (K, D); all with unit rows; the centre c (K)
    Ss_v = zs_v Cs^T            St_v = zt_v Ct^T
    p_v  = softmax((St_v - c) / Tt)        (rows; no gradient)
    ls_v = log_softmax(Ss_v / Ts)          (formed as Ss / Ts - lse, never as log(softmax))
    l12  = -(1/N) sum_{n,k} p_1 ls_2       l21 = -(1/N) sum_{n,k} p_2 ls_1       loss = (l12 + l21) / 2
    ent  = -(1/(2N)) sum_{v,n,k} p_v ((St_v - c) / Tt - lse_t)                   (the mean teacher entropy)
    dSs_2 = (softmax(Ss_2 / Ts) - p_1) / (2 N Ts)       dSs_1 = (softmax(Ss_1 / Ts) - p_2) / (2 N Ts)
    dz_v = dSs_v Cs                        dC = dSs_1^T zs_1 + dSs_2^T zs_2
    c'   = cm c + (1 - cm) (1/(2N)) sum_{v,n} St_v[n,:]       AFTER the loss has used c

Dispatch: ONE route, 64 x 64 MFMA tiles for the scores and one 256-thread workgroup per row and direction; the case list
straddles the tile edge on every axis and the workgroup's stride of 256 along K."""
import numpy as np

DEFAULTS = dict(K=4096, Ts=0.1, Tt=0.04, cm=0.9)
TILE = 64
ROW_STRIDE = 256
BAR = 1e-5              # the GPU bar: max-norm error relative to the largest reference entry of each array; the next power of ten
                        # above 4 x the worst error measured on the cases of tests/test_gpu_dino.py (2.45e-6), and no more than
                        # 1e-4

# (N, D, K): one-element tiles, odd sizes, 64 / 65 on every axis, D across the staging chunk, K across a workgroup's stride,
# both range ends of K
KERNEL_CASES = [(2, 1, 2), (3, 5, 7), (33, 130, 65), (64, 128, 128), (65, 128, 3000), (256, 128, 1000), (4096, 16, 64),
                (4, 16, 16384), (2, 8, 65536)]
TEMPERATURE_CASES = [(33, 130, 65), (65, 128, 3000)]
TEMPERATURES = [(0.1, 0.07), (0.5, 0.02)]                  # (Ts, Tt) next to the default (0.1, 0.04)
ADVERSARIAL_CASES = [(33, 130, 65), (65, 7, 300)]
CENTER_SIZE = 0.1


def check_sizes(N, D, K):
    if not (2 <= N <= 8192 and 2 <= K <= 65536 and 1 <= D <= 8192):
        raise ValueError('dino: 2 <= N <= 8192, 2 <= K <= 65536, 1 <= D <= 8192 (got N=%d, K=%d, D=%d)' % (N, K, D))


def check_params(Ts, Tt, cm):
    Ts, Tt, cm = float(Ts), float(Tt), float(cm)
    for name, T in (('Ts', Ts), ('Tt', Tt)):
        if not (T > 0.0 and np.isfinite(T)):
            raise ValueError('dino: %s must be positive and finite (got %r)' % (name, T))
    if not 0.0 <= cm < 1.0:
        raise ValueError('dino: cm must lie in [0, 1) (got %r)' % cm)
    return Ts, Tt, cm


def ws_bytes(N, D, K):
    """gca_dino_ws_bytes: the teacher scores (2, N, K) and the row terms (4, N)."""
    check_sizes(N, D, K)
    return (2 * N * K + 4 * N) * 4


def log_softmax(X):
    m = X.max(axis=1, keepdims=True)
    return X - m - np.log(np.exp(X - m).sum(axis=1, keepdims=True))


def forward(zs1, zs2, Cs, zt1, zt2, Ct, c, Ts=DEFAULTS['Ts'], Tt=DEFAULTS['Tt'], cm=DEFAULTS['cm'], g=1.0):
    """-> dict(loss, l12, l21, ent, probs (2, N, K), dS1, dS2, dz1, dz2, dC of g * loss, center: the centre after the step)."""
    zs1, zs2, Cs, zt1, zt2, Ct, c = (np.asarray(a, dtype=np.float64) for a in (zs1, zs2, Cs, zt1, zt2, Ct, c))
    if zs1.ndim != 2 or Cs.ndim != 2 or Cs.shape[1] != zs1.shape[1]:
        raise ValueError('dino: (N, D) views and (K, D) prototypes expected')
    if not (zs2.shape == zt1.shape == zt2.shape == zs1.shape and Ct.shape == Cs.shape and c.shape == (Cs.shape[0],)):
        raise ValueError('dino: the two views, the teacher operands and the centre must match the student shapes')
    check_sizes(zs1.shape[0], zs1.shape[1], Cs.shape[0])
    Ts, Tt, cm = check_params(Ts, Tt, cm)
    N = zs1.shape[0]
    Ss1, Ss2, St1, St2 = zs1 @ Cs.T, zs2 @ Cs.T, zt1 @ Ct.T, zt2 @ Ct.T
    lp1, lp2 = log_softmax((St1 - c) / Tt), log_softmax((St2 - c) / Tt)
    p1, p2 = np.exp(lp1), np.exp(lp2)
    ls1, ls2 = log_softmax(Ss1 / Ts), log_softmax(Ss2 / Ts)
    l12 = -(p1 * ls2).sum() / N
    l21 = -(p2 * ls1).sum() / N
    out = dict(loss=0.5 * (l12 + l21), l12=l12, l21=l21, ent=-((p1 * lp1).sum() + (p2 * lp2).sum()) / (2.0 * N))
    out['probs'] = np.stack([p1, p2])
    out['dS1'] = g * (np.exp(ls1) - p2) / (2.0 * N * Ts)
    out['dS2'] = g * (np.exp(ls2) - p1) / (2.0 * N * Ts)
    out['dz1'], out['dz2'] = out['dS1'] @ Cs, out['dS2'] @ Cs
    out['dC'] = out['dS1'].T @ zs1 + out['dS2'].T @ zs2
    out['center'] = cm * c + (1.0 - cm) * (St1.sum(axis=0) + St2.sum(axis=0)) / (2.0 * N)
    return out


def ema(p_ema, p, m):
    """The teacher's update, as the reference's _momentum_update writes it: p_ema m + (1 - m) p."""
    return np.asarray(p_ema, dtype=np.float64) * m + (1.0 - m) * np.asarray(p, dtype=np.float64)


# ----------------------------------------------------------------------------- the same arithmetic as a chain of torch ops
def torch_chain(zs1, zs2, Cs, zt1, zt2, Ct, c, Ts=DEFAULTS['Ts'], Tt=DEFAULTS['Tt'], cm=DEFAULTS['cm'], centring='teacher',
                center_first=False, swap_temperatures=False, cross=True, half=True):
    """-> (loss, l12, l21, ent, new centre), the loss differentiable.  The keyword arguments switch on the wrong variants that
    tests/test_dino_ref.py holds the specification apart from: no centring ('none') or the centre applied to the student
    ('student'), the centre updated before it is used, the two temperatures swapped, same-view pairs, a missing 1 / 2."""
    import torch
    Ss1, Ss2 = zs1 @ Cs.t(), zs2 @ Cs.t()
    with torch.no_grad():
        St1, St2 = zt1 @ Ct.t(), zt2 @ Ct.t()
        new_c = cm * c + (1.0 - cm) * torch.cat([St1, St2]).mean(dim=0)
        use = new_c if center_first else c
        tt, ts = (Ts, Tt) if swap_temperatures else (Tt, Ts)
        shift = use if centring == 'teacher' else 0.0
        lp1, lp2 = torch.log_softmax((St1 - shift) / tt, dim=1), torch.log_softmax((St2 - shift) / tt, dim=1)
        p1, p2 = lp1.exp(), lp2.exp()
        ent = -0.5 * ((p1 * lp1).sum(dim=1).mean() + (p2 * lp2).sum(dim=1).mean())
    if centring == 'student':
        Ss1, Ss2 = Ss1 - use, Ss2 - use
    ls1, ls2 = torch.log_softmax(Ss1 / ts, dim=1), torch.log_softmax(Ss2 / ts, dim=1)
    if not cross:
        ls1, ls2 = ls2, ls1
    l12 = -(p1 * ls2).sum(dim=1).mean()
    l21 = -(p2 * ls1).sum(dim=1).mean()
    return (0.5 if half else 1.0) * (l12 + l21), l12, l21, ent, new_c


# ----------------------------------------------------------------------------- inputs
def _unit(a):
    return a / np.sqrt((a * a).sum(axis=1, keepdims=True))


def unit_inputs(N, D, K, seed=0):
    """Seeded fp32 (zs1, zs2, Cs, zt1, zt2, Ct, c): the student operands are SwAV's seeded unit rows (view 2 is view 1 plus noise
    of its own size, renormalised), the teacher's are perturbed copies of them (noise of a quarter of their size, renormalised:
    a teacher that trails its student), and the centre is a random vector of size CENTER_SIZE -- never zero, since a zero
    centre hides a missing or misplaced centring.

    D = 1 leaves only +-1 for every row; the signs are set, not drawn, as in tests/swav_ref.py: view 1 all +1, view 2 and the
    prototypes alternating, the teacher equal to the student."""
    rng = np.random.RandomState(1000003 * seed + 7919 * N + 131 * D + K)
    if D == 1:
        alt = (1.0 - 2.0 * (np.arange(max(N, K)) % 2))[:, None]
        zs1, zs2, Cs = np.ones((N, 1)), alt[:N], alt[:K]
        zt1, zt2, Ct = zs1, zs2, Cs
    else:
        a = rng.randn(N, D)
        zs1 = _unit(a)
        zs2 = _unit(a + rng.randn(N, D))
        Cs = _unit(rng.randn(K, D))
        zt1 = _unit(zs1 + 0.25 * _unit(rng.randn(N, D)))
        zt2 = _unit(zs2 + 0.25 * _unit(rng.randn(N, D)))
        Ct = _unit(Cs + 0.25 * _unit(rng.randn(K, D)))
    c = CENTER_SIZE * rng.randn(K)
    return tuple(np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32)) for x in (zs1, zs2, Cs, zt1, zt2, Ct, c))


def equal_scores_inputs(N, D, K):
    """Every teacher score and every student score is -1 and the centre is constant: the teacher's probabilities are uniform,
    ent = log K and loss = log K."""
    z = np.zeros((N, D), dtype=np.float32)
    z[:, 0] = 1.0
    C = np.zeros((K, D), dtype=np.float32)
    C[:, 0] = -1.0
    c = np.full(K, 0.25, dtype=np.float32)
    return z, z.copy(), C, z.copy(), z.copy(), C.copy(), c


def one_hot_scores_inputs(N, D, K):
    """Prototype 0 scores +1 against every row and all others -1, centre zero: at Tt = 0.04 the teacher's probabilities outside
    prototype 0 are exp(-50), about 2e-22 -- normal fp32 numbers -- and the entropy is about 50 K exp(-50)."""
    z, _, C, _, _, _, _ = equal_scores_inputs(N, D, K)
    C[0, 0] = 1.0
    return z, z.copy(), C, z.copy(), z.copy(), C.copy(), np.zeros(K, dtype=np.float32)
