"""The arithmetic of SwAV's swapped-prediction loss (csrc/swav.hip, ops.swav_fwd / swav_bwd, lib.memory.swav.SwAVLoss) in fp64
numpy, the dispatch rule of the kernels, and the seeded inputs and case lists of tests/test_swav_ref.py (CPU) and
tests/test_gpu_swav.py.

    z1, z2 (N, D), C (K, D), all with unit rows;  S_v = z_v C^T
    sinkhorn(S, eps, iters):   Q = exp(S / eps).T;  Q /= Q.sum();  `iters` times: rows of Q to 1 / K, then columns to 1 / N;
                               -> (Q N).T, every row sums to 1.  No gradient flows through it.
    l12 = -mean_n sum_k q2 log_softmax(S1 / T)      l21 = -mean_n sum_k q1 log_softmax(S2 / T)      loss = (l12 + l21) / 2
    dS1 = (softmax(S1 / T) - q2) / (2 N T)          dS2 = (softmax(S2 / T) - q1) / (2 N T)
    dz_v = dS_v C                                   dC = dS1^T z1 + dS2^T z2

`sinkhorn` is the published loop, literally.  `sinkhorn_scaled` is the form the kernels carry -- two scaling vectors u (K) and v
(N) over a fixed P = exp((S - m) / eps) -- and equals it to rounding for any shift m (tests/test_swav_ref.py).

Dispatch: ONE route.  Every shape in the accepted range takes the tiled kernels (64 x 64 MFMA tiles for the three products, one
launch per Sinkhorn pass with both views in its grid); `route` is that rule, a pure function of the sizes, and TILE an edge the
case list has to straddle (N, K and D below, at and above a multiple of 64).  Inside the route one launch count depends on the
sizes: the backward's dz = dS C cuts its reduction over K into `dz_splits(N, D, K)` slabs -- as many as bring its grid to 256
workgroups, at most 32, none shorter than 256 prototypes -- and adds the slabs' partial tiles in a second launch when there is
more than one.  The case list has shapes with one slab and with several, and K on both sides of a slab boundary."""
import numpy as np

DEFAULTS = dict(K=3000, eps=0.05, T=0.1, iters=3)
TILE = 64
ROUTES = ('tiled',)
BAR = 1e-5              # the GPU bar: max-norm error relative to the largest reference entry of each array; the next power of ten
                        # above 4 x the worst error measured on the cases of tests/test_gpu_swav.py (1.87e-6)

# (N, D, K): the smallest shapes that reach each edge -- one element tiles, odd sizes, 64 / 65 on each axis, the workload's
# K = 3000 and D = 128, more than one row block, a tall and a wide one
KERNEL_CASES = [(2, 1, 2), (3, 5, 7), (33, 130, 65), (64, 128, 128), (65, 128, 3000), (256, 128, 1000), (4096, 16, 64), (4, 16, 16384)]
ADVERSARIAL_CASES = [(33, 130, 65), (65, 7, 130)]
ADVERSARIAL_EPS = 0.025


def route(N, D, K):
    """The kernel route for these sizes (ValueError outside the accepted range)."""
    check_sizes(N, D, K)
    return 'tiled'


def dz_splits(N, D, K):
    """Slabs of the reduction over K in the backward's dz product (gca_swav_dz_splits); 1: no second launch."""
    check_sizes(N, D, K)
    tiles = 2 * -(-N // TILE) * -(-D // TILE)
    return min(32, max(1, 256 // tiles), -(-K // 256))


def ws_bytes(N, D, K):
    """gca_swav_ws_bytes: the forward's u (2, K), v (2, N) and row terms (2, N), or the backward's slabs, whichever is larger."""
    s = dz_splits(N, D, K)
    return max((2 * K + 4 * N) * 4, s * 2 * N * D * 4 if s > 1 else 0)


def check_sizes(N, D, K):
    if not (2 <= N <= 8192 and 2 <= K <= 65536 and 1 <= D <= 8192):
        raise ValueError('swav: 2 <= N <= 8192, 2 <= K <= 65536, 1 <= D <= 8192 (got N=%d, K=%d, D=%d)' % (N, K, D))


def check_params(eps, T, iters):
    eps, T = float(eps), float(T)
    if not float(np.float32(0.025)) <= float(np.float32(eps)) <= 1.0:
        raise ValueError('swav: eps must lie in [0.025, 1] (got %r)' % eps)
    if not (T > 0.0 and np.isfinite(T)):
        raise ValueError('swav: T must be positive and finite (got %r)' % T)
    if int(iters) != iters or not 1 <= iters <= 16:
        raise ValueError('swav: iters must lie in [1, 16] (got %r)' % (iters,))
    return eps, T, int(iters)


def rows_normalize(C):
    """C[k,:] / ||C[k,:]||; an all-zero row stays as it is."""
    C = np.asarray(C, dtype=np.float64)
    nrm = np.sqrt((C * C).sum(axis=1, keepdims=True))
    return np.where(nrm > 0, C / np.where(nrm > 0, nrm, 1.0), C)


def sinkhorn(S, eps, iters):
    """The published loop on the (N, K) scores -> the (N, K) codes."""
    S = np.asarray(S, dtype=np.float64)
    N, K = S.shape
    Q = np.exp(S / eps).T
    Q /= Q.sum()
    for _ in range(iters):
        Q /= Q.sum(axis=1, keepdims=True)
        Q /= K
        Q /= Q.sum(axis=0, keepdims=True)
        Q /= N
    return (Q * N).T


def sinkhorn_scaled(S, eps, iters, shift=None):
    """The same codes as two scaling vectors over P = exp((S - shift) / eps), which is never rewritten (shift: the maximum of S
    by default; the kernels use the bound 1 of unit rows)."""
    S = np.asarray(S, dtype=np.float64)
    N, K = S.shape
    P = np.exp((S - (S.max() if shift is None else shift)) / eps)
    v = np.ones(N)
    for _ in range(iters):
        u = 1.0 / (K * (P * v[:, None]).sum(axis=0))
        v = 1.0 / (N * (P * u[None, :]).sum(axis=1))
    return N * P * u[None, :] * v[:, None]


def log_softmax(X):
    m = X.max(axis=1, keepdims=True)
    return X - m - np.log(np.exp(X - m).sum(axis=1, keepdims=True))


def loss_parts(z1, z2, C, eps=DEFAULTS['eps'], T=DEFAULTS['T'], iters=DEFAULTS['iters']):
    """-> dict(loss, l12, l21, q1, q2, S1, S2) in fp64."""
    z1, z2, C = (np.asarray(a, dtype=np.float64) for a in (z1, z2, C))
    if z1.ndim != 2 or z1.shape != z2.shape or C.ndim != 2 or C.shape[1] != z1.shape[1]:
        raise ValueError('swav: two (N, D) views and (K, D) prototypes expected')
    check_sizes(z1.shape[0], z1.shape[1], C.shape[0])
    eps, T, iters = check_params(eps, T, iters)
    N = z1.shape[0]
    S1, S2 = z1 @ C.T, z2 @ C.T
    q1, q2 = sinkhorn(S1, eps, iters), sinkhorn(S2, eps, iters)
    l12 = -(q2 * log_softmax(S1 / T)).sum() / N
    l21 = -(q1 * log_softmax(S2 / T)).sum() / N
    return dict(loss=0.5 * (l12 + l21), l12=l12, l21=l21, q1=q1, q2=q2, S1=S1, S2=S2)


def grads(z1, z2, C, eps=DEFAULTS['eps'], T=DEFAULTS['T'], iters=DEFAULTS['iters'], g=1.0):
    """loss_parts plus dS1, dS2, dz1, dz2, dC of g * loss."""
    out = loss_parts(z1, z2, C, eps, T, iters)
    z1, z2, C = (np.asarray(a, dtype=np.float64) for a in (z1, z2, C))
    N, T = z1.shape[0], float(T)
    out['dS1'] = g * (np.exp(log_softmax(out['S1'] / T)) - out['q2']) / (2.0 * N * T)
    out['dS2'] = g * (np.exp(log_softmax(out['S2'] / T)) - out['q1']) / (2.0 * N * T)
    out['dz1'], out['dz2'] = out['dS1'] @ C, out['dS2'] @ C
    out['dC'] = out['dS1'].T @ z1 + out['dS2'].T @ z2
    out['codes'] = np.stack([out['q1'], out['q2']])
    return out


# ----------------------------------------------------------------------------- the same arithmetic as a chain of torch ops
def torch_sinkhorn(S, eps, iters):
    """The published loop, transcribed op for op."""
    import torch
    N, K = S.shape
    Q = torch.exp(S / eps).t()
    Q = Q / Q.sum()
    for _ in range(iters):
        Q = Q / Q.sum(dim=1, keepdim=True)
        Q = Q / K
        Q = Q / Q.sum(dim=0, keepdim=True)
        Q = Q / N
    return (Q * N).t()


def torch_chain(z1, z2, C, eps=DEFAULTS['eps'], T=DEFAULTS['T'], iters=DEFAULTS['iters'], swapped=True, codes='sinkhorn',
                use_T=True, detach=True):
    """-> (loss, l12, l21) as differentiable torch scalars.  The keyword arguments switch on the wrong variants that
    tests/test_swav_ref.py holds the specification apart from: un-swapped codes, a row softmax of S / eps for the codes, a
    missing 1 / T, codes that carry gradient."""
    import torch
    S1, S2 = z1 @ C.t(), z2 @ C.t()
    if codes == 'sinkhorn':
        q1, q2 = torch_sinkhorn(S1, eps, iters), torch_sinkhorn(S2, eps, iters)
    else:
        q1, q2 = torch.softmax(S1 / eps, dim=1), torch.softmax(S2 / eps, dim=1)
    if detach:
        q1, q2 = q1.detach(), q2.detach()
    if not swapped:
        q1, q2 = q2, q1
    t = T if use_T else 1.0
    l12 = -(q2 * torch.log_softmax(S1 / t, dim=1)).sum(dim=1).mean()
    l21 = -(q1 * torch.log_softmax(S2 / t, dim=1)).sum(dim=1).mean()
    return 0.5 * (l12 + l21), l12, l21


# ----------------------------------------------------------------------------- inputs
def _unit(a):
    return a / np.sqrt((a * a).sum(axis=1, keepdims=True))


def unit_inputs(N, D, K, seed=0):
    """Seeded fp32 (z1, z2, C) with unit rows (to fp32 rounding): view 2 is view 1 plus noise of its own size, renormalised, so
    the two views' codes differ; the prototypes are independent directions.

    D = 1 leaves only +-1 for every row, and a random draw of signs can separate the rows perfectly: every code then sits on
    its row's top score, the loss is log(1 + exp(-2 / T)) = 2e-9 -- the residue of terms of size 1 / T = 10 cancelling, below what
    any fp32 evaluation of those terms resolves -- and softmax - q is a residue of the same kind.  A relative error against such
    a reference measures nothing, so for D = 1 the signs are set, not drawn: view 1 all +1 (equal rows, uniform codes), view 2 and
    the prototypes alternating (separated rows, one-hot codes), which leaves the loss at about 1 / T and the gradients at their
    full size (tests/test_swav_ref.py holds every case to that)."""
    if D == 1:
        alt = (1.0 - 2.0 * (np.arange(max(N, K)) % 2)).astype(np.float32)[:, None]
        return np.ones((N, 1), dtype=np.float32), np.ascontiguousarray(alt[:N]), np.ascontiguousarray(alt[:K])
    rng = np.random.RandomState(1000003 * seed + 7919 * N + 131 * D + K)
    a = rng.randn(N, D)
    z1 = _unit(a)
    z2 = _unit(a + rng.randn(N, D))
    C = _unit(rng.randn(K, D))
    return tuple(np.ascontiguousarray(x.astype(np.float32)) for x in (z1, z2, C))


def equal_scores_inputs(N, D, K):
    """Every score is -1, the far end of what unit rows allow: with the bound 1 as the shift every entry of P is
    exp(-2 / eps), the smallest the kernel can meet.  The codes are uniform, 1 / K, and the loss is log K."""
    z = np.zeros((N, D), dtype=np.float32)
    z[:, 0] = 1.0
    C = np.zeros((K, D), dtype=np.float32)
    C[:, 0] = -1.0
    return z, z.copy(), C


def one_hot_scores_inputs(N, D, K):
    """Prototype 0 scores 1 against every row and all others score -1: (max - min) / eps = 2 / eps inside every row and every
    column sum differs by exp(2 / eps) from its neighbour's.  Sinkhorn still equalises the columns: uniform codes."""
    z, _, C = equal_scores_inputs(N, D, K)
    C[0, 0] = 1.0
    return z, z.copy(), C
