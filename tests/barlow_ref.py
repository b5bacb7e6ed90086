"""Numpy (fp64) specification of gca_barlow_fwd / gca_barlow_bwd (csrc/barlow.hip): the Barlow Twins loss of two views.

    z1, z2 (N, D): the projector outputs of view 1 / view 2 of the same N clips;  lambda >= 0, eps >= 0
    mean_v[d] = (sum_n z_v[n,d]) / N      var_v[d] = (sum_n (z_v[n,d] - mean_v[d])^2) / N      rstd_v[d] = 1 / sqrt(var_v[d] + eps)
    a = (z1 - mean_1) * rstd_1            b = (z2 - mean_2) * rstd_2
    C[i,j]  = (sum_n a[n,i] * b[n,j]) / N
    on = sum_i (C[i,i] - 1)^2             off = sum_{i != j} C[i,j]^2          loss = on + lambda * off
    G[i,j]  = 2 (C[i,i] - 1) if i == j else 2 lambda C[i,j]
    r1[i]   = sum_j G[i,j] C[i,j]         r2[j] = sum_i G[i,j] C[i,j]
    dz1[n,i] = g * rstd_1[i] / N * (sum_j G[i,j] b[n,j] - a[n,i] r1[i])
    dz2[n,j] = g * rstd_2[j] / N * (sum_i G[i,j] a[n,i] - b[n,j] r2[j])

The kernels have one dispatch path (guarded 4-byte accesses, no alignment assumed), so there is no path rule to restate.
Inputs of the tests live here too, so the CPU tests can assert the properties the GPU tests rely on, next to a few
deliberately wrong variants of the arithmetic that those inputs must tell apart from the right one."""
import numpy as np

EXACT_LAMBDA = 2.0 ** -7
EXACT_CASES = [(2, 1), (2, 4), (8, 32), (16, 64), (16, 128)]                              # (N, D)
FLOAT_CASES = [(5, 1), (5, 33), (8, 32), (33, 130), (64, 128), (40, 512), (256, 512)]
FLOAT_LAMBDAS = (0.0051, 1.0)
MISTAKES = ('unbiased_var', 'lambda_on_diag', 'no_r_term', 'g_transposed')


def barlow(z1, z2, lambd, eps=1e-5, g=1.0, dtype=np.float64, reverse=False, mistake=None):
    """-> dict(stats (4, D), C, on, off, loss, rsum (2, D), dz1, dz2), evaluated in `dtype` from the given values (fp64: the
    specification).  reverse: every sum runs in the opposite order (the exact-input precondition).  mistake: one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES
    f = dtype
    z1, z2 = np.asarray(z1, dtype=f), np.asarray(z2, dtype=f)
    N, D = z1.shape
    if z2.shape != (N, D) or N < 2 or D < 1:
        raise ValueError('two (N, D) views with N >= 2, D >= 1')
    lambd, eps, g, Nf = f(lambd), f(eps), f(g), f(N)
    flip = (lambda x, ax: np.flip(x, axis=ax)) if reverse else (lambda x, ax: x)

    def rsum(x, ax):                     # a plain left-to-right sum along `ax`, in dtype (np.sum's pairwise order is avoided)
        x = np.moveaxis(flip(x, ax), ax, 0)
        s = np.zeros(x.shape[1:], dtype=f)
        for row in x:
            s = (s + row).astype(f)
        return s

    def standardise(z):
        mean = rsum(z, 0) / Nf
        var = rsum((z - mean) ** 2, 0) / (f(N - 1) if mistake == 'unbiased_var' else Nf)
        rstd = f(1) / np.sqrt(var + eps)
        return mean, rstd, ((z - mean) * rstd).astype(f)

    def mm(x, y):                        # x @ y as outer products accumulated left to right (or right to left) along k
        s = np.zeros((x.shape[0], y.shape[1]), dtype=f)
        ks = range(x.shape[1])
        for k in (reversed(ks) if reverse else ks):
            s = (s + x[:, k, None] * y[None, k, :]).astype(f)
        return s

    m1, s1, a = standardise(z1)
    m2, s2, b = standardise(z2)
    C = (mm(a.T, b) / Nf).astype(f)
    eye = np.eye(D, dtype=bool)
    Cd = np.where(eye, C, f(0))
    Co = np.where(eye, f(0), C)
    on = rsum(np.diag((Cd - np.eye(D, dtype=f)) ** 2), 0)
    off = rsum(rsum(Co ** 2, 1), 0)
    diag_w = lambd if mistake == 'lambda_on_diag' else f(1)
    loss = diag_w * on + lambd * off
    G = np.where(eye, f(2) * diag_w * (C - f(1)), f(2) * lambd * C).astype(f)
    r1, r2 = rsum(G * C, 1), rsum(G * C, 0)
    if mistake == 'no_r_term':
        r1, r2 = np.zeros_like(r1), np.zeros_like(r2)
    G1, G2 = (G.T, G.T) if mistake == 'g_transposed' else (G, G)
    y1 = mm(b, G1.T)                                               # [n,i] = sum_j G[i,j] b[n,j]
    y2 = mm(a, G2)                                                 # [n,j] = sum_i G[i,j] a[n,i]
    dz1 = g * s1 / Nf * (y1 - a * r1)
    dz2 = g * s2 / Nf * (y2 - b * r2)
    return dict(stats=np.stack([m1, s1, m2, s2]), C=C, on=f(on), off=f(off), loss=f(loss), rsum=np.stack([r1, r2]),
                dz1=dz1.astype(f), dz2=dz2.astype(f))


def exact_inputs(N, D, seed=0):
    """(z1, z2) fp32 with entries +-1 and as many +1 as -1 in every column (N even): mean = 0 and var = 1 exactly, so with
    eps = 0 a = z1, b = z2, every C[i,j] is k / N and -- N a power of two, lambda = 2^-7 -- every quantity of the loss and
    of its gradient is a dyadic number of few bits, the same in fp32 and fp64 under any order of summation
    (tests/test_barlow_ref.py asserts that at EXACT_CASES).  View 2 is view 1 with, in every second column, one +1 and one
    -1 exchanged (C[i,i] = 1 - 4 / N there; for N = 2 the column is negated)."""
    assert N % 2 == 0
    rng = np.random.RandomState(100 * N + D + seed)
    col = np.array([1.0] * (N // 2) + [-1.0] * (N // 2), dtype=np.float32)
    z1 = np.stack([rng.permutation(col) for _ in range(D)], axis=1)
    z2 = z1.copy()
    for d in range(0, D, 2):
        p, m = np.flatnonzero(z1[:, d] > 0)[0], np.flatnonzero(z1[:, d] < 0)[0]
        z2[p, d], z2[m, d] = -1.0, 1.0
    return np.ascontiguousarray(z1), np.ascontiguousarray(z2)


def float_inputs(N, D, seed=0):
    """(z1, z2) fp32 as a projector produces them in training: D columns with scales spread over about 20x (log-uniform in
    [0.5, 10]) and means of a few units; view 2 is view 1 plus noise of 0.7 of the column's scale, so the diagonal of C is
    near 1 (about 0.82) and the off-diagonal small (about 1 / sqrt(N)).  (With less noise the gradient is the small difference
    b - C_ii a and the fp32 torch chain itself leaves the 3e-6 that tests/test_barlow_ref.py asks of it at 256 x 512.)"""
    rng = np.random.RandomState(31 * N + D + seed)
    scale = np.exp(rng.uniform(np.log(0.5), np.log(10.0), size=(1, D)))
    if D >= 2:
        scale[0, 0], scale[0, -1] = 0.5, 10.0
    mean = rng.uniform(-3.0, 3.0, size=(1, D))
    base = rng.randn(N, D)
    z1 = mean + scale * base
    z2 = mean + 0.5 + scale * (base + 0.7 * rng.randn(N, D))
    return z1.astype(np.float32), z2.astype(np.float32)


def torch_chain(z1, z2, lambd, eps=1e-5):
    """The same loss as a chain of torch ops in the dtype of its inputs (the comparator of tools/barlow_micro.py and the
    precondition of test_barlow_ref.py)."""
    import torch
    import torch.nn.functional as F
    N, D = z1.shape
    a = F.batch_norm(z1, None, None, training=True, eps=eps)
    b = F.batch_norm(z2, None, None, training=True, eps=eps)
    c = (a.t() @ b) / N
    on = (torch.diagonal(c) - 1).pow(2).sum()
    off = c.masked_fill(torch.eye(D, dtype=torch.bool, device=c.device), 0).pow(2).sum()
    return on + lambd * off
