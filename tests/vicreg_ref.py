"""Numpy (fp64) specification of gca_vicreg_fwd / gca_vicreg_bwd (csrc/vicreg.hip): the VICReg loss of two views.

    z1, z2 (N, D): the projector outputs of view 1 / view 2 of the same N clips;  sim, std, cov, eps >= 0.  Per view v, x = z_v:
    mean_v[d] = (sum_n x[n,d]) / N        xc = x - mean_v
    var_v[d]  = (sum_n xc[n,d]^2) / (N - 1)       sd_v[d] = sqrt(var_v[d] + eps)            (unbiased; eps inside the root)
    Cov_v[i,j] = (sum_n xc[n,i] xc[n,j]) / (N - 1)
    inv  = sum_{n,d} (z1 - z2)^2 / (N D)
    varl = sum_v sum_d max(0, 1 - sd_v[d]) / (2 D)
    covl = sum_v sum_{i != j} Cov_v[i,j]^2 / D
    loss = sim * inv + std * varl + cov * covl
    dz_v[n,j] = g * (s_v * 2 sim (z1 - z2)[n,j] / (N D) - std * [sd_v[j] < 1] * xc[n,j] / (2 D sd_v[j] (N - 1))
                     + cov * 4 / (D (N - 1)) * sum_{i != j} xc[n,i] Cov_v[i,j]),          s_1 = +1, s_2 = -1

The centring contributes no extra term: the columns of xc sum to zero, so the variance and the covariance gradient already have
zero column means.  With eps = 0 a constant column gives sd = 0 and 0 / 0 in its gradient, as the chain of torch ops does.
The kernels have one dispatch path (guarded 4-byte accesses, no alignment assumed), so there is no path rule to restate.
Inputs of the tests live here too, so the CPU tests can assert the properties the GPU tests rely on, next to a few
deliberately wrong variants of the arithmetic that those inputs must tell apart from the right one."""
import numpy as np

DEFAULTS = dict(sim=25.0, std=25.0, cov=1.0, eps=1e-4)
EXACT_COEFFS = (0.0, 16.0, 1.0)                                                           # sim, std, cov
EXACT_CASES = [(3, 1), (3, 4), (5, 2), (9, 32), (17, 64), (9, 128), (17, 128), (33, 128)]  # (N, D), N = 2^k + 1
FLOAT_CASES = [(5, 1), (5, 33), (8, 32), (33, 130), (64, 128), (40, 512), (256, 512)]
FLOAT_COEFFS = ((25.0, 25.0, 1.0), (1.0, 0.0, 4.0))
MISTAKES = ('biased_var', 'cov_by_n', 'diag_in_cov', 'no_hinge', 'hinge_not_halved', 'inv_sum_not_mean', 'eps_outside_root')


def vicreg(z1, z2, sim=25.0, std=25.0, cov=1.0, eps=1e-4, g=1.0, dtype=np.float64, reverse=False, mistake=None):
    """-> dict(stats (4, D) = mean_1, sd_1, mean_2, sd_2; covm (2, D, D); loss, inv, varl, covl; dz1, dz2), evaluated in `dtype`
    from the given values (fp64: the specification).  reverse: every sum runs in the opposite order (the exact-input
    precondition).  mistake: one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES
    f = dtype
    z1, z2 = np.asarray(z1, dtype=f), np.asarray(z2, dtype=f)
    if z1.ndim != 2 or z2.shape != z1.shape or z1.shape[0] < 2 or z1.shape[1] < 1:
        raise ValueError('two (N, D) views with N >= 2, D >= 1')
    N, D = z1.shape
    for name, val in (('sim', sim), ('std', std), ('cov', cov), ('eps', eps)):
        if not 0.0 <= float(val) < float('inf'):
            raise ValueError('%s must be non-negative and finite' % name)
    sim, std, cov, eps, g, Nf, Df = f(sim), f(std), f(cov), f(eps), f(g), f(N), f(D)
    N1 = f(N - 1)
    flip = (lambda x, ax: np.flip(x, axis=ax)) if reverse else (lambda x, ax: x)

    def rsum(x, ax):                     # a plain left-to-right sum along `ax`, in dtype (np.sum's pairwise order is avoided)
        x = np.moveaxis(flip(x, ax), ax, 0)
        s = np.zeros(x.shape[1:], dtype=f)
        for row in x:
            s = (s + row).astype(f)
        return s

    def mm(x, y):                        # x @ y as outer products accumulated left to right (or right to left) along k
        s = np.zeros((x.shape[0], y.shape[1]), dtype=f)
        ks = range(x.shape[1])
        for k in (reversed(ks) if reverse else ks):
            s = (s + x[:, k, None] * y[None, k, :]).astype(f)
        return s

    eye = np.eye(D, dtype=bool)
    diff = (z1 - z2).astype(f)
    inv = rsum(rsum(diff ** 2, 0), 0) / (f(1) if mistake == 'inv_sum_not_mean' else Nf * Df)
    cinv = f(2) * sim / (f(1) if mistake == 'inv_sum_not_mean' else Nf * Df)
    hdiv = Df if mistake == 'hinge_not_halved' else f(2) * Df
    stats, covm, dz = [], [], []
    varl, covl = f(0), f(0)
    for sign, x in ((f(1), z1), (f(-1), z2)):
        mean = rsum(x, 0) / Nf
        xc = (x - mean).astype(f)
        var = rsum(xc ** 2, 0) / (Nf if mistake == 'biased_var' else N1)
        sd = (np.sqrt(var) + eps if mistake == 'eps_outside_root' else np.sqrt(var + eps)).astype(f)
        C = (mm(xc.T, xc) / (Nf if mistake == 'cov_by_n' else N1)).astype(f)
        Co = C if mistake == 'diag_in_cov' else np.where(eye, f(0), C)
        active = np.zeros_like(sd, dtype=bool) if mistake == 'no_hinge' else sd < f(1)
        varl = varl + rsum(np.where(active, f(1) - sd, f(0)), 0) / hdiv
        covl = covl + rsum(rsum(Co ** 2, 1), 0) / Df
        with np.errstate(invalid='ignore', divide='ignore'):
            hinge = np.where(active, (std / (hdiv * N1)) * xc / sd, f(0))
        grad = sign * cinv * diff - hinge + (f(4) * cov / (Df * (Nf if mistake == 'cov_by_n' else N1))) * mm(xc, Co)
        stats += [mean, sd]
        covm.append(C)
        dz.append((g * grad).astype(f))
    loss = sim * inv + std * varl + cov * covl
    return dict(stats=np.stack(stats).astype(f), covm=np.stack(covm), loss=f(loss), inv=f(inv), varl=f(varl), covl=f(covl),
                dz1=dz[0], dz2=dz[1])


def exact_inputs(N, D, seed=0):
    """(z1, z2) fp32, N = 2^k + 1: every column holds 2^(k-1) entries of +1/2, 2^(k-1) of -1/2 and one 0 in a permuted order, so
    mean = 0, var = 1/4 and -- with eps = 0 -- sd = 1/2 exactly (the hinge is active) and every Cov[i,j] is m / 2^(k+2).  With
    sim = 0, std = 16, cov = 1 and D a power of two every quantity of the loss and of its gradient is a dyadic number of few
    bits, the same in fp32 and fp64 under any order of summation (tests/test_vicreg_ref.py asserts that at EXACT_CASES); `inv`
    alone, a division by N D with N odd, is only the correctly rounded quotient in either precision.  View 2 is view 1 with, in
    every second column, one +1/2 and one -1/2 exchanged."""
    assert N >= 3 and (N - 1) & (N - 2) == 0
    rng = np.random.RandomState(100 * N + D + seed)
    h = (N - 1) // 2
    col = np.array([0.5] * h + [-0.5] * h + [0.0], dtype=np.float32)
    z1 = np.stack([rng.permutation(col) for _ in range(D)], axis=1)
    z2 = z1.copy()
    for d in range(0, D, 2):
        p, m = np.flatnonzero(z1[:, d] > 0)[0], np.flatnonzero(z1[:, d] < 0)[0]
        z2[p, d], z2[m, d] = -0.5, 0.5
    return np.ascontiguousarray(z1), np.ascontiguousarray(z2)


def column_scales(D):
    """The standard deviations the float inputs aim at: alternately below 1 (0.3 .. 0.7: hinge active) and above it (1.5 .. 4),
    and 0.02 in column 0; all far enough from 1 that the sample value of no column comes within 1e-3 of it (asserted by tests/test_vicreg_ref.py)."""
    t = (np.arange(D) * 0.6180339887) % 1.0
    s = np.where(np.arange(D) % 2 == 0, 0.3 + 0.4 * t, 1.5 + 2.5 * t)
    s[0] = 0.02                          # one nearly collapsed column: var = 4e-4 is of the order of eps, so where eps sits shows
    return s


def float_inputs(N, D, seed=0):
    """(z1, z2) fp32 as a projector produces them in training, built as barlow_ref.float_inputs: means of a few units, view 2 a
    noisy copy of view 1 (noise 0.7 of the column's scale).  Each column is rescaled to the sample standard deviation of
    column_scales(D) in both views, so some hinges are active and some are not, and fp32 and fp64 take the same branch.  The
    last column (D >= 3) is constant in both views: sd = sqrt(eps) there and its hinge gradient is xc / sd = 0."""
    rng = np.random.RandomState(31 * N + D + seed)
    scale = column_scales(D)[None, :]
    mean = rng.uniform(-3.0, 3.0, size=(1, D))
    base = rng.randn(N, D)
    other = base + 0.7 * rng.randn(N, D)
    unit = lambda x: (x - x.mean(axis=0)) / x.std(axis=0, ddof=1)
    z1 = mean + scale * unit(base)
    z2 = mean + 0.5 + scale * unit(other)
    if D >= 3:
        z1[:, -1], z2[:, -1] = 1.25, -0.75
    return z1.astype(np.float32), z2.astype(np.float32)


def torch_chain(z1, z2, sim=25.0, std=25.0, cov=1.0, eps=1e-4):
    """The published loss as a chain of torch ops in the dtype of its inputs (the comparator of tools/vicreg_micro.py and the
    precondition of test_vicreg_ref.py) -> (loss, inv, varl, covl)."""
    import torch
    import torch.nn.functional as F
    N, D = z1.shape
    inv = F.mse_loss(z1, z2)
    x, y = z1 - z1.mean(dim=0), z2 - z2.mean(dim=0)
    sx, sy = torch.sqrt(x.var(dim=0) + eps), torch.sqrt(y.var(dim=0) + eps)
    varl = torch.mean(F.relu(1 - sx)) / 2 + torch.mean(F.relu(1 - sy)) / 2
    cx, cy = (x.T @ x) / (N - 1), (y.T @ y) / (N - 1)
    eye = torch.eye(D, dtype=torch.bool, device=z1.device)
    covl = cx.masked_fill(eye, 0).pow(2).sum() / D + cy.masked_fill(eye, 0).pow(2).sum() / D
    return sim * inv + std * varl + cov * covl, inv, varl, covl
