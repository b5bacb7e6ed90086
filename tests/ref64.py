"""Plain fp64 references of the non-convolution kernels, and the seeded edge-case inputs shared by the CPU
precondition tests (tests/test_ref64.py) and the GPU tests (tests/test_gpu_edges.py).

Every reference takes the fp32 (or fp16) tensors a kernel takes, widens them to fp64 on the CPU and does the operation
the obvious way: no tiling, no online rescaling, two-pass variance.  tests/test_ref64.py holds each of them to ATen /
the oracle package at 1e-12, so that a disagreement on the GPU is the kernel's.
"""
import math

import torch

F64 = torch.float64
EPS32 = float(torch.finfo(torch.float32).eps)           # 2^-23: clamp_probs' bound for fp32 probabilities
U32 = 2.0 ** -24                                        # unit roundoff of fp32 (one rounding to nearest)


def d(t):
    """fp64 CPU copy of a tensor (None passes through)."""
    return None if t is None else t.detach().to('cpu', F64)


def f32(v):
    """The value a Python float has after crossing the C ABI as a `float` argument."""
    return float(torch.tensor(v, dtype=torch.float32))


def rel(a, b):
    """max|a - b| / max|b|, the suite's relative measure (conftest.rel_err), in fp64."""
    a, b = d(a), d(b)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ----------------------------------------------------------------------------- InfoNCE / MoCo queue
def snapshot(queue, ov_start=0, ov_rows=None):
    """The pre-enqueue queue: rows [ov_start, ov_start + n) mod K of `queue` replaced by the saved rows `ov_rows`."""
    qu = d(queue).clone()
    if ov_rows is not None and ov_rows.shape[0]:
        ids = (torch.arange(ov_rows.shape[0]) + int(ov_start)) % qu.shape[0]
        qu[ids] = d(ov_rows)
    return qu


def infonce_bwd(logits, k, queue, inv_T, ov_start=0, ov_rows=None, gscale=1.0):
    """dq of loss = gscale * mean_i(lse_i - logits[i, 0]) given the logits, against the pre-enqueue snapshot."""
    lg, k, qu = d(logits), d(k), snapshot(queue, ov_start, ov_rows)
    g = torch.softmax(lg, dim=1)
    g[:, 0] -= 1.0
    g *= gscale / lg.shape[0]
    return (g[:, :1] * k + g[:, 1:] @ qu) * inv_T


def infonce(q, k, queue, inv_T, ov_start=0, ov_rows=None, gscale=1.0):
    """-> dict(logits (b, K+1), lse (b), loss (), rank (b) int64, dq (b, D)).  `queue` is the queue as the backward sees it;
    the logits and everything after them use the pre-enqueue snapshot (see `snapshot`)."""
    q, k, qu = d(q), d(k), snapshot(queue, ov_start, ov_rows)
    logits = torch.cat(((q * k).sum(1, keepdim=True), q @ qu.t()), dim=1) * inv_T
    lse = torch.logsumexp(logits, dim=1)
    return dict(logits=logits, lse=lse, loss=(lse - logits[:, 0]).mean(),
                rank=(logits[:, 1:] >= logits[:, :1]).sum(1),
                dq=infonce_bwd(logits, k, qu, inv_T, gscale=gscale))


def nce_dlogits(logits, gscale=1.0):
    lg = d(logits)
    g = torch.softmax(lg, dim=1)
    g[:, 0] -= 1.0
    return g * (gscale / lg.shape[0])


def rank_ge(output, target):
    """Number of columns j != target[i] with output[i, j] >= output[i, target[i]]."""
    o, t = d(output), target.detach().cpu().long()
    ref = o.gather(1, t[:, None])
    return (o >= ref).sum(1) - 1


# ----------------------------------------------------------------------------- temporal-graph block
def hop_weights(T, max_hop, alpha):
    """(T, T) matrix theta(|i - j|) inside the hop band, 0 outside (oracle.graph.hop_distance / theta)."""
    from oracle.graph import hop_distance, theta
    hop = hop_distance(T, max_hop)
    w = torch.zeros(T, T, dtype=F64)
    for h in range(min(int(max_hop), T - 1) + 1):
        w[hop == h] = theta(h, alpha)
    return w


def rsample(pre, u, temperature, eps=EPS32):
    """RelaxedBernoulli(temperature, probs=pre).rsample() with explicit uniforms, clamped at `eps` / 1 - eps as
    clamp_probs does for fp32 tensors (the kernels and the fp32 oracle clamp there; the default is that bound)."""
    p = pre.clamp(min=eps, max=1 - eps)
    uu = u.clamp(min=eps, max=1 - eps)
    return torch.sigmoid((uu.log() - (-uu).log1p() + p.log() - (-p).log1p()) / temperature)


def graph_adj(gq, gk, u, max_hop, alpha, temperature, dadj=None, eps=EPS32):
    """gq / gk (B, Ci, T, ...) -> dict(sim, pre, adj [, dgq, dgk by autograd for the upstream gradient dadj])."""
    B, Ci, T = gq.shape[:3]
    a = d(gq).reshape(B, Ci, T, -1).requires_grad_(dadj is not None)
    b = d(gk).reshape(B, Ci, T, -1).requires_grad_(dadj is not None)
    sim = torch.softmax(torch.einsum('bcip,bcjp->bij', a, b), dim=-1)
    pre = sim * hop_weights(T, max_hop, alpha)
    adj = rsample(pre, d(u), temperature, eps)
    out = dict(sim=sim.detach(), pre=pre.detach(), adj=adj.detach())
    if dadj is not None:
        adj.backward(d(dadj))
        out['dgq'], out['dgk'] = a.grad.reshape(gq.shape), b.grad.reshape(gk.shape)
    return out


def graph_adj_bwd_saved(dadj, gq, gk, sim, pre, adj, max_hop, alpha, temperature, eps=EPS32):
    """The backward from SAVED sim / pre / adj, as the ABI takes them.  adj = sigmoid(L), L = (logit(u) + logit(clamp(pre))) / T:
    the sigmoid's derivative adj (1 - adj) comes from the saved sample, dL / dpre by autograd through torch.clamp (which
    passes the gradient at pre == bound and blocks it beyond; u drops out), then the hop weights and the softmax by hand.
    -> dict(dpre, dS, dgq, dgk)."""
    B, Ci, T = gq.shape[:3]
    a, b, s, sample = d(gq).reshape(B, Ci, T, -1), d(gk).reshape(B, Ci, T, -1), d(sim), d(adj)
    p = d(pre).requires_grad_(True)
    pc = p.clamp(min=eps, max=1 - eps)
    ((pc.log() - (-pc).log1p()) / temperature).backward(d(dadj) * sample * (1 - sample))
    w = hop_weights(T, max_hop, alpha)
    ds = p.grad * w
    dS = s * (ds - (ds * s).sum(-1, keepdim=True))
    return dict(dpre=p.grad * (w != 0), dS=dS, dgq=torch.einsum('bij,bcjp->bcip', dS, b).reshape(gq.shape),
                dgk=torch.einsum('bij,bcip->bcjp', dS, a).reshape(gk.shape))


def graph_gcn(adj, s, dout=None):
    """out = einsum('bij,bcjp->bcip', adj, s) + s [, ds, dadj for the upstream gradient dout]."""
    B, Cc, T = s.shape[:3]
    a, x = d(adj), d(s).reshape(B, Cc, T, -1)
    out = dict(out=(torch.einsum('bij,bcjp->bcip', a, x) + x).reshape(s.shape))
    if dout is not None:
        g = d(dout).reshape(B, Cc, T, -1)
        out['ds'] = (torch.einsum('bij,bcip->bcjp', a, g) + g).reshape(s.shape)
        out['dadj'] = torch.einsum('bcip,bcjp->bij', g, x)
    return out


# ----------------------------------------------------------------------------- BatchNorm
def _cview(v):
    return v.reshape(1, -1, 1)


def bn_train(x, gamma, beta, eps, momentum=0.1, rmean=None, rvar=None, residual=None, relu=False, dz=None):
    """Training-mode BatchNorm on (N, C, SP) [+ residual][ReLU] with TWO-PASS variance.
    -> dict(z, mean, var, invstd, rmean, rvar [, dx, dgamma, dbeta, dres by autograd for the upstream gradient dz])."""
    need = dz is not None
    N, Cc = x.shape[:2]
    x3 = d(x).reshape(N, Cc, -1).requires_grad_(need)
    g, b = d(gamma).requires_grad_(need), d(beta).requires_grad_(need)
    r3 = None if residual is None else d(residual).reshape(N, Cc, -1).requires_grad_(need)
    n = x3.shape[0] * x3.shape[2]
    mean = x3.mean((0, 2))
    var = ((x3 - _cview(mean)) ** 2).mean((0, 2))
    invstd = 1.0 / torch.sqrt(var + eps)
    z = (x3 - _cview(mean)) * _cview(invstd * g) + _cview(b)
    if r3 is not None:
        z = z + r3
    if relu:
        z = torch.relu(z)
    out = dict(z=z.detach().reshape(x.shape), mean=mean.detach(), var=var.detach(), invstd=invstd.detach())
    if rmean is not None:
        out['rmean'] = (1 - momentum) * d(rmean) + momentum * mean.detach()
        out['rvar'] = (1 - momentum) * d(rvar) + momentum * var.detach() * (n / (n - 1.0) if n > 1 else 1.0)
    if need:
        z.backward(d(dz).reshape(N, Cc, -1))
        out.update(dx=x3.grad.reshape(x.shape), dgamma=g.grad, dbeta=b.grad)
        if r3 is not None:
            out['dres'] = r3.grad.reshape(x.shape)
    return out


def bn_bwd_saved(dz, x, gamma, mean, invstd, mask=None):
    """BatchNorm backward from SAVED mean / invstd (as the ABI takes them) and the ReLU mask of the forward:
    xhat = (x - mean) * invstd; dzm = dz * mask; dx = gamma * invstd * (dzm - mean(dzm) - xhat * mean(dzm * xhat)).
    -> dict(dx, dgamma, dbeta, dres)."""
    N, Cc = x.shape[:2]
    x3, g3 = d(x).reshape(N, Cc, -1), d(dz).reshape(N, Cc, -1)
    if mask is not None:
        g3 = g3 * d(mask).reshape(N, Cc, -1)
    xhat = (x3 - _cview(d(mean))) * _cview(d(invstd))
    dbeta, dgamma = g3.sum((0, 2)), (g3 * xhat).sum((0, 2))
    n = x3.shape[0] * x3.shape[2]
    dx = _cview(d(gamma) * d(invstd)) * (g3 - _cview(dbeta) / n - xhat * _cview(dgamma) / n)
    return dict(dx=dx.reshape(x.shape), dgamma=dgamma, dbeta=dbeta, dres=g3.reshape(x.shape))


def bn_eval_fold(gamma, beta, rmean, rvar, eps):
    scale = d(gamma) / torch.sqrt(d(rvar) + eps)
    return scale, d(beta) - d(rmean) * scale


# ----------------------------------------------------------------------------- head pieces, optimiser
def l2norm(x, eps, dy=None):
    """F.normalize(x, dim=1, eps): y = x / max(|x|, eps).  -> dict(y, inv [, dx]).  Below the clamp the denominator is a
    constant, so dx = dy / eps there (what autograd gives: the norm's subgradient at 0 is 0)."""
    x = d(x)
    nrm = x.norm(dim=1, keepdim=True)
    inv = 1.0 / nrm.clamp_min(eps)
    out = dict(y=x * inv, inv=inv[:, 0])
    if dy is not None:
        g = d(dy)
        proj = out['y'] * (g * out['y']).sum(1, keepdim=True)
        out['dx'] = inv * (g - torch.where(nrm > eps, proj, torch.zeros_like(proj)))
    return out


def negcos(p, z, scale, eps=1e-8):
    """-scale * mean_i cos(p_i, z_i) with each norm clamped at eps (F.cosine_similarity), z a constant.
    -> dict(cos (rows), loss (), dp)."""
    p, z = d(p), d(z)
    np_, nz = p.norm(dim=1, keepdim=True).clamp_min(eps), z.norm(dim=1, keepdim=True).clamp_min(eps)
    cos = (p * z).sum(1, keepdim=True) / (np_ * nz)
    kf = -scale / p.shape[0]
    return dict(cos=cos[:, 0], loss=-scale * cos.mean(), dp=kf * (z / (np_ * nz) - cos * p / (np_ * np_)))


def sgd(p, g, buf, lr, wd, momentum, nesterov, coef=1.0, first=False):
    """One torch.optim.SGD step with per-element lr / wd: -> (p, buf)."""
    p, buf = d(p), d(buf)
    dd = coef * d(g) + d(wd) * p
    buf = dd if first else momentum * buf + dd
    dd = dd + momentum * buf if nesterov else buf
    return p - d(lr) * dd, buf


# ----------------------------------------------------------------------------- InfoNCE forward: dispatch rule and cases
def infonce_path(b, K, D, counter=True, aligned=True):
    """The path gca_moco_logits_fwd takes, from its arguments alone (infonce.hip; a workspace is always given):
      persistent  b <= 32, D <= 128, D % 8 == 0, counter given, q / k / queue 16-byte aligned, K * D * 4 < 0xfffff000:
                  waves = 4 if ncb >= 64 else 2 if ncb >= 16 else 1 (ncb = ceil(K / 32)), grid = min(ceil(ncb / waves), 256)
      fused       D <= 128, D % 8 == 0, aligned: waves = 8 if ncb > 1024 else 4 if ncb > 512 else 2 if ncb > 256 else 1
      plain       otherwise: moco_logits_kernel<4> when K >= 32768, else <1>; then row_stats_kernel
    -> (name, waves, workgroups)."""
    ncb = -(-K // 32)
    vec = D <= 128 and D % 8 == 0 and aligned
    if vec and b <= 32 and counter and K * D * 4 < 0xfffff000:
        w = 4 if ncb >= 64 else 2 if ncb >= 16 else 1
        return 'persist', w, min(-(-ncb // w), 256)
    if vec:
        w = 8 if ncb > 1024 else 4 if ncb > 512 else 2 if ncb > 256 else 1
        return 'fused', w, -(-ncb // w)
    w = 4 if K >= 32768 else 1
    return 'plain', w, -(-K // (32 * w))


# (id, b, K, D, counter given, q aligned) -> the path it must take: (name, waves, workgroups or None = not pinned)
INFONCE_CASES = [
    ('persist-1w', 5, 300, 64, True, True, ('persist', 1, 10)),
    ('persist-2w', 5, 1000, 64, True, True, ('persist', 2, 16)),
    ('persist-4w', 5, 2100, 64, True, True, ('persist', 4, 17)),
    ('persist-capped', 7, 40017, 64, True, True, ('persist', 4, 256)),      # 1251 column blocks over 1024 waves
    ('persist-32rows', 32, 2100, 128, True, True, ('persist', 4, 17)),
    ('fused-small-b', 7, 2100, 64, False, True, ('fused', 1, 66)),
    ('fused-1w', 33, 700, 32, True, True, ('fused', 1, 22)),
    ('fused-2w', 33, 8200, 32, True, True, ('fused', 2, 129)),
    ('fused-4w', 33, 16500, 32, True, True, ('fused', 4, 129)),
    ('fused-8w', 33, 32800, 32, True, True, ('fused', 8, 129)),
    ('plain1-D100', 6, 2100, 100, True, True, ('plain', 1, 66)),
    ('plain4-D136', 3, 32800, 136, True, True, ('plain', 4, 257)),
    ('plain1-misaligned', 6, 2100, 64, True, False, ('plain', 1, 66)),
]
INFONCE_INV_T = 16.0
INFONCE_TIES = 3            # copies of every key planted in the queue


def infonce_exact_inputs(b, K, D, seed=0):
    """q, k, queue with entries (integer / 8) in [-2, 2]: with inv_T = 16 every product, partial sum and logit is a
    multiple of 1/4 far below 2^24 of them, i.e. exact in fp32 in ANY summation order.  INFONCE_TIES copies of each k_i sit
    at seeded queue rows (the last one in the final, ragged 32-row block), so every row has exact ties with its positive."""
    g = torch.Generator().manual_seed(1000 + seed)
    q = torch.randint(-16, 17, (b, D), generator=g).float() / 8
    k = torch.randint(-16, 17, (b, D), generator=g).float() / 8
    queue = torch.randint(-16, 17, (K, D), generator=g).float() / 8
    rows = torch.randperm(K - b, generator=g)[:(INFONCE_TIES - 1) * b].reshape(INFONCE_TIES - 1, b)
    for t in range(INFONCE_TIES - 1):
        queue[rows[t]] = k
    queue[K - b:] = k
    return q, k, queue


def infonce_wide_inputs(b=8, K=2100, D=128, seed=0):
    """Unnormalised randn q / k / queue (logits reach hundreds at inv_T = 1 / 0.07); rows 0 and 1 get k_i = 4 q_i / |q_i|,
    which makes their positive the row maximum by a wide margin (loss_i ~ 0: lse - l0 cancels)."""
    g = torch.Generator().manual_seed(2000 + seed)
    q, k, queue = torch.randn(b, D, generator=g), torch.randn(b, D, generator=g), torch.randn(K, D, generator=g)
    k[:2] = 4 * q[:2] / q[:2].norm(dim=1, keepdim=True)
    return q, k, queue


# ----------------------------------------------------------------------------- graph cases
GRAPH_SHAPES = [(1, 4), (2, 8), (3, 8), (4, 9), (5, 7), (8, 12), (16, 4), (16, 6), (32, 4)]       # (T, HW)


def graph_inputs(B, Cc, T, HW, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(3000 + seed)
    return [torch.randn(B, Cc, T, HW, 1, generator=g) * scale for _ in range(3)]


def graph_onehot_inputs(B=2, Ci=6, T=4, HW=8):
    """gq = gk = 6 * (+-1 pattern, rows of a Hadamard matrix per frame): <gq_i, gk_j> = 36 * Ci * HW * [i == j] (+ nothing
    else), so every softmax row is one-hot to within fp32 and adj_pre sits on BOTH clamps: 0 -> eps off the diagonal,
    theta(0) = 1 on it -> 1 - eps.  Clip 1 is scaled down (x 0.02) so that its rows are soft and interior."""
    had = torch.tensor([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]], dtype=torch.float32)
    assert T == 4 and HW % 4 == 0
    pat = had[:, None, :].repeat(1, Ci, HW // 4).reshape(T, Ci, HW).permute(1, 0, 2)      # (Ci, T, HW), frame i = row i
    gq = torch.stack([6.0 * pat, 0.02 * 6.0 * pat] + [6.0 * pat] * (B - 2))[:B].reshape(B, Ci, T, HW, 1).contiguous()
    return gq, gq.clone()


# ----------------------------------------------------------------------------- BatchNorm conditioning envelope
BN_SIGMAS = (0.05, 1.0, 20.0)
BN_RATIOS = (0, 3, 10, 30)
BN_SHAPES = [(4, 6, 24), (2, 4, 20000), (8, 6, 1), (2, 5, 1)]        # (N, C, SP): small, multi-part stats, BatchNorm1d, count 2


def bn_envelope_input(N, Cc, SP, k, seed=0, dtype=torch.float32):
    """x[:, c] = sigma_c * (k + zhat_c): zhat_c is randn standardised per channel in fp64 (zero mean, unit biased variance),
    so the realised |mean| / std IS k up to the rounding of x to `dtype` -- also at count = 2, where zhat = +-1.
    sigma_c cycles through BN_SIGMAS.  -> (x, sigma (C))."""
    g = torch.Generator().manual_seed(4000 + seed)
    zh = torch.randn(N, Cc, SP, generator=g, dtype=F64)
    zh = zh - zh.mean((0, 2), keepdim=True)
    zh = zh / zh.pow(2).mean((0, 2), keepdim=True).sqrt()
    sigma = torch.tensor([BN_SIGMAS[c % len(BN_SIGMAS)] for c in range(Cc)], dtype=F64)
    return (_cview(sigma) * (k + zh)).to(dtype), sigma


def bn_ratio(x):
    """Realised |mean| / std (biased) per channel of (N, C, SP), in fp64."""
    x3 = d(x).reshape(x.shape[0], x.shape[1], -1)
    m = x3.mean((0, 2))
    return m.abs() / ((x3 - _cview(m)) ** 2).mean((0, 2)).sqrt()


def bn_var_bound(k, roundings=1):
    """Relative error of var = E[x^2] - mean^2 when every partial of sum(x) and of sum(x^2) carries `roundings` fp32
    roundings: d(E[x^2]) <= r u (sigma^2 + mu^2) and d(mean^2) <= 2 r u mu^2, over sigma^2: r (1 + 3 k^2) 2^-24."""
    return roundings * (1 + 3 * k * k) * U32


def bn_invstd_bound(k, roundings=1):
    """Half the variance bound (invstd = (var + eps)^-1/2) + the rounding of the stored fp32 value and slack: 2^-23."""
    return 0.5 * bn_var_bound(k, roundings) + 2 * U32


def emulate_fp32_partials(x, parts):
    """The E[x^2] - mean^2 route of bn.hip on the CPU: per-part fp64 sums rounded to fp32, folded in fp64.
    x (n,) fp64 -> (mean, var)."""
    n = x.numel()
    s = q = 0.0
    for c in x.chunk(parts):
        s += float(c.sum().float())
        q += float((c * c).sum().float())
    m = s / n
    return m, max(q / n - m * m, 0.0)
