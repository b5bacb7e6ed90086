"""The specification of the fused LARS arena update (gca_lars_step), in fp64 numpy.

apex LARC(clip=False) around torch.optim.SGD (dampening 0).  For each tensor i of the arena with weights w, gradient grad, its
lr and wd, the trust coefficient tau, eps and the clip coefficient coef:

    g   = grad * coef
    nw  = ||w||_2          ng = ||g||_2 = coef * ||grad||_2
    q   = tau * nw / (ng + wd * nw + eps)   if the tensor is adapted and nw > 0 and ng > 0, else 1
    d   = q * (g + wd * w)
    buf = momentum * buf + d                (buf starts at 0)
    w  -= lr * (nesterov ? d + momentum * buf : buf)

tests/test_lars_ref.py holds it to torch.optim.SGD fed q * (g + wd * w) in fp64; tests/test_gpu_lars.py holds the kernels to it."""
import math

import numpy as np

from adam_ref import CHUNK, arena_layout, chunk_table, expand_chunks, padding_mask      # noqa: F401  (the arena's layout rules)


def norms_of(p, g, sizes, coef=1.0):
    """-> (n_tensors, 2) fp64: (||w||, coef * ||grad||) per tensor, each sum of squares formed exactly (math.fsum) and rounded
    once, then the square root: within 1.5 * 2^-53 relative of the true norm, whatever the tensor's size."""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    offs, _ = arena_layout(sizes)
    out = np.zeros((len(sizes), 2))
    for i, (o, n) in enumerate(zip(offs, sizes)):
        out[i, 0] = math.sqrt(math.fsum(p[o:o + n] * p[o:o + n]))
        out[i, 1] = abs(float(coef)) * math.sqrt(math.fsum(g[o:o + n] * g[o:o + n]))
    return out


def trust_of(norms, wd, adapt, tau, eps):
    """-> q per tensor from its (nw, ng), weight decay and adapt flag."""
    q = np.ones(len(norms))
    for i, ((nw, ng), w_, a) in enumerate(zip(norms, wd, adapt)):
        if a and nw > 0.0 and ng > 0.0:
            q[i] = float(tau) * nw / (ng + float(w_) * nw + float(eps))
    return q


def sgd_step(p, g, buf, lr, wd, momentum=0.9, nesterov=False, coef=1.0, skip=False, q=1.0):
    """torch.optim.SGD (dampening 0) on fp64 arrays with per-element (or scalar) lr / wd and the extra factor q on g + wd * p.
    -> (p, buf)"""
    p, g, buf = (np.asarray(a, dtype=np.float64) for a in (p, g, buf))
    if skip:
        return p.copy(), buf.copy()
    d = q * (g * float(coef) + wd * p)
    buf = float(momentum) * buf + d
    return p - lr * (d + float(momentum) * buf if nesterov else buf), buf


def lars_step(p, g, buf, sizes, lr, wd, adapt, momentum=0.9, nesterov=False, tau=0.001, eps=1e-8, coef=1.0, skip=False):
    """One step over the flat arena of tensors of `sizes` elements; lr / wd / adapt: one value per TENSOR.
    -> (p, buf, q per tensor, norms (n_tensors, 2)); on skip the state comes back unchanged and q, norms are None."""
    if skip:
        return sgd_step(p, g, buf, 0.0, 0.0, skip=True) + (None, None)
    norms = norms_of(p, g, sizes, coef)
    q = trust_of(norms, wd, adapt, tau, eps)
    p, buf = sgd_step(p, g, buf, expand_chunks(sizes, lr), expand_chunks(sizes, wd), momentum, nesterov, coef,
                      q=expand_chunks(sizes, q))
    return p, buf, q, norms


def update_magnitude(p, g, buf, sizes, lr, wd, q, momentum=0.9, nesterov=False, coef=1.0):
    """|update| of p and buf for the error bar k * 2^-24 * max(|value|, |update|): the step with every term replaced by its
    absolute value, so that nothing cancels (a rounding of any term on the way to a value is relative to that term, and these
    bound every one of them).  q: per tensor, as given.  -> (lr * (|d| + momentum * |buf'|  or  |buf'|), |buf'|) with
    |d| = q * (|grad * coef| + wd * |p|), |buf'| = momentum * |buf| + |d|."""
    p, g, buf = (np.abs(np.asarray(a, dtype=np.float64)) for a in (p, g, buf))
    lr, wd, q = (expand_chunks(sizes, v) for v in (lr, wd, q))
    d = q * (g * abs(float(coef)) + wd * p)
    b = float(momentum) * buf + d
    return lr * (d + float(momentum) * b if nesterov else b), b
