"""The specification of the fused Adam / AdamW arena update (gca_adam_step), in fp64 numpy.

torch.optim.Adam / AdamW with amsgrad=False, maximize=False, for step t (1-based), over per-element lr / weight-decay arrays:

    g  = grad * coef
    Adam : g += wd * p          AdamW : p *= 1 - lr * wd
    m  = beta1 * m + (1 - beta1) * g
    v  = beta2 * v + (1 - beta2) * g * g
    p -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)

tests/test_adam_ref.py holds it to torch's own optimizers in fp64; tests/test_gpu_adam.py holds the kernel to it."""
import numpy as np

CHUNK = 256


def adam_step(p, g, m, v, t, lr, wd, betas=(0.9, 0.999), eps=1e-8, decoupled=False, coef=1.0, skip=False):
    """-> (p, m, v) after step t.  All arrays fp64 of one shape (lr / wd per element, or scalars); skip: the step does not happen."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    if skip:
        return p.copy(), m.copy(), v.copy()
    b1, b2 = float(betas[0]), float(betas[1])
    lr, wd = np.asarray(lr, dtype=np.float64), np.asarray(wd, dtype=np.float64)
    g = g * float(coef)
    if decoupled:
        p = p * (1.0 - lr * wd)
    else:
        g = g + wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** int(t), 1.0 - b2 ** int(t)
    p = p - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    return p, m, v


def update_magnitude(p, g, m, v, t, lr, wd, betas=(0.9, 0.999), eps=1e-8, decoupled=False, coef=1.0):
    """|update| of p, m and v for the error bar k * 2^-24 * max(|value|, |update|): the step above with every term replaced by
    its absolute value, so that nothing cancels -- a rounding of any term on the way to a value is relative to that term, and
    these bound every one of them.  -> (|lr / bc1 * m / denom|, |beta1 * m| + |(1 - beta1) * g|, beta2 * v + (1 - beta2) * g^2)
    with |g| = |grad * coef| + wd * |p| under Adam."""
    p, g, m, v = (np.abs(np.asarray(a, dtype=np.float64)) for a in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    lr, wd = np.asarray(lr, dtype=np.float64), np.asarray(wd, dtype=np.float64)
    g = g * abs(float(coef))
    if not decoupled:
        g = g + wd * p
    ms = b1 * m + (1.0 - b1) * g
    vs = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** int(t), 1.0 - b2 ** int(t)
    return (lr / bc1) * ms / (np.sqrt(vs) / np.sqrt(bc2) + eps), ms, vs


def arena_layout(sizes):
    """-> (offsets, total) of tensors of `sizes` elements in an arena that pads each to a multiple of 256."""
    offs, off = [], 0
    for s in sizes:
        offs.append(off)
        off += (int(s) + CHUNK - 1) // CHUNK * CHUNK
    return offs, off


def expand_chunks(sizes, values):
    """One value per tensor -> one per ELEMENT of the arena (padding elements take their tensor's value, as the chunk tables
    of the product give every chunk of a tensor that tensor's value)."""
    offs, total = arena_layout(sizes)
    out = np.zeros(total, dtype=np.float64)
    for o, s, val in zip(offs, sizes, values):
        out[o:o + (int(s) + CHUNK - 1) // CHUNK * CHUNK] = float(val)
    return out


def chunk_table(sizes, values):
    """One value per tensor -> one per 256-element chunk (what the kernel reads)."""
    return expand_chunks(sizes, values)[::CHUNK].copy()


def padding_mask(sizes):
    offs, total = arena_layout(sizes)
    pad = np.ones(total, dtype=bool)
    for o, s in zip(offs, sizes):
        pad[o:o + int(s)] = False
    return pad
