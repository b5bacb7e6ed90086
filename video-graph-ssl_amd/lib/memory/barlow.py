"""The Barlow Twins loss (redundancy reduction between the two views' features) on the fused HIP kernels (csrc/barlow.hip).

The reference has no such objective; it needs no negatives, queue, momentum encoder or predictor: each view's (N, D) features
are standardised per column over the batch, C = a^T b / N is their (D, D) cross-correlation and the loss pulls C towards the
identity, ``sum_i (C_ii - 1)^2 + lambd * sum_{i != j} C_ij^2``.  ``BarlowTwinsLoss(lambd, eps)(z1, z2) -> loss`` (0-dim,
unscaled) is differentiable through ONE autograd node; after a forward ``.on_diag`` and ``.off_diag`` hold the two sums
(device scalars) for logging.  tests/barlow_ref.py states the arithmetic."""
import torch
import torch.nn as nn

from ...engine import ops


class _BarlowFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z1, z2, mod):
        z1, z2 = z1.contiguous(), z2.contiguous()
        loss3, stats, cmat, rsum = ops.barlow_fwd(z1, z2, mod.lambd, mod.eps)
        mod.on_diag, mod.off_diag = loss3[1], loss3[2]
        ctx.saved, ctx.lambd = (z1, z2, stats, cmat, rsum), mod.lambd
        return loss3[0].reshape(())

    @staticmethod
    def backward(ctx, g):
        dz1, dz2 = ops.barlow_bwd(*ctx.saved, ctx.lambd, gscale_dev=g.contiguous().reshape(1))
        return dz1, dz2, None


class BarlowTwinsLoss(nn.Module):
    def __init__(self, lambd=0.0051, eps=1e-5):
        super().__init__()
        lambd, eps = float(lambd), float(eps)
        if not 0.0 <= lambd < float('inf'):
            raise ValueError('BarlowTwinsLoss: lambd must be non-negative and finite (got %r)' % lambd)
        if not 0.0 <= eps < float('inf'):
            raise ValueError('BarlowTwinsLoss: eps must be non-negative and finite (got %r)' % eps)
        self.lambd, self.eps = lambd, eps
        self.on_diag = self.off_diag = None

    def forward(self, z1, z2):
        if z1.dim() != 2 or z1.shape != z2.shape:
            raise ValueError('BarlowTwinsLoss: two (N, D) views expected (got %s, %s)' % (tuple(z1.shape), tuple(z2.shape)))
        return _BarlowFn.apply(z1, z2, self)
