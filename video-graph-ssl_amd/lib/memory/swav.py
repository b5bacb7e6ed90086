"""SwAV's swapped-prediction loss (Caron et al. 2020, "Unsupervised Learning of Visual Features by Contrasting Cluster
Assignments") on the fused HIP kernels (csrc/swav.hip).

The reference has no such objective.  The unit-row features of the two views are scored against K learned unit-row prototypes,
``S_v = z_v C^T``; a Sinkhorn-Knopp normalisation of ``exp(S_v / eps)`` (`iters` rounds, no gradient) gives each view's codes
``q_v``, and each view predicts the other's codes: ``loss = -(mean_n sum_k q_2 log_softmax(S_1 / T) + mean_n sum_k q_1
log_softmax(S_2 / T)) / 2``.  ``SwAVLoss(eps, T, iters)(z1, z2, C) -> loss`` (0-dim) is differentiable in z1, z2 and C through
ONE autograd node; after a forward ``.l12`` and ``.l21`` hold the two terms (device scalars) for logging.  Unit rows of z and C
are the caller's business (the trainer's model normalises both).  tests/swav_ref.py states the arithmetic."""
import torch
import torch.nn as nn

from ...engine import ops


class _SwAVFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z1, z2, C, mod):
        z1, z2, C = z1.contiguous(), z2.contiguous(), C.contiguous()
        parts, dS = ops.swav_fwd(z1, z2, C, mod.eps, mod.T, mod.iters)
        mod.l12, mod.l21 = parts[1], parts[2]
        ctx.saved = (z1, z2, C, dS)
        return parts[0].reshape(())

    @staticmethod
    def backward(ctx, g):
        z1, z2, C, dS = ctx.saved
        dC = torch.empty_like(C)
        dz1, dz2 = ops.swav_bwd(z1, z2, C, dS, dC, False, gscale_dev=g.contiguous().reshape(1))
        return dz1, dz2, dC, None


class SwAVLoss(nn.Module):
    def __init__(self, eps=0.05, T=0.1, iters=3):
        super().__init__()
        self.eps, self.T, self.iters = ops.swav_params('SwAVLoss', eps, T, iters)
        self.l12 = self.l21 = None

    def forward(self, z1, z2, C):
        if z1.dim() != 2 or z1.shape != z2.shape or C.dim() != 2 or C.shape[1] != z1.shape[1]:
            raise ValueError('SwAVLoss: two (N, D) views and (K, D) prototypes expected (got %s, %s, %s)'
                             % (tuple(z1.shape), tuple(z2.shape), tuple(C.shape)))
        return _SwAVFn.apply(z1, z2, C, self)
