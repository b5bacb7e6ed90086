"""NNCLR's loss (Dwibedi et al. 2021, "With a Little Help from My Friends: Nearest-Neighbor Contrastive Learning of Visual
Representations", Algorithm 1) on the fused HIP kernels (csrc/nnclr.hip, csrc/mocov3.hip).

A MoCo-style FIFO of past projections (``memory``, as lib.memory.mem_moco.RGBMoCo keeps it) serves as a SUPPORT SET, not as
negatives: each view's projection z is replaced by its nearest neighbour in the support set, and that neighbour is contrasted
in-batch against the other view's prediction p -- row i's positive is column i, every other clip of the batch is a negative,
the softmax runs over the predictions.  No momentum encoder.

``NNCLRLoss(n_dim, K, T)(z1, z2, p1, p2) -> loss`` (0-dim), ``(CE(nn1 p2^T / T) + CE(nn2 p1^T / T)) / 2``, is differentiable
in p1 and p2 through ONE autograd node; z1 and z2 are used detached and receive nothing (the arg-max has no gradient).  Order of
a forward: (1) search the PRE-enqueue support set, (2) the loss, (3) z1 is written at rows (index + i) % K and ``index``
advances -- a Python attribute, as RGBMoCo's.  After a forward ``.idx`` / ``.sim`` (2, N) hold the neighbours and their scores,
``.rank`` (2, N) int32 how many other predictions score at least the positive, ``.l12`` / ``.l21`` the two direction losses.
Unit rows are the caller's business.  tests/nnclr_ref.py states the arithmetic."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ...engine import ops


class _NNCLRFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p1, p2, z1, z2, mod):
        p1, p2 = p1.detach().contiguous(), p2.detach().contiguous()
        inv_T = 1.0 / mod.T
        mod.idx, mod.sim, nn1, nn2 = ops.nnclr_search(z1, z2, mod.memory)
        loss, lse, mod.rank, _ = ops.mocov3_fwd(nn1, nn2, p1, p2, inv_T, w=ops.nnclr_weight(), want_rank=True)
        mod.l12, mod.l21 = loss[1], loss[2]
        ctx.ops, ctx.lse, ctx.inv_T = (nn1, nn2, p1, p2), lse, inv_T
        return loss[0].reshape(())

    @staticmethod
    def backward(ctx, g):
        dp1, dp2 = ops.nnclr_bwd(*ctx.ops, ctx.lse, ctx.inv_T, gscale_dev=g.contiguous().reshape(1))
        return dp1, dp2, None, None, None


class NNCLRLoss(nn.Module):
    def __init__(self, n_dim, K=65536, T=0.1):
        super().__init__()
        T = float(T)
        if not (T > 0 and T < 3.0e38 and 1.0 / T < 3.0e38):
            raise ValueError('NNCLRLoss: the temperature must be positive, T and 1 / T finite in fp32 (got %r)' % T)
        for name, v in (('n_dim', n_dim), ('K', K)):
            if isinstance(v, bool) or int(v) != v or int(v) < 1:
                raise ValueError('NNCLRLoss: %s must be a positive integer (got %r)' % (name, v))
        self.K, self.T, self.index = int(K), T, 0
        self.idx = self.sim = self.rank = self.l12 = self.l21 = None
        self.register_buffer('memory', F.normalize(torch.randn(int(K), int(n_dim))))     # as RGBMoCo's queue

    def forward(self, z1, z2, p1, p2):
        if p1.dim() != 2 or any(t.shape != p1.shape for t in (z1, z2, p2)):
            raise ValueError('NNCLRLoss: four (N, D) matrices of one shape expected (got %s)'
                             % ', '.join(str(tuple(t.shape)) for t in (z1, z2, p1, p2)))
        n = p1.shape[0]
        if n > self.K:
            raise ValueError('NNCLRLoss: cannot enqueue %d rows into a support set of %d' % (n, self.K))
        z1, z2 = z1.detach().contiguous(), z2.detach().contiguous()
        loss = _NNCLRFn.apply(p1, p2, z1, z2, self)
        ops.queue_enqueue(self.memory, z1, self.index)
        self.index = (self.index + n) % self.K
        return loss
