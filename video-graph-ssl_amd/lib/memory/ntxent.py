"""NT-Xent, SimCLR's in-batch contrastive loss, on the fused HIP kernels (csrc/ntxent.hip).

The reference has no such objective (its memories are the MoCo queue and SimSiam's none); this is the loss its LARS-era
relatives train with: the two views of a batch of b clips give N = 2b rows, the positive of a row is the other view of its
clip and every other row is a negative -- no queue, no momentum encoder.  ``NTXent(T)(z1, z2) -> loss`` (0-dim) is
differentiable through ONE autograd node; after a forward ``NTXent.rank`` holds, per row, how many negatives score at least
its positive (int32, on the device; top-k hit iff rank < k).  tests/ntxent_ref.py states the arithmetic."""
import torch
import torch.nn as nn

from ...engine import ops


class _NTXentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z1, z2, mod):
        b = z1.shape[0]
        z = torch.cat([z1, z2], 0).contiguous()
        loss, lse, mod.rank = ops.ntxent_fwd(z, 1.0 / mod.T, want_rank=True)
        ctx.z, ctx.lse, ctx.inv_T, ctx.b = z, lse, 1.0 / mod.T, b
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        dz = ops.ntxent_bwd(ctx.z, ctx.lse, ctx.inv_T, gscale_dev=g.contiguous().reshape(1))
        return dz[:ctx.b], dz[ctx.b:], None


class NTXent(nn.Module):
    def __init__(self, T=0.07):
        super().__init__()
        T = float(T)
        if not T > 0:
            raise ValueError('NTXent: the temperature must be positive (got %r)' % T)
        self.T, self.rank = T, None

    def forward(self, z1, z2):
        if z1.dim() != 2 or z1.shape != z2.shape:
            raise ValueError('NTXent: two (b, D) views expected (got %s, %s)' % (tuple(z1.shape), tuple(z2.shape)))
        return _NTXentFn.apply(z1, z2, self)
