"""MoCo v3's loss (Chen, Xie, He 2021, "An Empirical Study of Training Self-Supervised Vision Transformers", Algorithm 1) on the
fused HIP kernels (csrc/mocov3.hip).

The queue-free, symmetrised successor of the MoCo the reference trains: the student's predictor outputs q1, q2 of the two views
are scored against the momentum teacher's projector outputs k1, k2 of the same batch, q1 against k2 and q2 against k1; the
positive of row i is column i and every other clip of the batch is a negative.  ``MoCoV3Loss(T)(q1, q2, k1, k2) -> loss`` (0-dim),
2 T (CE(q1 k2^T / T) + CE(q2 k1^T / T)), is differentiable in q1 and q2 through ONE autograd node; k1 and k2 are the detached
teacher's and receive no gradient.  After a forward ``.rank`` (2, N) int32 holds, per direction and row, how many other columns
score at least the positive (on the device; top-k hit iff rank < k) and ``.l12`` / ``.l21`` the two direction losses.  Unit
rows are the caller's business.  tests/mocov3_ref.py states the arithmetic."""
import torch
import torch.nn as nn

from ...engine import ops


class _MoCoV3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q1, q2, k1, k2, mod):
        q1, q2, k1, k2 = (t.detach().contiguous() for t in (q1, q2, k1, k2))
        inv_T = 1.0 / mod.T
        loss, lse, mod.rank, _ = ops.mocov3_fwd(q1, q2, k1, k2, inv_T, want_rank=True)
        mod.l12, mod.l21 = loss[1], loss[2]
        ctx.ops, ctx.lse, ctx.inv_T = (q1, q2, k1, k2), lse, inv_T
        return loss[0].reshape(())

    @staticmethod
    def backward(ctx, g):
        dq1, dq2 = ops.mocov3_bwd(*ctx.ops, ctx.lse, ctx.inv_T, gscale_dev=g.contiguous().reshape(1))
        return dq1, dq2, None, None, None


class MoCoV3Loss(nn.Module):
    def __init__(self, T=0.2):
        super().__init__()
        T = float(T)
        if not (T > 0 and T < 3.0e38 and 1.0 / T < 3.0e38):
            raise ValueError('MoCoV3Loss: the temperature must be positive, T and 1 / T finite in fp32 (got %r)' % T)
        self.T, self.rank, self.l12, self.l21 = T, None, None, None

    def forward(self, q1, q2, k1, k2):
        if q1.dim() != 2 or any(t.shape != q1.shape for t in (q2, k1, k2)):
            raise ValueError('MoCoV3Loss: four (N, D) matrices of one shape expected (got %s)'
                             % ', '.join(str(tuple(t.shape)) for t in (q1, q2, k1, k2)))
        return _MoCoV3Fn.apply(q1, q2, k1, k2, self)
