"""ReSSL's loss (Zheng et al. 2021, "ReSSL: Relational Self-Supervised Learning with Weak Augmentation") on the fused HIP
kernels (csrc/ressl.hip).

The MoCo queue (``memory``, as lib.memory.mem_moco.RGBMoCo keeps it) holds the ANCHORS of a relation, not negatives: the
momentum teacher's row k_i is compared with every queue row at a sharp temperature Tt, the student's row q_i at Ts >= Tt, and the
student is taught the teacher's distribution over the anchors:

    loss = mean_i  - sum_j softmax(k_i Q^T / Tt)_j  log softmax(q_i Q^T / Ts)_j

``ReSSLLoss(n_dim, K, Ts, Tt)(q, k, all_k=None) -> loss`` (0-dim) is differentiable in q through ONE autograd node; k is used
detached and receives nothing.  Order of a forward: (1) the loss against the PRE-enqueue queue, (2) when q needs a gradient,
d loss / d q against that same queue in the same call (so the enqueue below needs no saved rows), (3) ``all_k`` (or k) is written
at rows (index + i) % K and ``index`` advances -- a Python attribute, as RGBMoCo's.  After a forward ``.ent`` holds the teacher's
mean entropy (0-dim; it falls towards 0 when the teacher collapses onto single anchors and sits at log K for a uniform one) and
``.row_loss`` the (N,) per-row losses.  Unit rows are the caller's business.  tests/ressl_ref.py states the arithmetic."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ...engine import ops


class _ReSSLFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, mod, want_grad):
        q = q.detach().contiguous()
        inv_Ts, inv_Tt = 1.0 / mod.Ts, 1.0 / mod.Tt
        loss, row_lse, mod.row_loss = ops.ressl_fwd(q, k, mod.memory, inv_Ts, inv_Tt)
        mod.ent = loss[1].reshape(())
        ctx.dq = ops.ressl_bwd(q, k, mod.memory, row_lse, inv_Ts, inv_Tt) if want_grad else None
        return loss[0].reshape(())

    @staticmethod
    def backward(ctx, g):
        if ctx.dq is None:
            raise RuntimeError('ReSSLLoss: no gradient to hand out (q did not require one when the loss was computed, or this is '
                               'a second backward through the same forward)')
        dq, ctx.dq = ctx.dq, None                                      # scaled in place: one backward per forward
        ops.scale_dev_(dq, g.to(torch.float32).contiguous().reshape(1))
        return dq, None, None, None


class ReSSLLoss(nn.Module):
    def __init__(self, n_dim, K=65536, Ts=0.1, Tt=0.04):
        super().__init__()
        Ts, Tt = float(Ts), float(Tt)
        for name, T in (('Ts', Ts), ('Tt', Tt)):
            if not (T > 0 and T < 3.0e38 and 1.0 / T < 3.0e38):
                raise ValueError('ReSSLLoss: %s must be positive, T and 1 / T finite in fp32 (got %r)' % (name, T))
        if Tt > Ts:
            raise ValueError('ReSSLLoss: the teacher must be the sharper one, Tt <= Ts (got Ts=%r, Tt=%r)' % (Ts, Tt))
        for name, v in (('n_dim', n_dim), ('K', K)):
            if isinstance(v, bool) or int(v) != v or int(v) < 1:
                raise ValueError('ReSSLLoss: %s must be a positive integer (got %r)' % (name, v))
        self.K, self.Ts, self.Tt, self.index = int(K), Ts, Tt, 0
        self.ent = self.row_loss = None
        self.register_buffer('memory', F.normalize(torch.randn(int(K), int(n_dim))))     # as RGBMoCo's queue

    def forward(self, q, k, all_k=None):
        if q.dim() != 2 or k.shape != q.shape:
            raise ValueError('ReSSLLoss: q and k are (N, D) matrices of one shape (got %s, %s)' % (tuple(q.shape), tuple(k.shape)))
        k = k.detach().contiguous()
        all_k = k if all_k is None else all_k.detach().contiguous()
        n = all_k.shape[0]
        if n > self.K:
            raise ValueError('ReSSLLoss: cannot enqueue %d rows into a queue of %d' % (n, self.K))
        loss = _ReSSLFn.apply(q, k, self, bool(q.requires_grad and torch.is_grad_enabled()))
        ops.queue_enqueue(self.memory, all_k, self.index)
        self.index = (self.index + n) % self.K
        return loss
