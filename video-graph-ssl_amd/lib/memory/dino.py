"""DINO's self-distillation loss (Caron et al. 2021, "Emerging Properties in Self-Supervised Vision Transformers") on the fused
HIP kernels (csrc/dino.hip).

The reference has no such objective.  The unit-row features of the two views are scored against K unit-row prototypes, by the
student (``Ss_v = zs_v Cs^T``) and by its momentum teacher (``St_v = zt_v Ct^T``); the teacher's scores are centred and
sharpened, ``p_v = softmax((St_v - c) / Tt)`` (no gradient), and the student's other view predicts them: ``loss = -(mean_n sum_k
p_1 log_softmax(Ss_2 / Ts) + mean_n sum_k p_2 log_softmax(Ss_1 / Ts)) / 2``.  The centre ``c`` is an EMA (momentum ``cm``) of the
teacher scores' batch mean, moved AFTER the loss has used it and only in training mode.

``DINOLoss(K, Ts, Tt, cm)(zs1, zs2, Cs, zt1, zt2, Ct) -> loss`` (0-dim) is differentiable in zs1, zs2 and Cs through ONE autograd
node; after a forward ``.l12``, ``.l21`` and ``.ent`` (the mean teacher entropy, log K when collapsed to uniform, 0 when collapsed
to one prototype) hold device scalars for logging.  ``center`` is a registered buffer (K, zeros); ``set_teacher_temp`` moves the
teacher temperature, which the kernels read from the device.  Unit rows are the caller's business.  tests/dino_ref.py states the
arithmetic."""
import torch
import torch.nn as nn

from ...engine import ops


class _DINOFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, zs1, zs2, Cs, zt1, zt2, Ct, mod):
        zs1, zs2, Cs = zs1.contiguous(), zs2.contiguous(), Cs.contiguous()
        parts, dS = ops.dino_fwd(zs1, zs2, Cs, zt1.detach(), zt2.detach(), Ct.detach(), mod.Ts, mod.tt_dev(zs1.device), mod.cm,
                                 mod.center, mod.training)
        mod.l12, mod.l21, mod.ent = parts[1], parts[2], parts[3]
        ctx.saved = (zs1, zs2, Cs, dS)
        return parts[0].reshape(())

    @staticmethod
    def backward(ctx, g):
        zs1, zs2, Cs, dS = ctx.saved
        dC = torch.empty_like(Cs)
        dz1, dz2 = ops.dino_bwd(zs1, zs2, Cs, dS, dC, False, gscale_dev=g.contiguous().reshape(1))
        return dz1, dz2, dC, None, None, None, None


class DINOLoss(nn.Module):
    def __init__(self, K=4096, Ts=0.1, Tt=0.04, cm=0.9):
        super().__init__()
        if isinstance(K, bool) or int(K) != K or not 2 <= int(K) <= 65536:
            raise ValueError('DINOLoss: the number of prototypes must lie in [2, 65536] (got %r)' % (K,))
        self.K = int(K)
        self.Ts, self.Tt, self.cm = ops.dino_params('DINOLoss', Ts, Tt, cm)
        self.register_buffer('center', torch.zeros(self.K))
        self._tt = None                     # the teacher temperature on the device, made on first use
        self.l12 = self.l21 = self.ent = None

    def set_teacher_temp(self, Tt):
        """The teacher temperature of the following forwards (its warm-up schedule: lib.solver.dino_teacher_temp)."""
        self.Tt = ops.dino_temperature('DINOLoss', Tt)
        if self._tt is not None:
            self._tt.fill_(self.Tt)

    def tt_dev(self, device):
        if self._tt is None or self._tt.device != device:
            self._tt = torch.full((1,), self.Tt, dtype=torch.float32, device=device)
        return self._tt

    def forward(self, zs1, zs2, Cs, zt1, zt2, Ct):
        if zs1.dim() != 2 or zs1.shape != zs2.shape or Cs.dim() != 2 or Cs.shape != (self.K, zs1.shape[1]):
            raise ValueError('DINOLoss: two (N, D) views and (%d, D) prototypes expected (got %s, %s, %s)'
                             % (self.K, tuple(zs1.shape), tuple(zs2.shape), tuple(Cs.shape)))
        if zt1.shape != zs1.shape or zt2.shape != zs1.shape or Ct.shape != Cs.shape:
            raise ValueError('DINOLoss: the teacher operands must have the student shapes, two %s views and %s prototypes (got %s, %s, %s)'
                             % (tuple(zs1.shape), tuple(Cs.shape), tuple(zt1.shape), tuple(zt2.shape), tuple(Ct.shape)))
        return _DINOFn.apply(zs1, zs2, Cs, zt1, zt2, Ct, self)
