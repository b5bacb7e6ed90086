"""The VICReg loss (variance / invariance / covariance regularisation of the two views' features) on the fused HIP kernels
(csrc/vicreg.hip).

The reference has no such objective; like Barlow Twins it needs no negatives, queue, momentum encoder or predictor, and it does
not standardise the features: ``sim * mse(z1, z2) + std * mean(relu(1 - sd)) / 2 (both views) + cov * sum of squared
off-diagonal covariances / D (both views)`` with the unbiased per-column variance and ``sd = sqrt(var + eps)``.
``VICRegLoss(sim_coeff, std_coeff, cov_coeff, eps)(z1, z2) -> loss`` (0-dim) is differentiable through ONE autograd node;
after a forward ``.inv``, ``.var`` and ``.cov`` hold the three unweighted parts (device scalars) for logging.  With ``eps = 0``
a constant column gives 0 / 0 in its gradient, as the chain of torch ops does.  tests/vicreg_ref.py states the arithmetic."""
import torch
import torch.nn as nn

from ...engine import ops


class _VICRegFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z1, z2, mod):
        z1, z2 = z1.contiguous(), z2.contiguous()
        coeffs = (mod.sim_coeff, mod.std_coeff, mod.cov_coeff)
        loss4, stats, covm = ops.vicreg_fwd(z1, z2, *coeffs, mod.eps)
        mod.inv, mod.var, mod.cov = loss4[1], loss4[2], loss4[3]
        ctx.saved, ctx.coeffs = (z1, z2, stats, covm), coeffs
        return loss4[0].reshape(())

    @staticmethod
    def backward(ctx, g):
        dz1, dz2 = ops.vicreg_bwd(*ctx.saved, *ctx.coeffs, gscale_dev=g.contiguous().reshape(1))
        return dz1, dz2, None


def check_coeffs(what, **kw):
    """-> the values as floats; ValueError for a negative or non-finite one."""
    out = []
    for name, v in kw.items():
        v = float(v)
        if not 0.0 <= v < float('inf'):
            raise ValueError('%s: %s must be non-negative and finite (got %r)' % (what, name, v))
        out.append(v)
    return out


class VICRegLoss(nn.Module):
    def __init__(self, sim_coeff=25., std_coeff=25., cov_coeff=1., eps=1e-4):
        super().__init__()
        self.sim_coeff, self.std_coeff, self.cov_coeff, self.eps = check_coeffs(
            'VICRegLoss', sim_coeff=sim_coeff, std_coeff=std_coeff, cov_coeff=cov_coeff, eps=eps)
        self.inv = self.var = self.cov = None

    def forward(self, z1, z2):
        if z1.dim() != 2 or z1.shape != z2.shape:
            raise ValueError('VICRegLoss: two (N, D) views expected (got %s, %s)' % (tuple(z1.shape), tuple(z2.shape)))
        return _VICRegFn.apply(z1, z2, self)
