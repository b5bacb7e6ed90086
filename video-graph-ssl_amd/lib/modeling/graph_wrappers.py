"""ContrastWrapper / SimSiam / GraphWrapper (reference: lib/modeling/graph_wrappers.py) on the engine, SimCLR (the
reference's ContrastWrapper trained with the in-batch NT-Xent loss; not in the reference) and SwAV (the same wrapper with
learned prototypes and the swapped-prediction loss; not in the reference either) and DINO (the same wrapper with prototypes,
built twice -- student and momentum teacher -- and trained by DINOTrainer; not in the reference either) and MoCoV3 (SimSiam's
encoder + projector + predictor, built twice -- the teacher without the predictor -- and trained by MoCoV3Trainer; not in the
reference either) and NNCLR (the same three modules once, returning projection AND prediction, trained by NNCLRTrainer; not
in the reference either).

``GraphWrapper.forward(x)`` keeps the reference behaviour (MoCo: (b,3,T,H,W) -> (b,FEAT_DIM) unit
rows; SimSiam and SimCLR: (b,6,T,H,W) -> scalar loss) and is differentiable through torch.autograd as ONE
node (engine/autograd_bridge.py); the trainer's fused step calls ``fwd`` directly."""
import torch
import torch.nn as nn

from .project_head import BarlowProjector, PredictionMLP, ProjectHead, ProjectionMLP
from ...engine import layers as L, ops
from ...engine.autograd_bridge import run_module
from ...engine.tape import Tape, Var
from ..memory.vicreg import check_coeffs


class ContrastWrapper(nn.Module):
    def __init__(self, encoder, hid_dim=128, head_type='mlp'):
        super().__init__()
        self.encoder = encoder
        self.proj_head = ProjectHead(encoder.feature_dim, hid_dim, head_type)

    def fwd(self, tape, xv):
        return self.proj_head.fwd(tape, self.encoder.fwd(tape, xv))

    def forward(self, x, bb_grad=True):
        out = run_module(self, x)
        return out if bb_grad else out.detach()


class D(nn.Module):
    """Negative cosine similarity with stop-gradient on the target (graph_wrappers.py:93-108)."""

    def __init__(self, fun_type='v2'):
        super().__init__()
        if fun_type not in ('v1', 'v2'):
            raise ValueError('Unknown type in simsiam D!')
        self.fun_type = fun_type


class SimSiam(nn.Module):
    def __init__(self, encoder, hid_dim=1024):
        super().__init__()
        self.encoder = encoder
        self.feature_dim = encoder.feature_dim
        self.projection = ProjectionMLP(self.feature_dim, hid_dim, hid_dim)
        self.prediction = PredictionMLP(hid_dim, hid_dim // 2, hid_dim)
        self.d = D()

    def fwd(self, tape, xv):
        """loss = D(p1, sg z2)/2 + D(p2, sg z1)/2 with both views through the encoder WITH grad (:48-71)."""
        x = xv.t
        x1, x2 = torch.chunk(x, 2, dim=1)          # views, read in place through the batch stride
        z1 = self.projection.fwd(tape, self.encoder.fwd(tape, Var(x1)))
        p1 = self.prediction.fwd(tape, z1)
        z2 = self.projection.fwd(tape, self.encoder.fwd(tape, Var(x2)))
        p2 = self.prediction.fwd(tape, z2)
        b = p1.t.shape[0]
        loss = torch.empty(1 + b, dtype=torch.float32, device=x.device)
        dp1 = ops.negcos(p1.t, z2.t, 0.5, loss, accumulate=False)
        dp2 = ops.negcos(p2.t, z1.t, 0.5, loss, accumulate=True)
        lv = Var(loss[:1], tape.recording)

        def back():
            # d loss / d p (already scaled by 1/2 and 1/b); upstream scalar gradient folds in here
            g = lv.grad
            if g is not None:
                gs = float(g.item()) if g.numel() == 1 and not torch.cuda.is_current_stream_capturing() else 1.0
                if gs != 1.0:
                    ops.scale_(dp1, gs)
                    ops.scale_(dp2, gs)
            st = ops.LOSS_SCALE_STATE[0]
            if st is not None:                       # fp16 storage: the loss gradient is seeded x the (device-resident) loss scale
                ops.scale_dev_(dp1, st)
                ops.scale_dev_(dp2, st)
            p1.add_grad(dp1)
            p2.add_grad(dp2)
        tape.record(back)
        return lv

    def forward(self, x):
        return run_module(self, x).reshape(())


class SimCLR(ContrastWrapper):
    """ContrastWrapper (encoder + projection head + Normalize) trained with NT-Xent on the two views of a (b,6,T,H,W) batch.
    No parameters or buffers of its own: the state dict is ContrastWrapper's (``encoder.*``, ``proj_head.*``), so every
    loader of MoCo checkpoints reads it.  The views go through encoder + head in TWO passes, so BatchNorm statistics are per
    view (as in this package's SimSiam and in MoCo v3), not over the concatenated 2b clips as in SimCLR's own code."""

    def __init__(self, encoder, hid_dim=128, head_type='mlp', T=0.07):
        super().__init__(encoder, hid_dim, head_type)
        T = float(T)
        if not T > 0:
            raise ValueError('SimCLR: the temperature must be positive (got %r)' % T)
        self.T, self.rank = T, None          # rank: per row, the negatives that score at least the positive (last forward)

    def fwd(self, tape, xv):
        """loss = NT-Xent(z1, z2) over the N = 2b rows, both views through the encoder WITH grad."""
        x = xv.t
        x1, x2 = torch.chunk(x, 2, dim=1)          # views, read in place through the batch stride
        z1 = ContrastWrapper.fwd(self, tape, Var(x1))
        z2 = ContrastWrapper.fwd(self, tape, Var(x2))
        b, dim = z1.t.shape
        z = torch.empty((2 * b, dim), dtype=torch.float32, device=x.device)
        z[:b].copy_(z1.t)
        z[b:].copy_(z2.t)
        inv_T = 1.0 / self.T
        loss, lse, self.rank = ops.ntxent_fwd(z, inv_T, want_rank=True)
        lv = Var(loss, tape.recording)

        def back():
            # d loss / d z in one launch pair; the upstream scalar and the fp16-storage loss scale fold into its scale
            g = lv.grad
            gs = 1.0
            if g is not None and g.numel() == 1 and not torch.cuda.is_current_stream_capturing():
                gs = float(g.item())
            dz = ops.ntxent_bwd(z, lse, inv_T, gscale_dev=ops.LOSS_SCALE_STATE[0], gscale_host=gs)
            z1.add_grad(dz[:b])                      # the two halves of one buffer: no copy
            z2.add_grad(dz[b:])
        tape.record(back)
        return lv

    def forward(self, x):
        return run_module(self, x).reshape(())


def _two_view_loss(model, tape, xv, loss_fwd, loss_bwd, fwd_args, bwd_args):
    """The step that BarlowTwins and VICReg share: both views of a (b,6,T,H,W) batch through model.encoder + model.projection
    in two passes, then one fused loss pair of engine.ops on the two (N, D) feature matrices: ``loss_fwd(z1, z2, *fwd_args) ->
    (parts, *saved)`` with the loss in parts[0], and on the way back ``loss_bwd(z1, z2, *saved, *bwd_args, gscale_dev,
    gscale_host) -> (dz1, dz2)``.  -> (the loss Var, parts)."""
    x = xv.t
    x1, x2 = torch.chunk(x, 2, dim=1)          # views, read in place through the batch stride
    z1 = model.projection.fwd(tape, model.encoder.fwd(tape, Var(x1)))
    z2 = model.projection.fwd(tape, model.encoder.fwd(tape, Var(x2)))
    a, b = z1.t.contiguous(), z2.t.contiguous()
    parts, *saved = loss_fwd(a, b, *fwd_args)
    lv = Var(parts[:1], tape.recording)

    def back():
        # d loss / d (z1, z2) in one launch; the upstream scalar and the fp16-storage loss scale fold into its scale
        g = lv.grad
        gs = 1.0
        if g is not None and g.numel() == 1 and not torch.cuda.is_current_stream_capturing():
            gs = float(g.item())
        dz1, dz2 = loss_bwd(a, b, *saved, *bwd_args, gscale_dev=ops.LOSS_SCALE_STATE[0], gscale_host=gs)
        z1.add_grad(dz1)
        z2.add_grad(dz2)
    tape.record(back)
    return lv, parts


class BarlowTwins(nn.Module):
    """Encoder + BarlowProjector trained with the Barlow Twins loss on the two views of a (b,6,T,H,W) batch (state dict:
    ``encoder.*``, ``projection.*``, as SimSiam's without the predictor).  The views go through encoder + projector in TWO
    passes, so BatchNorm statistics are per view, as in this package's SimSiam and SimCLR.  The loss is unscaled (the
    original code multiplies it by a constant that LARS' trust ratio cancels)."""

    def __init__(self, encoder, hid_dim=1024, lambd=0.0051, eps=1e-5):
        super().__init__()
        lambd = float(lambd)
        if not 0.0 <= lambd < float('inf'):
            raise ValueError('BarlowTwins: lambd must be non-negative and finite (got %r)' % lambd)
        self.encoder = encoder
        self.feature_dim = encoder.feature_dim
        self.projection = BarlowProjector(self.feature_dim, hid_dim, hid_dim)
        self.lambd, self.eps = lambd, float(eps)
        self.on_diag = self.off_diag = None     # the two sums of the last forward (device scalars)

    def fwd(self, tape, xv):
        """loss = on + lambd * off of the views' cross-correlation, both views through the encoder WITH grad."""
        lv, loss3 = _two_view_loss(self, tape, xv, ops.barlow_fwd, ops.barlow_bwd, (self.lambd, self.eps), (self.lambd,))
        self.on_diag, self.off_diag = loss3[1:2], loss3[2:3]
        return lv

    def forward(self, x):
        return run_module(self, x).reshape(())


class VICReg(nn.Module):
    """Encoder + expander trained with the VICReg loss on the two views of a (b,6,T,H,W) batch (state dict: ``encoder.*``,
    ``projection.*``).  VICReg's expander -- two Linear-BN-ReLU layers and a bare last Linear -- is BarlowProjector.  The views
    go through encoder + expander in TWO passes, so BatchNorm statistics are per view, as in this package's other two-view
    objectives."""

    def __init__(self, encoder, hid_dim=1024, sim_coeff=25.0, std_coeff=25.0, cov_coeff=1.0, eps=1e-4):
        super().__init__()
        self.sim_coeff, self.std_coeff, self.cov_coeff, self.eps = check_coeffs(
            'VICReg', sim_coeff=sim_coeff, std_coeff=std_coeff, cov_coeff=cov_coeff, eps=eps)
        self.encoder = encoder
        self.feature_dim = encoder.feature_dim
        self.projection = BarlowProjector(self.feature_dim, hid_dim, hid_dim)
        self.inv = self.var = self.cov = None   # the three unweighted parts of the last forward (device scalars)

    def fwd(self, tape, xv):
        """loss = sim inv + std varl + cov covl of the two views' features, both views through the encoder WITH grad."""
        coeffs = (self.sim_coeff, self.std_coeff, self.cov_coeff)
        lv, loss4 = _two_view_loss(self, tape, xv, ops.vicreg_fwd, ops.vicreg_bwd, coeffs + (self.eps,), coeffs)
        self.inv, self.var, self.cov = loss4[1:2], loss4[2:3], loss4[3:4]
        return lv

    def forward(self, x):
        return run_module(self, x).reshape(())


class Prototypes(nn.Module):
    """SwAV's K prototype vectors: a plain (K, dim) parameter with unit rows, drawn as nn.Linear's weight and normalised."""

    def __init__(self, dim, K):
        super().__init__()
        w = nn.Linear(dim, K, bias=False).weight.detach()
        self.weight = nn.Parameter(w / w.norm(dim=1, keepdim=True))


class SwAV(ContrastWrapper):
    """ContrastWrapper (encoder + projection head + Normalize) and K learned prototypes, trained with SwAV's swapped-prediction
    loss on the two views of a (b,6,T,H,W) batch (state dict: ``encoder.*``, ``proj_head.*``, ``prototypes.weight``, so every
    loader of MoCo / SimCLR checkpoints reads the encoder).  The views go through encoder + head in TWO passes, so BatchNorm
    statistics are per view, as in this package's other two-view objectives.  No multi-crop, no feature queue and no frozen
    prototypes."""

    def __init__(self, encoder, hid_dim=128, head_type='mlp', K=3000, eps=0.05, T=0.1, iters=3):
        super().__init__(encoder, hid_dim, head_type)
        self.eps, self.T, self.iters = ops.swav_params('SwAV', eps, T, iters)
        if isinstance(K, bool) or int(K) != K or not 2 <= int(K) <= 65536:
            raise ValueError('SwAV: the number of prototypes must lie in [2, 65536] (got %r)' % (K,))
        self.prototypes = Prototypes(hid_dim, int(K))
        self.l12 = self.l21 = None              # the two swapped terms of the last forward (device scalars)

    def fwd(self, tape, xv):
        """loss = (l12 + l21) / 2 of the two views' scores against the prototypes, both views through the encoder WITH grad.
        A recording forward first renormalises the prototype rows in place, as the authors' training loop does before every
        step."""
        C = self.prototypes.weight
        if tape.recording:
            ops.rows_normalize_(C.data)
        x = xv.t
        x1, x2 = torch.chunk(x, 2, dim=1)          # views, read in place through the batch stride
        z1 = ContrastWrapper.fwd(self, tape, Var(x1))
        z2 = ContrastWrapper.fwd(self, tape, Var(x2))
        a, b = z1.t.contiguous(), z2.t.contiguous()
        parts, dS = ops.swav_fwd(a, b, C.data, self.eps, self.T, self.iters)
        self.l12, self.l21 = parts[1:2], parts[2:3]
        lv = Var(parts[:1], tape.recording)

        def back():
            # d loss / d (z1, z2, C) in two launches; the upstream scalar and the fp16-storage loss scale fold into their scale
            g = lv.grad
            gs = 1.0
            if g is not None and g.numel() == 1 and not torch.cuda.is_current_stream_capturing():
                gs = float(g.item())
            dz1, dz2 = ops.swav_bwd(a, b, C.data, dS, L._grad_of(C), True, gscale_dev=ops.LOSS_SCALE_STATE[0], gscale_host=gs)
            z1.add_grad(dz1)
            z2.add_grad(dz2)
        tape.record(back)
        return lv

    def forward(self, x):
        return run_module(self, x).reshape(())


class DINO(ContrastWrapper):
    """ContrastWrapper (encoder + projection head + Normalize) and K prototypes: the student, and in a second instance of the
    same layout the momentum teacher, of DINO's self-distillation (state dict: ``encoder.*``, ``proj_head.*``,
    ``prototypes.weight``, so every loader of MoCo / SimCLR checkpoints reads the encoder).  ``forward(x)`` / ``fwd`` are
    ContrastWrapper's: (b,3,T,H,W) -> (b, hid_dim) unit rows; the loss (lib.memory.dino.DINOLoss, csrc/dino.hip) needs both
    instances and lives in the trainer.  The paper's GELU / bottleneck head and the weight-normalised last layer are not built:
    the existing ProjectHead + Normalize feeds unit-row prototypes that the trainer renormalises before every step."""

    def __init__(self, encoder, hid_dim=128, head_type='mlp', K=4096):
        super().__init__(encoder, hid_dim, head_type)
        if isinstance(K, bool) or int(K) != K or not 2 <= int(K) <= 65536:
            raise ValueError('DINO: the number of prototypes must lie in [2, 65536] (got %r)' % (K,))
        self.prototypes = Prototypes(hid_dim, int(K))


class MoCoV3(nn.Module):
    """Encoder + projector (+ predictor): the student, and built with ``predictor=False`` the momentum teacher, of MoCo v3
    (Chen, Xie, He 2021).  Modules in this registration order: ``encoder``, ``projection = ProjectionMLP(feature_dim, hid_dim,
    out_dim)`` and, for the student, ``prediction = PredictionMLP(out_dim, hid_dim, out_dim)`` -- the teacher's parameters are
    then exactly the leading ones of the student's, which MoCoV3Trainer's one-launch EMA relies on.  The state-dict names are
    SimSiam's (``encoder.*``, ``projection.*``, ``prediction.*``), so SimSiam checkpoints and every encoder loader read it.
    ``forward(x)`` / ``fwd``: one view (b,3,T,H,W) -> (b, out_dim) unit rows (predictor outputs for the student, projector outputs
    for the teacher); the loss (lib.memory.mocov3.MoCoV3Loss, csrc/mocov3.hip) needs both instances and lives in the trainer.
    Deviation from the paper: the projector's last BatchNorm keeps its affine parameters (ProjectionMLP as it is)."""

    def __init__(self, encoder, out_dim=256, hid_dim=4096, predictor=True):
        super().__init__()
        for name, v in (('out_dim', out_dim), ('hid_dim', hid_dim)):
            if isinstance(v, bool) or int(v) != v or int(v) < 1:
                raise ValueError('MoCoV3: %s must be a positive integer (got %r)' % (name, v))
        self.encoder = encoder
        self.feature_dim = encoder.feature_dim
        self.projection = ProjectionMLP(self.feature_dim, int(hid_dim), int(out_dim))
        if predictor:
            self.prediction = PredictionMLP(int(out_dim), int(hid_dim), int(out_dim))
        self.has_predictor = bool(predictor)

    def fwd(self, tape, xv):
        z = self.projection.fwd(tape, self.encoder.fwd(tape, xv))
        if self.has_predictor:
            z = self.prediction.fwd(tape, z)
        return L.f_l2norm(tape, z)

    def forward(self, x):
        return run_module(self, x)


class NNCLR(nn.Module):
    """Encoder + projector + predictor of NNCLR (Dwibedi et al. 2021).  Modules in MoCoV3's registration order: ``encoder``,
    ``projection = ProjectionMLP(feature_dim, hid_dim, out_dim)``, ``prediction = PredictionMLP(out_dim, hid_dim, out_dim)``;
    the state-dict names are SimSiam's (``encoder.*``, ``projection.*``, ``prediction.*``), so SimSiam checkpoints and every
    encoder loader read it.  ``fwd_zp(tape, xv)``: one view (b,3,T,H,W) -> (z, p), the projection (what the support set holds and
    the search uses) and the prediction, both (b, out_dim) unit rows; ``fwd`` / ``forward(x)`` give p.  The loss
    (lib.memory.nnclr.NNCLRLoss, csrc/nnclr.hip) owns the support set and lives in the trainer.  Deviations from the paper: the
    predictor shares the projector's hidden width, and the projector's last BatchNorm keeps its affine parameters."""

    def __init__(self, encoder, out_dim=256, hid_dim=2048):
        super().__init__()
        for name, v in (('out_dim', out_dim), ('hid_dim', hid_dim)):
            if isinstance(v, bool) or int(v) != v or int(v) < 1:
                raise ValueError('NNCLR: %s must be a positive integer (got %r)' % (name, v))
        self.encoder = encoder
        self.feature_dim = encoder.feature_dim
        self.projection = ProjectionMLP(self.feature_dim, int(hid_dim), int(out_dim))
        self.prediction = PredictionMLP(int(out_dim), int(hid_dim), int(out_dim))

    def fwd_zp(self, tape, xv):
        z = self.projection.fwd(tape, self.encoder.fwd(tape, xv))
        p = self.prediction.fwd(tape, z)
        # z is used detached (the arg-max of the search has no gradient): its normalisation stays off the tape
        return L.f_l2norm(Tape(False), z), L.f_l2norm(tape, p)

    def fwd(self, tape, xv):
        return self.fwd_zp(tape, xv)[1]

    def forward(self, x):
        return run_module(self, x)


class GraphWrapper(nn.Module):
    def __init__(self, encoder, hid_dim=1024, head_type='mlp', mem_type='simsiam', nce_t=0.07, bt_lambda=0.0051,
                 vic_coeffs=(25.0, 25.0, 1.0), swav_args=(3000, 0.05, 0.1, 3), dino_k=4096, v3_hid=4096, v3_predictor=True,
                 nn_hid=2048):
        super().__init__()
        if mem_type == 'simsiam':
            self.model = SimSiam(encoder=encoder, hid_dim=hid_dim)
        elif mem_type == 'simclr':
            self.model = SimCLR(encoder=encoder, hid_dim=hid_dim, head_type=head_type, T=nce_t)
        elif mem_type == 'barlow':
            self.model = BarlowTwins(encoder=encoder, hid_dim=hid_dim, lambd=bt_lambda)
        elif mem_type == 'vicreg':
            self.model = VICReg(encoder, hid_dim, *vic_coeffs)
        elif mem_type == 'swav':
            self.model = SwAV(encoder, hid_dim, head_type, *swav_args)
        elif mem_type == 'dino':
            self.model = DINO(encoder, hid_dim, head_type, dino_k)
        elif mem_type == 'mocov3':
            self.model = MoCoV3(encoder, hid_dim, v3_hid, predictor=v3_predictor)
        elif mem_type == 'nnclr':
            self.model = NNCLR(encoder, hid_dim, nn_hid)
        else:
            self.model = ContrastWrapper(encoder=encoder, hid_dim=hid_dim, head_type=head_type)

    def fwd(self, tape, xv):
        return self.model.fwd(tape, xv)

    def forward(self, x):
        return self.model(x)
