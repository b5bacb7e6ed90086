"""Optimiser / LR-schedule factories (reference: lib/solver/build.py:24-71).

``make_optimizer(cfg, model)`` returns a HipSGD, a HipAdam or a HipLARS (SOLVER.OPTIMIZER_NAME 'SGD' | 'Adam' | 'AdamW' |
'LARS') whose
``param_groups`` mirror the reference's (one group PER PARAMETER; names containing "bias" get lr * BIAS_LR_FACTOR and
WEIGHT_DECAY_BIAS), but whose ``step()`` is ONE multi-tensor kernel over the flat parameter arena instead of one
launch per tensor."""
import torch

from .lr_scheduler import WarmupMultiStepLR
from ...engine import ops
from ...engine.arena import CHUNK, arena_of

_FORMATS = 'torch.optim.SGD\'s format (state entries hold `momentum_buffer`) / torch.optim.Adam\'s (`step`, `exp_avg`, `exp_avg_sq`)'


def _state_keys(sd):
    """The per-parameter state keys an optimizer state dict carries (the flat `momentum_buffer` layout of early builds included)."""
    keys = set(k for k in sd if k not in ('state', 'param_groups'))
    for st in (sd.get('state') or {}).values():
        keys.update(st)
    return keys


class _ArenaOptimizer(object):
    """What the fused optimizers share: the arena binding, the per-chunk (lr, weight decay) tables, zero_grad, the clip
    coefficient and the param-group half of torch's wire format."""

    def _bind(self, model, groups):
        self.arena = arena_of(model)
        if len(groups) != len(self.arena.params):
            raise ValueError('one param group per parameter expected')
        self.param_groups = groups

    def _make_tables(self):
        self.chunk_lr = torch.zeros(self.arena.total // CHUNK, dtype=torch.float32, device=self.arena.flat.device)
        self.chunk_wd = torch.zeros_like(self.chunk_lr)
        self._uploaded = None
        self._sync_tables()

    def _table_key(self, g):
        return (g['lr'], g['weight_decay'])

    def _upload_tables(self):
        self.chunk_lr.copy_(self.arena.chunk_table([g['lr'] for g in self.param_groups]), non_blocking=False)
        self.chunk_wd.copy_(self.arena.chunk_table([g['weight_decay'] for g in self.param_groups]))

    def _sync_tables(self):
        key = tuple(self._table_key(g) for g in self.param_groups)
        if key != self._uploaded:
            self._upload_tables()
            self._uploaded = key

    def zero_grad(self, set_to_none=False):
        self.arena.rebind()
        ops.fill(self.arena.grad, 0.0)

    def clip_grad_norm(self, max_norm, out=None):
        """torch.nn.utils.clip_grad_norm_ as the reference applies it between backward and step
        (tools/train_video_contrast_dis.py:420-423), over the flat gradient arena, without a host sync: returns the
        device pair (total_norm, coef); pass it to step(grad_clip=...) -- the gradients themselves are left unscaled."""
        return ops.grad_clip_coef(self.arena.grad, max_norm, out)

    def _per_param(self, flat):
        """{parameter index: copy of its slice of an arena-shaped buffer, in the parameter's shape}"""
        a = self.arena
        return {i: flat[o:o + n].view(p.shape).clone() for i, (o, n, p) in enumerate(zip(a.offsets, a.sizes, a.params))}

    def _groups_out(self):
        return [dict({k: v for k, v in g.items() if k != 'params'}, params=[i]) for i, g in enumerate(self.param_groups)]

    def _groups_merged(self, sd):
        """The param groups as they will be once `sd` is loaded (nothing is changed yet)."""
        if len(sd['param_groups']) != len(self.param_groups):
            raise ValueError('optimizer state has %d param groups, this model needs %d'
                             % (len(sd['param_groups']), len(self.param_groups)))
        return [dict(g, **{k: v for k, v in s_.items() if k != 'params'}) for g, s_ in zip(self.param_groups, sd['param_groups'])]

    def _groups_in(self, merged):
        for g, s_ in zip(self.param_groups, merged):
            g.update(s_)
        self._uploaded = None


class HipSGD(_ArenaOptimizer):
    """torch.optim.SGD semantics (momentum, weight decay, optional nesterov; dampening 0) on the arena."""

    def __init__(self, model, groups, momentum=0.9, nesterov=False):
        self._bind(model, groups)
        for g in groups:
            g.setdefault('initial_lr', g['lr'])
            g.setdefault('momentum', momentum)
            g.setdefault('nesterov', nesterov)
        self.momentum, self.nesterov = momentum, nesterov
        self.buf = torch.zeros_like(self.arena.flat)          # momentum buffers (zero == "first step" semantics)
        self._make_tables()

    def step(self, grad_clip=None):
        """grad_clip: optional device (norm, coef, skip, -) record from clip_grad_norm() / ops.grad_unscale_clip(): the
        coefficient is applied to every gradient inside the update kernel; a set skip flag (non-finite gradient under
        loss scaling) leaves parameters and momentum untouched."""
        self._sync_tables()
        ops.sgd_step(self.arena.flat, self.arena.grad, self.buf, self.chunk_lr, self.chunk_wd, 1.0,
                     self.momentum, self.nesterov, grad_clip)

    def state_dict(self):
        """torch.optim.SGD's wire format (what the reference checkpoints hold, tools/...dis.py:274-286): per-parameter
        `momentum_buffer`s keyed by parameter index, one param group per parameter.  The buffers are copies."""
        state = {i: {'momentum_buffer': b} for i, b in self._per_param(self.buf).items()}
        return {'state': state, 'param_groups': self._groups_out()}

    def load_state_dict(self, sd):
        if _state_keys(sd) & {'exp_avg', 'exp_avg_sq'}:
            raise ValueError('HipSGD loads %s, and was handed the latter' % _FORMATS)
        a = self.arena
        if 'momentum_buffer' in sd:                       # flat layout written by earlier builds of this package
            self.buf.copy_(sd['momentum_buffer'])
        else:
            self.buf.zero_()
            for i, (o, n) in enumerate(zip(a.offsets, a.sizes)):
                st = sd['state'].get(i, sd['state'].get(str(i)))
                if st is not None and st.get('momentum_buffer') is not None:
                    self.buf[o:o + n].copy_(st['momentum_buffer'].reshape(-1))
        self._groups_in(self._groups_merged(sd))
        # the update kernel takes ONE momentum / nesterov setting: re-read it from the loaded groups
        moms = set(float(g.get('momentum', self.momentum)) for g in self.param_groups)
        nest = set(bool(g.get('nesterov', self.nesterov)) for g in self.param_groups)
        if len(moms) != 1 or len(nest) != 1:
            raise NotImplementedError('per-group momentum / nesterov settings are not supported by the fused SGD kernel')
        self.momentum, self.nesterov = moms.pop(), nest.pop()


class HipLARS(_ArenaOptimizer):
    """LARS -- apex LARC(clip=False) around torch.optim.SGD (dampening 0) -- on the arena: every tensor whose group has
    `lars_adapt` set (default: p.ndim > 1, so biases and BatchNorm parameters take plain SGD) scales g + wd * w by its trust
    ratio trust_coef * |w| / (|g| + wd * |w| + lars_eps) before momentum.  Three launches of gca_lars_step, no host sync.
    `trust` (fp32, one per parameter) and `norms` (fp64 (n_params, 2): |w|, |g| with the clip coefficient in) are device
    tensors that every applied step overwrites."""

    def __init__(self, model, groups, momentum=0.9, nesterov=False, trust_coef=0.001, eps=1e-8):
        self._bind(model, groups)
        for g, p in zip(groups, self.arena.params):
            g.setdefault('initial_lr', g['lr'])
            g.setdefault('momentum', momentum)
            g.setdefault('nesterov', nesterov)
            g.setdefault('trust_coef', trust_coef)
            g.setdefault('lars_eps', eps)
            g.setdefault('lars_adapt', p.ndim > 1)
        self.momentum, self.nesterov, self.trust_coef, self.eps = self._settings(groups)
        a = self.arena
        self.buf = torch.zeros_like(a.flat)
        self.plan = ops.LarsPlan(a.offsets, a.sizes, a.total, a.flat.device)
        self.trust, self.norms = self.plan.trust, self.plan.norms
        self._make_tables()

    def _settings(self, gs):
        """The kernels take ONE (momentum, nesterov, trust_coef, lars_eps) setting: read it from the groups `gs`."""
        sets = [set(kind(g[k]) for g in gs) for k, kind in (('momentum', float), ('nesterov', bool), ('trust_coef', float),
                                                           ('lars_eps', float))]
        if any(len(s_) != 1 for s_ in sets):
            raise NotImplementedError('per-group momentum / nesterov / trust_coef / lars_eps settings are not supported by the '
                                      'fused LARS kernels')
        mom, nest, tau, eps = (s_.pop() for s_ in sets)
        if not 0.0 <= mom < 1.0 or not tau > 0.0 or not eps >= 0.0:
            raise ValueError('LARS needs 0 <= momentum < 1, trust_coef > 0, lars_eps >= 0 (got %r, %r, %r)' % (mom, tau, eps))
        return mom, nest, tau, eps

    def _table_key(self, g):
        return (g['lr'], g['weight_decay'], bool(g['lars_adapt']))

    def _upload_tables(self):
        super(HipLARS, self)._upload_tables()
        self.plan.adapt.copy_(torch.tensor([int(bool(g['lars_adapt'])) for g in self.param_groups], dtype=torch.int32))

    def step(self, grad_clip=None):
        """grad_clip: as for HipSGD.step -- the coefficient scales every gradient, inside the trust ratio too; a set skip flag
        leaves parameters, momentum, `trust` and `norms` untouched."""
        self._sync_tables()
        ops.lars_step(self.arena.flat, self.arena.grad, self.buf, self.chunk_lr, self.chunk_wd, self.plan, self.momentum,
                      self.nesterov, self.trust_coef, self.eps, grad_clip)

    def state_dict(self):
        """torch.optim.SGD's wire format, as HipSGD writes it (loads into a torch.optim.SGD over the same parameters); the
        LARS settings ride in the param groups."""
        state = {i: {'momentum_buffer': b} for i, b in self._per_param(self.buf).items()}
        return {'state': state, 'param_groups': self._groups_out()}

    def load_state_dict(self, sd):
        """Its own state, or a plain SGD one (torch's or HipSGD's): groups without the LARS keys keep this optimizer's."""
        if _state_keys(sd) & {'exp_avg', 'exp_avg_sq'}:
            raise ValueError('HipLARS loads %s, and was handed the latter' % _FORMATS)
        merged = self._groups_merged(sd)
        settings = self._settings(merged)                    # refuses before anything is changed
        a = self.arena
        if 'momentum_buffer' in sd:                       # flat layout written by earlier builds of this package
            self.buf.copy_(sd['momentum_buffer'])
        else:
            self.buf.zero_()
            for i, (o, n) in enumerate(zip(a.offsets, a.sizes)):
                st = sd['state'].get(i, sd['state'].get(str(i)))
                if st is not None and st.get('momentum_buffer') is not None:
                    self.buf[o:o + n].copy_(st['momentum_buffer'].reshape(-1))
        self._groups_in(merged)
        self.momentum, self.nesterov, self.trust_coef, self.eps = settings


class HipAdam(_ArenaOptimizer):
    """torch.optim.Adam (decoupled=False) / AdamW (decoupled=True) semantics, amsgrad=False, on the arena: one launch of
    gca_adam_step over parameters, gradients and both moment buffers.  The step count lives on the device (`self.steps`, one
    int64 that a launch behind the update increments), so a captured hipGraph keeps counting."""

    def __init__(self, model, groups, betas=(0.9, 0.999), eps=1e-8, decoupled=False):
        self._bind(model, groups)
        self.betas, self.eps, self.decoupled = (float(betas[0]), float(betas[1])), float(eps), bool(decoupled)
        for g in groups:
            g.setdefault('initial_lr', g['lr'])
            g.setdefault('betas', self.betas)
            g.setdefault('eps', self.eps)
            g.setdefault('amsgrad', False)
            g.setdefault('decoupled_weight_decay', self.decoupled)
        self.betas, self.eps, self.decoupled = self._settings(groups)
        self.exp_avg = torch.zeros_like(self.arena.flat)
        self.exp_avg_sq = torch.zeros_like(self.arena.flat)
        self.steps = torch.zeros(1, dtype=torch.int64, device=self.arena.flat.device)
        self._make_tables()

    def _settings(self, gs):
        """The update kernel takes ONE (betas, eps, decoupled) setting: read it from the groups `gs`."""
        if any(g.get('amsgrad', False) or g.get('maximize', False) for g in gs):
            raise NotImplementedError('amsgrad / maximize are not built into the fused Adam kernel')
        betas = set((float(g['betas'][0]), float(g['betas'][1])) for g in gs)
        eps = set(float(g['eps']) for g in gs)
        dec = set(bool(g.get('decoupled_weight_decay', self.decoupled)) for g in gs)
        if len(betas) != 1 or len(eps) != 1 or len(dec) != 1:
            raise NotImplementedError('per-group betas / eps / decoupled weight decay are not supported by the fused Adam kernel')
        return betas.pop(), eps.pop(), dec.pop()

    def step(self, grad_clip=None):
        """grad_clip: as for HipSGD.step -- the coefficient is applied to every gradient inside the update kernel; a set skip
        flag leaves parameters, both moments and the step count untouched."""
        self._sync_tables()
        ops.adam_step(self.arena.flat, self.arena.grad, self.exp_avg, self.exp_avg_sq, self.chunk_lr, self.chunk_wd,
                      self.betas[0], self.betas[1], self.eps, self.decoupled, self.steps, grad_clip)

    def state_dict(self):
        """torch.optim.Adam's wire format: per parameter index `step` (a float32 scalar, as torch keeps it), `exp_avg`,
        `exp_avg_sq`; one param group per parameter.  Loads into a torch.optim.Adam / AdamW over the same parameters.  Reads
        the device step count (one host sync); the buffers are copies."""
        t = float(int(self.steps))
        m, v = self._per_param(self.exp_avg), self._per_param(self.exp_avg_sq)
        state = {i: {'step': torch.tensor(t, dtype=torch.float32), 'exp_avg': m[i], 'exp_avg_sq': v[i]} for i in m}
        return {'state': state, 'param_groups': self._groups_out()}

    def load_state_dict(self, sd):
        if 'momentum_buffer' in _state_keys(sd):
            raise ValueError('HipAdam loads %s, and was handed the former' % _FORMATS)
        a = self.arena
        entries = [sd['state'].get(i, sd['state'].get(str(i))) for i in range(len(a.params))]
        steps = set(int(float(st['step'])) for st in entries if st)
        if len(steps) > 1:
            raise NotImplementedError('per-parameter step counts %s are not supported by the fused Adam kernel' % sorted(steps))
        merged = self._groups_merged(sd)
        self.betas, self.eps, self.decoupled = self._settings(merged)        # refuses before anything is changed
        self._groups_in(merged)
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        for st, o, n in zip(entries, a.offsets, a.sizes):
            if st:
                self.exp_avg[o:o + n].copy_(st['exp_avg'].reshape(-1))
                self.exp_avg_sq[o:o + n].copy_(st['exp_avg_sq'].reshape(-1))
        self.steps.fill_(steps.pop() if steps else 0)


def clip_value_of(cfg):
    """SOLVER.CLIP_GRADIENT: 'none' (every shipped YAML) or the max 2-norm (tools/train_video_contrast_dis.py:420)."""
    v = getattr(cfg.SOLVER, 'CLIP_GRADIENT', 'none')
    if isinstance(v, str):
        if v.lower() == 'none':
            return None
        v = float(v)
    v = float(v)
    if not v > 0:
        raise ValueError('SOLVER.CLIP_GRADIENT must be "none" or a positive max-norm (got %r)' % (v,))
    return v


OPTIMIZERS = ('SGD', 'Adam', 'AdamW', 'LARS')


def check_optimizer_name(cfg):
    if cfg.SOLVER.OPTIMIZER_NAME not in OPTIMIZERS:
        raise NotImplementedError('SOLVER.OPTIMIZER_NAME %r: %s are built' % (cfg.SOLVER.OPTIMIZER_NAME, ', '.join(OPTIMIZERS)))


def make_optimizer(cfg, model, name_prefix=''):
    """The reference's make_optimizer over `model` (a sub-module whose parameters are the only ones trained: pass its
    place in the whole model as name_prefix -- the group names are then the whole model's).  SGD takes MOMENTUM / NESTEROV;
    Adam / AdamW take the per-parameter lr / weight decay alone, with torch's default betas and eps (reference :57); LARS takes
    MOMENTUM / NESTEROV, LARS_TRUST_COEF and LARS_EPS, and adapts every parameter of more than one dimension."""
    if cfg.SOLVER.USE_TRICK:
        raise NotImplementedError('SOLVER.USE_TRICK (TSN-style policies) is a downstream-only path')
    check_optimizer_name(cfg)
    groups = []
    for key, value in model.named_parameters():
        if not value.requires_grad:
            raise NotImplementedError('frozen parameters are not on the pre-training path')
        lr, wd = cfg.SOLVER.BASE_LR, cfg.SOLVER.WEIGHT_DECAY
        if 'bias' in key:
            lr, wd = cfg.SOLVER.BASE_LR * cfg.SOLVER.BIAS_LR_FACTOR, cfg.SOLVER.WEIGHT_DECAY_BIAS
        groups.append({'params': [value], 'lr': lr, 'weight_decay': wd, 'name': name_prefix + key})
    if cfg.SOLVER.OPTIMIZER_NAME == 'SGD':
        return HipSGD(model, groups, momentum=cfg.SOLVER.MOMENTUM, nesterov=cfg.SOLVER.NESTEROV)
    if cfg.SOLVER.OPTIMIZER_NAME == 'LARS':
        return HipLARS(model, groups, momentum=cfg.SOLVER.MOMENTUM, nesterov=cfg.SOLVER.NESTEROV,
                       trust_coef=cfg.SOLVER.LARS_TRUST_COEF, eps=cfg.SOLVER.LARS_EPS)
    return HipAdam(model, groups, decoupled=cfg.SOLVER.OPTIMIZER_NAME == 'AdamW')


def make_lr_scheduler(cfg, optimizer):
    return WarmupMultiStepLR(optimizer=optimizer, milestones=cfg.SOLVER.STEPS, gamma=cfg.SOLVER.GAMMA,
                             warmup_factor=cfg.SOLVER.WARMUP_FACTOR, warmup_iters=cfg.SOLVER.WARMUP_ITERS,
                             warmup_method=cfg.SOLVER.WARMUP_METHOD, mode=cfg.SOLVER.LR_SCHEDULER,
                             max_epochs=cfg.SOLVER.MAX_EPOCHS)
