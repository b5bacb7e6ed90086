"""fp64 CPU references of the fused layer units of engine/layers.py (conv -> training-mode BatchNorm [+ residual] [-> ReLU]
[-> max pool]), the input builders that make a unit's BACKWARD well-posed, and the table of routes the units can take.
Shared by tests/test_units_ref.py (every precondition, asserted on the CPU from the reference alone) and tests/test_gpu_units.py
(every route on the device against these references).  Nothing of the engine is used here: plain torch in double, differentiated
by autograd.

Why the inputs are special.  A single kernel is linear in (x, dy); a unit is not: one ReLU sign or one pool winner decided the
other way than fp64 moves dW by about 1 / sqrt(M), far above any per-kernel bar.  So every decision is taken out of the inputs:

* The FIRST unit of a case reads dyadic x and w (exact.grid: x = k / 4, w = k / 8, |k| <= 8) whose conv output is the fp64
  answer bit for bit in every arithmetic mode (exact.exact_in_fp32 < 1), and every pre-activation p = y * scale + shift [+ res]
  stays 64 fp32 roundings of its own terms away from zero (`first_unit_margin`): the kernel's ReLU mask IS the reference's.
  Pool windows over such a unit compare values of one channel, p is strictly monotone in y there, so the winner (and an exact
  tie, which goes to the first index) is the reference's too.
* A LATER unit reads rounded numbers.  There the SEED gradient is set to zero, for the device run and the reference alike,
  wherever the reference's decision is closer than m = 16 * (per-kernel forward bar of the arithmetic mode) * max |p|
  (`keep_relu`, `keep_pool`): a decision that flips under a zero seed changes no gradient.  At most 2 % of a seed may go.
"""
import functools

import torch
import torch.nn.functional as F

import exact

F64 = torch.float64
U32 = 2.0 ** -24                    # one fp32 rounding
EPS, MOMENTUM = 1e-5, 0.1           # HipBatchNorm3d's defaults
MODES = ('f32', 'bf16x3', 'bf16x6')
BARS = {'f32': 1e-5, 'bf16x6': 1e-5, 'bf16x3': 5e-5}       # per-kernel forward bars: tests/test_gpu_ops.py, test_gpu_stem_dzf.BARS
F16_BARS = (1.5e-3, 2e-4)           # tests/test_gpu_f16.py: fp16 outputs, fp32 outputs
MARGIN_ROUNDINGS, MARGIN_BARS, SEED_CAP = 64, 16, 0.02

HALO = 2048                         # engine.tune.TUNE_HALO
box = lambda d, h, w: d | h << 8 | w << 16

# ----------------------------------------------------------------------------- geometry of the cases
K333, K133, K311 = ((3, 3, 3), (1, 1, 1), (1, 1, 1)), ((1, 3, 3), (1, 1, 1), (0, 1, 1)), ((3, 1, 1), (1, 1, 1), (1, 0, 0))
KERNELS = {'k333': K333, 'k133': K133}
R1_X, R1_K = (2, 24, 4, 12, 13), 16           # N * SP = 1248, odd W
R6_X = (2, 16, 4, 12, 13)                     # Cin = K: the block's input is its residual
R3_X, R4_X = (2, 8, 4, 64, 65), (2, 8, 4, 64, 68)      # N * SP = 33280 / 34816 > 32768: the producer is lazy
R5_X = (2, 3, 4, 144, 144)                    # stem: (1,7,7)/(1,2,2)/(0,3,3) -> (2,16,4,72,72), N * SP = 41472
STEM = ((1, 7, 7), (1, 2, 2), (0, 3, 3))
POOL_122, POOL_321 = ((1, 3, 3), (1, 2, 2), (0, 1, 1)), ((3, 3, 3), (2, 2, 2), (1, 1, 1))
BN_SMALL_ELEMS = 32768                        # engine.layers: at or below, finalize + apply are one launch and nothing is lazy

# Launch codes pinned on the plan a unit looks up (fields of gca_conv_geom.tune_*), and what the host side of the library must
# resolve them to -- tests/test_units_ref.py asserts this table without a device, the GPU cases assert it again before they run.
#   name -> (x shape, K, (k, s, p), pins, {mode: (fwd kernel, fwd splits, fwd_ws > 0, wgrad kernel, conv_xf_ok, conv_dzf_ok)})
_all = lambda v: {m: v for m in MODES}
_split = lambda v32, v: {'f32': v32, 'bf16x3': v, 'bf16x6': v}
ROUTES = {
    'r1_k333': (R1_X, 16, K333, dict(fwd_bm=64, fwd_splits=1), _all(('gather', 1, False, 'gather', False, False))),
    'r1_k133': (R1_X, 16, K133, dict(fwd_bm=64, fwd_splits=1), _all(('gather', 1, False, 'gather', False, False))),
    'r5_small': (R1_X, 16, K311, dict(fwd_bm=64, fwd_splits=1), _all(('gather', 1, False, 'gather', False, False))),
    'r6_a': (R6_X, 16, K333, dict(fwd_bm=64, fwd_splits=1), _all(('gather', 1, False, 'gather', False, False))),
    'r3_a': (R3_X, 16, K133, dict(), _all(('gather', 1, False, 'gather', False, False))),
    'r4_a': (R4_X, 16, K133, dict(), _all(('gather', 1, False, 'gather', False, False))),
    # a (1,3,3) consumer: the spatial streaming kernel is selected, yet conv_xf_ok stays false -- only the temporal kernels set xf
    'r4_b': ((2, 16, 4, 64, 68), 16, K133, dict(fwd_bm=64 | HALO, fwd_box=box(1, 2, 64), wgrad_tile=13, wgrad_splits=2),
             _split(('halo', 1, False, 'gather', False, False), ('halo', 1, False, 'spatial', False, False))),
    'r5_stem': (R5_X, 16, STEM, dict(wgrad_tile=14),
                _split(('gather', 2, True, 'gather', False, False), ('stem', 1, False, 'stem', False, True))),
    'r5_t': ((2, 16, 4, 72, 72), 16, K311, dict(fwd_bm=64 | HALO, fwd_box=box(1, 2, 64), wgrad_tile=11, wgrad_splits=2),
             _split(('halo', 1, False, 'gather', False, False), ('halo', 1, False, 'temporal32', True, False))),
}
for _sp in (2, 3, 5):
    for _kn, _kk in KERNELS.items():
        ROUTES['r2_%s_s%d' % (_kn, _sp)] = (R1_X, 16, _kk, dict(fwd_bm=64, fwd_splits=_sp), _all(('gather', _sp, True, 'gather', False, False)))
for _b in ((1, 1, 128), (1, 2, 64), (1, 4, 32)):
    for _tile, _kern in ((11, 'temporal32'), (12, 'temporal64')):
        ROUTES['r3_b_%dx%dx%d_t%d' % (_b + (_tile,))] = (
            (2, 16, 4, 64, 65), 24, K311, dict(fwd_bm=64 | HALO, fwd_box=box(*_b), wgrad_tile=_tile, wgrad_splits=2),
            _split(('halo', 1, False, 'gather', False, False), ('halo', 1, False, _kern, True, False)))
R3_B = 'r3_b_1x2x64_t11'            # the pins the GPU cases of R3 / R4 / R9 use for the temporal consumer
K111, K111S2, K333S2 = ((1, 1, 1), (1, 1, 1), (0, 0, 0)), ((1, 1, 1), (2, 2, 2), (0, 0, 0)), ((3, 3, 3), (2, 2, 2), (1, 1, 1))
POOL_311 = ((3, 3, 3), (1, 1, 1), (1, 1, 1))
# R7, the three-branch mini-Mixed over R1's input: 1x1x1 -> 6 | 1x1x1 -> 8, (1,3,3) -> 9 | max pool 3/1/1, 1x1x1 -> 7
MIXED_WIDTHS, MIXED_MID = (6, 9, 7), 8
MIXED_GEOMS = {'b0': (R1_X, 6, K111), 'b1a': (R1_X, MIXED_MID, K111), 'b1b': ((2, MIXED_MID, 4, 12, 13), 9, K133), 'b2': (R1_X, 7, K111)}
for _n, (_x, _k, _ksp) in MIXED_GEOMS.items():
    for _sp in (1, 2):
        ROUTES['r7_%s_s%d' % (_n, _sp)] = (_x, _k, _ksp, dict(fwd_bm=32, fwd_splits=_sp), _all(('gather', _sp, _sp > 1, 'gather', False, False)))
# the real BasicBlock(16, 32, stride=2, downsample) at R6's input: both 3x3x3 convs split, the shortcut does not
ROUTES['r6s_a'] = (R6_X, 32, K333S2, dict(fwd_bm=32, fwd_splits=3), _all(('gather', 3, True, 'gather', False, False)))
ROUTES['r6s_b'] = ((2, 32, 2, 6, 7), 32, K333, dict(fwd_bm=32, fwd_splits=4), _all(('gather', 4, True, 'gather', False, False)))
ROUTES['r6s_s'] = (R6_X, 32, K111S2, dict(fwd_bm=32, fwd_splits=1), _all(('gather', 1, False, 'gather', False, False)))
# SepConv3d(8, 16, 3, 1, 1) at R3's input: conv_s is 'r3_a', conv_t the temporal consumer at 16 channels
ROUTES['sep_t'] = ((2, 16, 4, 64, 65), 16, K311, dict(fwd_bm=64 | HALO, fwd_box=box(1, 2, 64), wgrad_tile=12, wgrad_splits=2),
                   _split(('halo', 1, False, 'gather', False, False), ('halo', 1, False, 'temporal64', True, False)))
SEP_BN = dict(eps=1e-3, momentum=0.001)          # s3d_1._BN


# ----------------------------------------------------------------------------- input builders
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def dyadic_x(shape, seed):
    return exact.grid(shape, 8, 1 / 4, seed)


def dyadic_w(K, C, k, seed):
    return exact.grid((K, C) + tuple(k), 8, 1 / 8, seed)


def bn_params(K, seed):
    """gamma in [0.5, 1.5), beta about 0.3 randn: fp32 numbers, as the module stores them."""
    g = _gen(seed)
    return (torch.rand(K, generator=g) + 0.5).to(F64), (torch.randn(K, generator=g) * 0.3).to(F64)


def rand_w(K, C, k, seed):
    """A later unit's weights: fp32 numbers of the size kaiming_uniform gives."""
    fan = C * k[0] * k[1] * k[2]
    return (torch.randn((K, C) + tuple(k), generator=_gen(seed)) / fan ** 0.5).to(F64)


def randn64(shape, seed, scale=1.0):
    return (torch.randn(tuple(shape), generator=_gen(seed)) * scale).to(F64)


# ----------------------------------------------------------------------------- the reference of one unit
class _Store16(torch.autograd.Function):
    """A tensor kept in HBM as IEEE fp16 (ops.set_conv_math('fp16')): the value is rounded where it is stored, and so is the
    gradient that flows back into it, which lives in an fp16 buffer too."""

    @staticmethod
    def forward(ctx, t):
        return t.float().half().to(F64)

    @staticmethod
    def backward(ctx, g):
        return g.float().half().to(F64)


def store16(t):
    return _Store16.apply(t)


def unit(x, w, gamma, beta, ksp, relu=True, res=None, eps=EPS, momentum=MOMENTUM, store=None):
    """conv3d -> training-mode batch norm written out (biased variance for the output, unbiased for running_var) -> + res ->
    relu.  -> dict of autograd tensors (y, ys = y * scale, p = pre-activation, z) and of the statistics.  `store`: applied to
    y and z where the engine writes them to memory (store16 for the fp16-storage path); everything downstream reads the stored
    tensor, as the kernels do."""
    k, s, p = ksp
    if store is not None:
        # the MFMA operands are fp16: the fp32 master weights are rounded where the kernels load them (conv3d.hip, MATH == 3),
        # forward and dgrad alike; their gradient is an fp32 tensor and is not
        w = w + (store(w.detach()) - w.detach())
    y = F.conv3d(x, w, None, s, p)
    if store is not None:
        y = store(y)
    M = y.numel() // y.shape[1]
    mean = y.mean((0, 2, 3, 4))
    var = ((y - mean.view(1, -1, 1, 1, 1)) ** 2).mean((0, 2, 3, 4))
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    ys = y * scale.view(1, -1, 1, 1, 1)
    pre = ys + shift.view(1, -1, 1, 1, 1)
    if res is not None:
        pre = pre + res
    z = torch.relu(pre) if relu else pre
    if store is not None:
        z = store(z)
    return dict(y=y, ys=ys, p=pre, z=z, res=res, mean=mean, var=var, invstd=invstd, scale=scale, shift=shift, M=M, relu=relu,
                running_mean=momentum * mean.detach(), running_var=(1 - momentum) + momentum * var.detach() * M / (M - 1))


def eval_unit(x, w, gamma, beta, rmean, rvar, ksp, relu=True):
    k, s, p = ksp
    y = F.conv3d(x, w, None, s, p)
    scale = gamma / torch.sqrt(rvar + EPS)
    shift = beta - rmean * scale
    pre = y * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)
    return dict(y=y, z=torch.relu(pre) if relu else pre, scale=scale, shift=shift)


def conv_budget(x, w, ksp):
    """Share of the fp32 integer range the conv of dyadic x (units 1/4) and w (1/8) uses; below 1 the output is exact."""
    k, s, p = ksp
    return exact.exact_in_fp32(F.conv3d(x.abs(), w.abs(), None, s, p), 1 / 32)


def first_unit_margin(u):
    """min over ALL elements of |p| / (64 * 2^-24 * (|y scale| + |shift| + |res| + |p|)): at or above 1, no sum of 64 fp32
    roundings of p's own terms reaches zero.  -> (that minimum, share of elements with p > 0)."""
    pre = u['p'].detach()
    mag = u['ys'].detach().abs() + u['shift'].detach().abs().view(1, -1, 1, 1, 1) + pre.abs()
    if u['res'] is not None:
        mag = mag + u['res'].detach().abs()
    return float((pre.abs() / (MARGIN_ROUNDINGS * U32 * mag)).min()), float((pre > 0).double().mean())


def z_interval(u):
    """Per-element bound on |z_kernel - z_fp64| of a FIRST unit (y exact), from the operations of the kernels
    (bn.hip: bn_finalize_kernel, bn_apply_kernel), counted in fp32 roundings U = 2^-24:
      mean: the fp32 partial sums of exact y are exact (budget asserted), folded in double, stored as float: 1 U.
      var = q / M - mean^2 in double from fp32 partial sums of y^2: a partial is one output tile, at most 256 positions, so its
        chain of fp32 additions is at most 256 long: |dq| <= 256 U q, i.e. |dvar| / var <= 256 U (var + mean^2) / var;
        invstd = (var + eps)^-1/2: half of that, + 1 U stored as float.
      scale = gamma * float(invstd): + 1 U.   shift = beta - float(mean) * scale: 2 U on its larger term + the errors carried in.
      z = y * scale + shift [+ res], relu: 2 U on the largest intermediate [+ 1 U].
    -> tensor of bounds, shape of z."""
    v = lambda t: t.detach().view(1, -1, 1, 1, 1)
    d_scale = 128.0 * (u['var'] + u['mean'] ** 2).detach() / u['var'].detach() + 2.0               # roundings of scale, relative
    ms = (u['mean'] * u['scale']).detach().abs()
    shift_err = v((d_scale + 3.0) * ms + u['shift'].detach().abs() + u['beta'].abs())              # roundings x magnitude
    ys, pre = u['ys'].detach().abs(), u['p'].detach().abs()
    bound = v(d_scale) * ys + shift_err + 2.0 * (ys + v(u['shift']).abs()) + pre
    if u['res'] is not None:
        bound = bound + u['res'].detach().abs() + pre
    return U32 * bound


def keep_relu(pre, bar):
    """1 where the reference's ReLU decision is at least m = 16 * bar * max |p| away from zero."""
    pre = pre.detach()
    return (pre.abs() >= MARGIN_BARS * bar * float(pre.abs().max())).to(F64)


def keep_pool(pre, pool, bar):
    """Per pool window of z = relu(p): 1 where either a positive winner is at least m above zero AND above the runner-up
    POSITION, or every p of the window is at least m below zero (the output is 0 and whichever position receives the gradient,
    the ReLU mask stops it).  m = 16 * bar * max |p|."""
    k, s, pd = pool
    pre = pre.detach()
    m = MARGIN_BARS * bar * float(pre.abs().max())
    q = F.pad(pre, (pd[2], pd[2], pd[1], pd[1], pd[0], pd[0]), value=float('-inf'))
    win = q.unfold(2, k[0], s[0]).unfold(3, k[1], s[1]).unfold(4, k[2], s[2]).reshape(*q.shape[:2], -1, k[0] * k[1] * k[2])
    top = win.topk(2, dim=-1).values
    ok = ((top[..., 0] >= m) & (top[..., 0] - top[..., 1] >= m)) | (top[..., 0] <= -m)
    OD, OH, OW = [(pre.shape[2 + i] + 2 * pd[i] - k[i]) // s[i] + 1 for i in range(3)]
    return ok.view(pre.shape[0], pre.shape[1], OD, OH, OW).to(F64)


def maxpool(z, pool):
    return F.max_pool3d(z, pool[0], pool[1], pool[2])


# ----------------------------------------------------------------------------- the cases
class Case:
    """leaves: name -> fp64 leaf (requires_grad where a gradient is compared); units: name -> unit() record; outs: name ->
    (tensor, keep) with keep(bar) -> 0/1 seed mask or None; first: names of units that read dyadic operands (margin asserted);
    budgets: name -> share of 2^24."""

    def __init__(self, leaves, units, outs, first, budgets, seed):
        self.leaves, self.units, self.outs, self.first, self.budgets, self.seed = leaves, units, outs, first, budgets, seed
        self._grads = {}

    def seeds(self, bar):
        """name -> (seed gradient with the undecided positions zeroed, share zeroed)."""
        out = {}
        for i, (name, (t, keep)) in enumerate(sorted(self.outs.items())):
            g = randn64(t.shape, self.seed + 50 + i)
            mask = keep(bar) if keep is not None else None
            out[name] = (g if mask is None else g * mask, 0.0 if mask is None else 1.0 - float(mask.mean()))
        return out

    def grads_with(self, seeds):
        """seeds: name of an output -> seed gradient.  -> name of a leaf -> d(sum_o <seed_o, out_o>) / d(leaf), in double."""
        names = [n for n, t in self.leaves.items() if t.requires_grad]
        outs = sorted(self.outs)
        gs = torch.autograd.grad([self.outs[o][0] for o in outs], [self.leaves[n] for n in names], [seeds[o] for o in outs],
                                 retain_graph=True)
        return dict(zip(names, gs))

    def grads(self, bar):
        """grads_with the seeds of `bar`; cached per bar."""
        if bar not in self._grads:
            self._grads[bar] = self.grads_with({o: g for o, (g, _) in self.seeds(bar).items()})
        return self._grads[bar]


def _leaf(t):
    return t.clone().requires_grad_(True)


def _unit_leaves(tag, K, C, k, seed, dyadic):
    w = dyadic_w(K, C, k, seed) if dyadic else rand_w(K, C, k, seed)
    gamma, beta = bn_params(K, seed + 1)
    return {'w' + tag: _leaf(w), 'gamma' + tag: _leaf(gamma), 'beta' + tag: _leaf(beta)}


def _run(lv, tag, x, ksp, relu=True, res=None, **bn):
    u = unit(x, lv['w' + tag], lv['gamma' + tag], lv['beta' + tag], ksp, relu, res, **bn)
    u['beta'] = lv['beta' + tag].detach()
    return u


@functools.lru_cache(maxsize=None)
def single(kname, relu, with_res):
    """R1 / R2 / R8: one unit at (2, 24, 4, 12, 13) -> 16 channels, dyadic operands, optional fp32 residual."""
    s = 100 + 10 * sorted(KERNELS).index(kname) + 2 * relu + with_res      # (a seed that broke a precondition would be replaced here)
    ksp = KERNELS[kname]
    lv = {'x': _leaf(dyadic_x(R1_X, s))}
    lv.update(_unit_leaves('A', R1_K, R1_X[1], ksp[0], s + 1, True))
    if with_res:
        lv['res'] = _leaf(randn64((R1_X[0], R1_K) + R1_X[2:], s + 3, 0.5))
    u = _run(lv, 'A', lv['x'], ksp, relu, lv.get('res'))
    return Case(lv, {'A': u}, {'z': (u['z'], None)}, ['A'] if relu else [], {'A': conv_budget(lv['x'].detach(), lv['wA'].detach(), ksp)}, s)


def _producer(x_shape, ksp, s, K=16):
    lv = {'x': dyadic_x(x_shape, s)}                  # a first layer: no gradient wrt the clip
    lv.update(_unit_leaves('A', K, x_shape[1], ksp[0], s + 1, True))
    a = _run(lv, 'A', lv['x'], ksp)
    return lv, a, {'A': conv_budget(lv['x'], lv['wA'].detach(), ksp)}


@functools.lru_cache(maxsize=None)
def chain(name):
    """The two-unit cases.  'r3': lazy (1,3,3) producer -> (3,1,1) consumer.  'r4conv': -> (1,3,3) consumer at W = 68.
    'r4pool': -> max pool (1,3,3)/(1,2,2)/(0,1,1).  'r4both': -> the temporal consumer AND the pool.  'r5': stem -> (3,1,1) conv
    + BatchNorm + ReLU + max pool 3/2/1.  'r5small': one dyadic unit at R1's size into the same pool.  'r6': the residual block
    z = relu(BN_B(conv_B(relu(BN_A(conv_A x)))) + x).  'r6s': the same with a stride-2 main branch and a relu=False 1x1x1 stride-2
    shortcut unit S as the residual (resnet.BasicBlock with downsample).  'sep': s3d_1.SepConv3d(8, 16, 3, 1, 1) at R3's input
    (BatchNorm eps 1e-3, momentum 1e-3).  'mixed': R7's three branches written into channel slices of one buffer."""
    s = 200 + 10 * CHAINS.index(name)
    if name in ('r3', 'r4conv', 'r4pool', 'r4both'):
        lv, a, budgets = _producer(R4_X if name == 'r4conv' else R3_X, K133, s)
        units, outs = {'A': a}, {}
        if name in ('r3', 'r4both'):
            lv.update(_unit_leaves('B', 24, 16, K311[0], s + 5, False))
            b = units['B'] = _run(lv, 'B', a['z'], K311)
            outs['zB'] = (b['z'], lambda bar, b=b: keep_relu(b['p'], bar))
        if name == 'r4conv':
            lv.update(_unit_leaves('B', 16, 16, K133[0], s + 5, False))
            b = units['B'] = _run(lv, 'B', a['z'], K133)
            outs['zB'] = (b['z'], lambda bar, b=b: keep_relu(b['p'], bar))
        if name in ('r4pool', 'r4both'):
            outs['pool'] = (maxpool(a['z'], POOL_122), None)
        return Case(lv, units, outs, ['A'], budgets, s)
    if name == 'r5':
        lv, a, budgets = _producer(R5_X, STEM, s)
        lv.update(_unit_leaves('B', 16, 16, K311[0], s + 5, False))
        b = _run(lv, 'B', a['z'], K311)
        return Case(lv, {'A': a, 'B': b}, {'pool': (maxpool(b['z'], POOL_321), lambda bar: keep_pool(b['p'], POOL_321, bar))}, ['A'], budgets, s)
    if name == 'r5small':
        lv = {'x': _leaf(dyadic_x(R1_X, s))}
        lv.update(_unit_leaves('A', 16, R1_X[1], K311[0], s + 1, True))
        a = _run(lv, 'A', lv['x'], K311)
        return Case(lv, {'A': a}, {'pool': (maxpool(a['z'], POOL_321), None)}, ['A'], {'A': conv_budget(lv['x'].detach(), lv['wA'].detach(), K311)}, s)
    if name == 'r6':
        lv = {'x': _leaf(dyadic_x(R6_X, s))}
        lv.update(_unit_leaves('A', 16, 16, K333[0], s + 1, True))
        lv.update(_unit_leaves('B', 16, 16, K333[0], s + 5, False))
        a = _run(lv, 'A', lv['x'], K333)
        b = _run(lv, 'B', a['z'], K333, True, lv['x'])
        return Case(lv, {'A': a, 'B': b}, {'zB': (b['z'], lambda bar: keep_relu(b['p'], bar))}, ['A'],
                    {'A': conv_budget(lv['x'].detach(), lv['wA'].detach(), K333)}, s)
    if name == 'r6s':
        lv = {'x': _leaf(dyadic_x(R6_X, s))}
        lv.update(_unit_leaves('A', 32, 16, K333S2[0], s + 1, True))
        lv.update(_unit_leaves('S', 32, 16, K111S2[0], s + 3, True))
        lv.update(_unit_leaves('B', 32, 32, K333[0], s + 5, False))
        a = _run(lv, 'A', lv['x'], K333S2)
        sc = _run(lv, 'S', lv['x'], K111S2, False)
        b = _run(lv, 'B', a['z'], K333, True, sc['z'])
        xd = lv['x'].detach()
        return Case(lv, {'A': a, 'S': sc, 'B': b}, {'zB': (b['z'], lambda bar: keep_relu(b['p'], bar))}, ['A'],
                    {'A': conv_budget(xd, lv['wA'].detach(), K333S2), 'S': conv_budget(xd, lv['wS'].detach(), K111S2)}, s)
    if name == 'sep':
        lv = {'x': dyadic_x(R3_X, s)}
        lv.update(_unit_leaves('A', 16, 8, K133[0], s + 1, True))
        lv.update(_unit_leaves('B', 16, 16, K311[0], s + 5, False))
        a = _run(lv, 'A', lv['x'], K133, **SEP_BN)
        b = _run(lv, 'B', a['z'], K311, **SEP_BN)
        return Case(lv, {'A': a, 'B': b}, {'zB': (b['z'], lambda bar: keep_relu(b['p'], bar))}, ['A'],
                    {'A': conv_budget(lv['x'], lv['wA'].detach(), K133)}, s)
    if name == 'mixed':
        lv = {'x': _leaf(dyadic_x(R1_X, s))}
        xd = lv['x'].detach()
        for i, (tag, (xs, K, ksp)) in enumerate(sorted(MIXED_GEOMS.items())):
            lv.update(_unit_leaves(tag, K, xs[1], ksp[0], s + 1 + 2 * i, tag != 'b1b'))
        pooled = maxpool(lv['x'], POOL_311)
        b0, b1a, b2 = _run(lv, 'b0', lv['x'], K111), _run(lv, 'b1a', lv['x'], K111), _run(lv, 'b2', pooled, K111)
        b1b = _run(lv, 'b1b', b1a['z'], K133)
        one = lambda u: torch.ones_like(u['p'].detach())
        keep = lambda bar: torch.cat([one(b0), keep_relu(b1b['p'], bar), one(b2)], 1)
        budgets = {'b0': conv_budget(xd, lv['wb0'].detach(), K111), 'b1a': conv_budget(xd, lv['wb1a'].detach(), K111),
                   'b2': conv_budget(pooled.detach(), lv['wb2'].detach(), K111)}
        return Case(lv, {'b0': b0, 'b1a': b1a, 'b1b': b1b, 'b2': b2}, {'buf': (torch.cat([b0['z'], b1b['z'], b2['z']], 1), keep)},
                    ['b0', 'b1a', 'b2'], budgets, s)
    raise KeyError(name)


CHAINS = ('r3', 'r4conv', 'r4pool', 'r4both', 'r5', 'r5small', 'r6', 'r6s', 'sep', 'mixed')
SINGLES = [(kn, relu, res) for kn in sorted(KERNELS) for relu in (True, False) for res in (False, True)]


@functools.lru_cache(maxsize=None)
def eval_case(kname):
    """R8: the unit of single(kname, True, False) in eval mode, with running statistics that are not the defaults."""
    c = single(kname, True, False)
    g = _gen(c.seed + 9)
    rmean, rvar = (torch.randn(R1_K, generator=g) * 0.5).to(F64), (torch.rand(R1_K, generator=g) * 4 + 2).to(F64)
    lv = c.leaves
    out = eval_unit(lv['x'].detach(), lv['wA'].detach(), lv['gammaA'].detach(), lv['betaA'].detach(), rmean, rvar, KERNELS[kname])
    out.update(rmean=rmean, rvar=rvar)
    return out


# ----------------------------------------------------------------------------- R10: the chain of R3 under fp16 storage
F16_MARGIN_ULPS = 4          # seed margin of the fp16 chain, in fp16 roundings (2^-11) of the largest |y * scale|


@functools.lru_cache(maxsize=None)
def r3_f16():
    """R3's operands through the fp16-STORAGE path, in double: every tensor the engine keeps in HBM (y, z of both units, and on
    the way back dz, dy of both) is rounded to fp16 where it is stored (store16), the weights where the fp16 MFMAs read them (their
    gradient is taken at the rounded value and stays fp32), everything else -- convolution sums,
    statistics, parameter gradients -- is exact.  This is the reference tests/test_gpu_f16.py's bars are declared against
    ("the fp32 result of the fp16-rounded operands, rounded once"), carried through two units.

    Decisions.  y_A is dyadic with at most 11 significant bits, an fp16 number (asserted on the CPU), so A's mask is decided as in
    fp32 storage.  B reads rounded numbers: the kernel's fp32 sum and this double sum can land on either side of an fp16
    rounding boundary, so a stored y_B may differ by ONE fp16 rounding, which moves p by at most 2^-11 |y scale|.  The seed is
    zero wherever |p| < 4 x 2^-11 x max |y scale|.  (The issue's formula, 16 x the per-kernel bar x max |p|, with the fp16 bar
    1.5e-3 would zero a tenth of the seed, five times its own cap.)
    -> dict(A, B: unit records; seed: fp16 numbers; zeroed: share; grads: leaf name -> gradient under storage rounding;
    plain: the same seed through the unrounded fp64 chain of chain('r3'))."""
    c = chain('r3')
    lv = c.leaves
    a = unit(lv['x'], lv['wA'], lv['gammaA'], lv['betaA'], K133, store=store16)
    b = unit(a['z'], lv['wB'], lv['gammaB'], lv['betaB'], K311, store=store16)
    pre = b['p'].detach()
    keep = (pre.abs() >= F16_MARGIN_ULPS * 2.0 ** -11 * float(b['ys'].detach().abs().max())).to(F64)
    seed = (randn64(pre.shape, c.seed + 50) * keep).float().half().to(F64)
    names = [n for n, t in lv.items() if t.requires_grad]
    grads = dict(zip(names, torch.autograd.grad(b['z'], [lv[n] for n in names], seed)))
    return dict(A=a, B=b, seed=seed, zeroed=1.0 - float(keep.mean()), grads=grads, plain=c.grads_with({'zB': seed}))
