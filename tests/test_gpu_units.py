"""Every route of the fused layer units (engine/layers.py: f_conv_bn_act, f_conv_bn_relu_maxpool, _conv_input, f_concat, the pool
and residual plumbing; engine/tape.py: Var.grad_buffer, LazyVar) against the fp64 references of tests/units_ref.py, forward AND
backward, with the exact sequence of ops.* calls of each route asserted by a spy.

What makes a unit's backward comparable with fp64 at per-kernel bars is in the inputs, not in the bars: see tests/units_ref.py
(dyadic first units whose every ReLU decision is 64 roundings clear of zero; zeroed seeds where a later unit's decision is
closer than 16 bars) and tests/test_units_ref.py, which asserts all of it on the CPU.

Bars.  Forward: first-unit y bit-equal to the fp64 conv; first-unit z per element inside units_ref.z_interval (derived from the
operation counts of bn.hip); statistics and later-unit y / z within the mode's per-kernel bar (1e-5 f32 and bf16x6, 5e-5 bf16x3)
by conftest.rel_err.  Backward: n x that bar, n = the number of kernels between the seed and the tensor (given per case).
Route against route: torch.equal where two routes run the same kernels on the same bits (lazy vs LAZY_BN off above 32768
positions, xf vs materialised, deferred vs immediate reduce); where the kernels differ (fused small-BatchNorm vs eager, dzf vs
bn_bwd) the fused route's fp64 error is at most 1.5 x the unfused route's on the same inputs.

fp16 storage (R10) is held to units_ref.r3_f16, the same double arithmetic rounding to fp16 where the engine stores: forward at
1.5e-3 / 2e-4, every gradient at n x 2e-4; and to the unrounded chain at n x 1.5e-3 (see the test for why not tighter).
Not run: `out=` combined with a residual -- no model does it, and ops.bn_bwd takes ONE slice stride, for dz, so a strided z
under mask mode 1 has no form.

MEASURED on an MI355X: the worst rel_err of each route and mode as a share of ITS bar (n x per-kernel bar), and the tensor it
was; every test prints all its figures as MEASURED lines, the module's finaliser prints this table.  100 cases, 13 s.
  route            f32                   bf16x3                bf16x6
  R1               2.7e-07 .01 dx        2.9e-06 .03 dx        2.1e-07 .01 dW
  R2               2.8e-07 .01 dW        2.9e-06 .03 dx        2.1e-07 .01 dW        (out= slices: 2.6e-07 / 2.7e-06 / 2.1e-07)
  R2 -> R1         2.8e-07 .01 dW        2.9e-06 .03 dx        1.2e-07 .01 z
  R3 (and R9)      3.6e-06 .18 dW_B      7.3e-06 .15 y_B       2.4e-06 .08 dbeta_A
  R4 pool          3.7e-07 .01 dW_A      2.5e-06 .02 dW_A      3.3e-07 .01 dW_A
  R4 spatial       2.7e-06 .14 dW_B      7.7e-06 .15 y_B       3.4e-06 .11 dbeta_A
  R4 two readers   2.5e-06 .12 dW_B      1.0e-05 .21 z_B       1.7e-06 .09 dW_B
  R5               2.6e-06 .09 dW_B      9.2e-06 .18 y_B       2.2e-06 .07 dW_B      (STEM_DZF off: the same figures)
  R5 direct        2.9e-07 .01 dW        2.8e-06 .02 dW        4.8e-08 .00 running_var
  R6               5.9e-07 .06 y_B       5.6e-06 .11 dgamma_B  6.0e-07 .06 y_B
  R6 BasicBlock    2.9e-07 .03 y_B       5.3e-06 .11 dgamma_B  4.8e-07 .05 y_B       (FUSE_SPLITK_BN off: 2.4e-07 / 5.2e-06 / 4.8e-07)
  R7 (all four)    4.2e-06 .21 dW_b2     9.7e-06 .19 z_b1b     2.7e-06 .13 dW_b2
  R8               7.7e-08 .01 z         7.7e-08 .00 z         7.7e-08 .01 z
  R8 lazy -> eval  2.6e-07 .03 z_B       7.3e-06 .15 y_B       2.4e-07 .02 y_B
  SepConv3d        4.3e-06 .22 dW_B      7.9e-06 .16 dgamma_B  2.0e-06 .10 dW_B
  R10 (fp16), against the fp16-storage reference: y_A 0, z_A 1.5e-04, y_B 4.5e-04, z_B 5.8e-04 (.38 of 1.5e-3); statistics at most
                   4.7e-06 (.02 of 2e-4); dgamma_B 4.0e-05 (.20 of 2e-4), dbeta_B 2.5e-08, dW_B 7.9e-05 (.20 of 4e-4), dgamma_A 1.1e-04
                   (.18 of 6e-4), dbeta_A 8.7e-05 (.15), dW_A 7.7e-05 (.10 of 8e-4); against the unrounded chain 3.3e-04 .. 4.2e-04
                   (at most .22 of n x 1.5e-3)
  first-unit z, worst element as a share of its own interval (288 tensors): median 0.14, largest 0.25
"""
import inspect
import math

import pytest
import torch
import torch.nn as nn

import units_ref as U
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NAN = float('nan')


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
    """Every case here is a valid call.  Should a kernel fault all the same, nothing more is started on that device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit('GPU error after a test of test_gpu_units.py: %s' % e, returncode=3)


SPIED = ('conv_fwd', 'conv_fwd_xf', 'conv_bn_small_fwd', 'bn_finalize', 'bn_train_fwd', 'bn_apply', 'bn_fold_eval', 'bn_bwd',
         'bn_bwd_sums', 'conv_wgrad', 'conv_wgrad_dzf', 'conv_dgrad', 'maxpool_fwd', 'maxpool_bwd')


def _token(name, p):
    """The call as the route tables below spell it, from its arguments BY PARAMETER NAME (p: inspect.Signature.bind of the real
    function, defaults applied -- a renamed or dropped parameter is a KeyError here, not a mislabelled call): bn_bwd with its
    mask mode (0 none, 1 from z, 2 recomputed from y), '+res' when it writes a residual gradient and ':acc' when it adds to it;
    conv_wgrad ':xf'; conv_dgrad / maxpool_bwd ':new' (first writer of the buffer), ':acc' or ':own' (allocates its result);
    ':out' when the BatchNorm writes into a caller's slice."""
    if name == 'bn_bwd':
        return 'bn_bwd:%d%s%s' % (int(p['relu']), '+res' if p['dres'] is not None else '', ':acc' if p['dres_accumulate'] else '')
    if name == 'conv_wgrad':
        return 'conv_wgrad:xf' if p['xf'] is not None else 'conv_wgrad'
    if name in ('conv_dgrad', 'maxpool_bwd'):
        return '%s:%s' % (name, 'own' if p['dx'] is None else ('acc' if p['accumulate'] else 'new'))
    if name in ('bn_train_fwd', 'conv_bn_small_fwd', 'bn_apply') and p['out'] is not None:
        return name + ':out'
    return name


class Engine:
    def __init__(self, pkg, monkeypatch):
        self.pkg, self.mp = pkg, monkeypatch
        self.ops, self.layers, self.tape = pkg.engine.ops, pkg.engine.layers, pkg.engine.tape
        self.calls = []
        for name in SPIED:
            monkeypatch.setattr(self.ops, name, self._spy(name, getattr(self.ops, name)))
        for mod, flag in ((self.layers, 'LAZY_BN'), (self.ops, 'FUSE_SPLITK_BN'), (self.ops, 'STEM_DZF')):
            monkeypatch.setattr(mod, flag, True)
        self.mode = None

    def _spy(self, name, real):
        sig = inspect.signature(real)

        def call(*a, **k):
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            ret = real(*a, **k)
            self.calls.append((_token(name, bound.arguments), ret))
            return ret
        return call

    def reset(self):
        del self.calls[:]

    def names(self):
        return [c[0] for c in self.calls]

    def set_mode(self, mode):
        self.ops.set_conv_math(mode)
        self.mode = mode

    def flag(self, name, value):
        self.mp.setattr(self.layers if name == 'LAZY_BN' else self.ops, name, value)

    def pin(self, route):
        """Pin the launch codes of U.ROUTES[route] on the plan the layer will look up, and hold the library to the table."""
        shape, K, (k, s, p), pins, want = U.ROUTES[route]
        plan = self.ops.conv_plan(shape, K, k, s, p, DEV)
        plan.tuned = [True, True, True]
        for f, v in pins.items():
            setattr(plan.g, 'tune_' + f, v)
        plan.refresh()
        got = (plan.kernel(0), plan.cfg(0)[2], plan.fwd_ws > 0, plan.kernel(2), self.ops.conv_xf_ok(plan), self.ops.conv_dzf_ok(plan))
        assert got == want[self.mode], (route, self.mode, got)
        return plan

    def unit(self, lv, tag, ksp, **bn_kw):
        w = lv['w' + tag].detach()
        conv = self.layers.HipConv3d(w.shape[1], w.shape[0], *ksp).to(DEV)
        bn = self.layers.HipBatchNorm3d(w.shape[0], **bn_kw).to(DEV)
        load(conv, bn, lv, tag)
        return conv, bn


def load(conv, bn, lv, tag):
    with torch.no_grad():
        conv.weight.copy_(f32(lv['w' + tag]))
        bn.weight.copy_(f32(lv['gamma' + tag]))
        bn.bias.copy_(f32(lv['beta' + tag]))


@pytest.fixture()
def eng(pkg, monkeypatch):
    e = Engine(pkg, monkeypatch)
    default = e.ops.get_conv_math()
    e.ops._conv_plan.cache_clear()
    yield e
    e.ops.DEFER[0] = None
    e.ops.set_conv_math(default)
    e.ops._conv_plan.cache_clear()          # the pinned plans are shared per geometry: none survives the test


def f32(t):
    return t.detach().float().to(DEV)


def nan_like(shape, off4=False):
    """A NaN-filled fp32 tensor; off4: starting 4 bytes into its allocation (4-byte aligned, not 16)."""
    n = math.prod(shape)
    if not off4:
        return torch.full(tuple(shape), NAN, device=DEV)
    raw = torch.full((n + 8,), NAN, device=DEV)
    v = raw[1:1 + n].view(tuple(shape))
    assert v.data_ptr() % 16 == 4
    return v


def unit_records(calls):
    """The spy's returns grouped per unit, in forward order: [dict(y, mean, invstd)]."""
    recs = []
    for tok, ret in calls:
        n = tok.split(':')[0]
        if n in ('conv_fwd', 'conv_fwd_xf'):
            recs.append(dict(y=ret[0] if isinstance(ret, tuple) else ret))
        elif n == 'conv_bn_small_fwd':
            recs.append(dict(y=ret[0], mean=ret[2], invstd=ret[3]))
        elif n == 'bn_finalize':
            recs[-1].update(mean=ret[0], invstd=ret[1])
        elif n == 'bn_train_fwd':
            recs[-1].update(mean=ret[1], invstd=ret[2])
    return recs


def param_grads(units):
    out = {}
    for tag, (conv, bn) in units.items():
        out.update({'w' + tag: conv.weight.grad, 'gamma' + tag: bn.weight.grad, 'beta' + tag: bn.bias.grad})
    assert all(g is not None for g in out.values()), [n for n, g in out.items() if g is None]
    return {n: g.clone() for n, g in out.items()}


WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _worst_errors_per_route():
    """After the module's last case: the worst measured error per route and mode of whatever ran (what the docstring lists)."""
    yield
    for (route, mode), (what, err, bar) in sorted(WORST.items()):
        print('MEASURED WORST %-16s %-7s %.3e = %.2f of its bar %.1e (%s)' % (route, mode, err, err / bar, bar, what))


def note(route, mode, what, err, bar):
    print('MEASURED %s %s %s: %.3e (bar %.3e)' % (route, mode, what, err, bar))
    key = (route, mode)
    if key not in WORST or err / bar > WORST[key][1] / WORST[key][2]:
        WORST[key] = (what, err, bar)
    assert err == err, (route, mode, what)           # a NaN is an element nobody wrote
    return err


def check_stats(route, mode, tag, u, rec, bn, bar, momentum_steps=1):
    errs = {}
    for name, got, want in (('mean', rec['mean'], u['mean']), ('invstd', rec['invstd'], u['invstd']),
                            ('running_mean', bn.running_mean, u['running_mean']), ('running_var', bn.running_var, u['running_var'])):
        errs[name] = note(route, mode, '%s %s' % (tag, name), rel_err(got, want), bar)
        assert errs[name] < bar, (route, mode, tag, name, errs[name])
    assert int(bn.num_batches_tracked) == momentum_steps
    return errs


def check_first(route, mode, tag, u, rec, z, bn, bar=None):
    """A unit on dyadic operands: y IS the fp64 conv; z per element inside its interval (z None: never written, a lazy unit)."""
    bar = U.BARS[mode] if bar is None else bar
    assert torch.equal(rec['y'].double().cpu(), u['y'].detach()), (route, mode, tag, 'y')
    errs = check_stats(route, mode, tag, u, rec, bn, bar)
    if z is not None:
        ratio = float(((z.double().cpu() - u['z'].detach()).abs() / U.z_interval(u)).max())
        print('MEASURED %s %s %s z: worst element at %.3f of its interval' % (route, mode, tag, ratio))
        assert ratio <= 1.0, (route, mode, tag, ratio)            # (a NaN compares false)
        errs['z'] = note(route, mode, '%s z' % tag, rel_err(z, u['z']), bar)
    return errs


def check_later(route, mode, tag, u, rec, z, bn, bar=None):
    bar = U.BARS[mode] if bar is None else bar
    errs = check_stats(route, mode, tag, u, rec, bn, bar)
    for name, got in (('y', rec['y']), ('z', z)):
        if got is not None:
            errs[name] = note(route, mode, '%s %s' % (tag, name), rel_err(got, u[name]), bar)
            assert errs[name] < bar, (route, mode, tag, name, errs[name])
    return errs


def check_grads(route, mode, want, got, ns):
    """got / want: name -> gradient; ns: name -> number of kernels between the seed and that tensor."""
    errs = {}
    assert set(ns) <= set(got), (sorted(ns), sorted(got))
    for name, n in ns.items():
        bar = n * U.BARS[mode]
        errs[name] = note(route, mode, 'd' + name, rel_err(got[name], want[name]), bar)
        assert errs[name] < bar, (route, mode, name, errs[name], bar)
    return errs


def same_bits(a, b, what):
    for name in a:
        assert torch.equal(a[name], b[name]), (what, name, float((a[name] - b[name]).abs().max()))


def no_worse(fused, unfused, names, what):
    """The 1.5 x rule of test_gpu_stem_dzf.py, on the tensors it is applied to there: `names` are conv gradients (dW, dx), whose
    error is a sum over thousands of terms.  Everything else is held otherwise, on BOTH routes: z per element by its interval
    (its norm-wise error is one or two fp32 roundings of the largest element either way, 5e-8 .. 1.2e-7 measured: a ratio of
    those ranks nothing), the residual gradient bit for bit between the routes, the per-channel vectors by their bars."""
    assert names and all(n == 'x' or n.startswith('w') for n in names), names
    for name in names:
        assert fused[name] <= 1.5 * unfused[name], (what, name, fused[name], unfused[name])


def backward(e, tp, defer=False):
    """Tape.backward, optionally under a DeferredReduce -> the collector."""
    coll = None
    e.reset()
    if defer:
        coll = e.ops.DeferredReduce()
        e.ops.DEFER[0] = coll
    try:
        tp.backward()
    finally:
        e.ops.DEFER[0] = None
    torch.cuda.synchronize()
    if defer:
        assert coll.launches == 1 and not coll.pending
    return coll


# ----------------------------------------------------------------------------- R1 / R2 / R8: one unit
def run_single(e, route, kname, relu, needs_grad, with_res, out_slice=False, off4=False):
    c = U.single(kname, relu, with_res)
    lv, u, mode = c.leaves, c.units['A'], e.mode
    conv, bn = e.unit(lv, 'A', U.KERNELS[kname])
    xv = e.tape.Var(f32(lv['x']), needs_grad)
    rv = e.tape.Var(f32(lv['res']), True) if with_res else None
    out = buf = None
    if out_slice:
        buf = nan_like((U.R1_X[0], U.R1_K + 5) + U.R1_X[2:], off4)
        out = buf[:, 3:3 + U.R1_K]
    tp = e.tape.Tape(True)
    e.reset()
    zv = e.layers.f_conv_bn_act(tp, conv, bn, xv, relu=relu, residual=rv, out=out)
    fwd, rec = e.names(), unit_records(e.calls)[0]
    torch.cuda.synchronize()
    if out_slice:
        assert zv.t.data_ptr() == out.data_ptr() and zv.t.stride() == out.stride()
        assert bool(torch.isnan(buf[:, :3]).all()) and bool(torch.isnan(buf[:, 3 + U.R1_K:]).all())
    assert not isinstance(zv, e.tape.LazyVar)
    errs = check_first(route, mode, 'A', u, rec, zv.t, bn)
    assert errs['z'] < U.BARS[mode]
    zv.grad = f32(c.seeds(U.BARS[mode])['z'][0])
    backward(e, tp)
    bwd = e.names()
    got = param_grads({'A': (conv, bn)})
    ns = {'wA': 2, 'gammaA': 1, 'betaA': 1}
    if needs_grad:
        got['x'], ns['x'] = xv.grad, 2
    else:
        assert xv.grad is None
    if with_res:
        got['res'], ns['res'] = rv.grad, 1
    errs.update(check_grads(route, mode, c.grads(U.BARS[mode]), got, ns))
    got.update(y=rec['y'], z=zv.t.clone(), mean=rec['mean'], invstd=rec['invstd'])
    return fwd, bwd, errs, got


def single_bwd(relu, needs_grad, with_res):
    mask = ('bn_bwd:1+res' if with_res else 'bn_bwd:2') if relu else ('bn_bwd:0+res' if with_res else 'bn_bwd:0')
    return [mask, 'conv_wgrad'] + (['conv_dgrad:new'] if needs_grad else [])


@pytest.mark.parametrize('kname', sorted(U.KERNELS))
@pytest.mark.parametrize('mode', U.MODES)
def test_r1_eager_unit(eng, mode, kname):
    """R1: conv_fwd(stats) + bn_train_fwd; backward bn_bwd + conv_wgrad [+ conv_dgrad], relu and needs_grad both ways, one split
    pinned (the heuristic shape of this geometry splits, which is R2).  n: dgamma / dbeta 1 (bn_bwd), dW and dx 2."""
    eng.set_mode(mode)
    eng.pin('r1_' + kname)
    for relu in (True, False):
        for needs_grad in (True, False):
            fwd, bwd, _, _ = run_single(eng, 'R1', kname, relu, needs_grad, False)
            assert fwd == ['conv_fwd', 'bn_train_fwd'], fwd
            assert bwd == single_bwd(relu, needs_grad, False), bwd


@pytest.mark.parametrize('splits', [2, 3, 5])
@pytest.mark.parametrize('kname', sorted(U.KERNELS))
@pytest.mark.parametrize('mode', U.MODES)
def test_r2_splitk_slabs_into_the_small_batchnorm(eng, mode, kname, splits):
    """R2: conv_bn_small_fwd, with / without residual, relu both ways, and into a channel slice (16-byte aligned and 4 bytes
    off); FUSE_SPLITK_BN off takes R1 on the same plan.  The kernels differ (the BatchNorm kernel folds the slabs and takes
    its sums from them; the eager route takes fp32 partials from the conv epilogue), so: the fused route's fp64 error of dW and
    dx is at most 1.5 x the eager route's on the same inputs; y and the residual gradient are bit-equal between the routes; z,
    the statistics and dgamma / dbeta are held by their interval and bars on both."""
    eng.set_mode(mode)
    eng.pin('r2_%s_s%d' % (kname, splits))
    for relu, with_res in ((True, False), (False, False), (True, True), (False, True)):
        arms = {}
        for fuse in (True, False):
            eng.flag('FUSE_SPLITK_BN', fuse)
            fwd, bwd, errs, got = arms[fuse] = run_single(eng, 'R2' if fuse else 'R2->R1', kname, relu, True, with_res)
            assert fwd == (['conv_bn_small_fwd'] if fuse else ['conv_fwd', 'bn_train_fwd']), (fuse, fwd)
            assert bwd == single_bwd(relu, True, with_res), bwd
        no_worse(arms[True][2], arms[False][2], ['x', 'wA'], ('R2', mode, kname, splits, relu, with_res))
        assert torch.equal(arms[True][3]['y'], arms[False][3]['y'])
        if with_res:
            assert torch.equal(arms[True][3]['res'], arms[False][3]['res'])
    eng.flag('FUSE_SPLITK_BN', True)
    for off4 in (False, True):
        fwd, bwd, _, _ = run_single(eng, 'R2 out=', kname, True, True, False, out_slice=True, off4=off4)
        assert fwd == ['conv_bn_small_fwd:out'] and bwd == single_bwd(True, True, False)


@pytest.mark.parametrize('kname', sorted(U.KERNELS))
@pytest.mark.parametrize('mode', U.MODES)
def test_r8_eval_mode(eng, mode, kname):
    """R8: bn_fold_eval + bn_apply, forward only; running statistics untouched; recording a backward raises."""
    eng.set_mode(mode)
    eng.pin('r1_' + kname)
    c, ref = U.single(kname, True, False), U.eval_case(kname)
    conv, bn = eng.unit(c.leaves, 'A', U.KERNELS[kname])
    with torch.no_grad():
        bn.running_mean.copy_(f32(ref['rmean']))
        bn.running_var.copy_(f32(ref['rvar']))
    bn.eval()
    x = f32(c.leaves['x'])
    for out_slice in (False, True):
        buf = nan_like((2, 21) + U.R1_X[2:]) if out_slice else None
        eng.reset()
        zv = eng.layers.f_conv_bn_act(eng.tape.Tape(False), conv, bn, eng.tape.Var(x, False), out=None if buf is None else buf[:, 3:19])
        torch.cuda.synchronize()
        assert eng.names() == ['conv_fwd', 'bn_fold_eval', 'bn_apply:out' if out_slice else 'bn_apply'], eng.names()
        assert torch.equal(eng.calls[0][1].double().cpu(), ref['y'])
        err = note('R8', mode, 'z', rel_err(zv.t, ref['z']), U.BARS[mode])
        assert err < U.BARS[mode]
        if out_slice:
            assert bool(torch.isnan(buf[:, :3]).all()) and bool(torch.isnan(buf[:, 19:]).all())
    assert torch.equal(bn.running_mean, f32(ref['rmean'])) and torch.equal(bn.running_var, f32(ref['rvar']))
    assert int(bn.num_batches_tracked) == 0
    with pytest.raises(NotImplementedError):
        eng.layers.f_conv_bn_act(eng.tape.Tape(True), conv, bn, eng.tape.Var(x, False))


# ----------------------------------------------------------------------------- R3 / R9 / R10: lazy producer -> temporal consumer
def run_r3(e, lazy=True, defer=False, route_b=U.R3_B, fp16=False):
    c = U.chain('r3')
    lv, mode = c.leaves, e.mode
    e.flag('LAZY_BN', lazy)
    if not fp16:
        e.pin('r3_a')
        e.pin(route_b)
    A, B = e.unit(lv, 'A', U.K133), e.unit(lv, 'B', U.K311)
    tp = e.tape.Tape(True)
    e.reset()
    av = e.layers.f_conv_bn_act(tp, *A, e.tape.Var(f32(lv['x']), False))
    bv = e.layers.f_conv_bn_act(tp, *B, av)
    fwd, recs = e.names(), unit_records(e.calls)
    a_unwritten = isinstance(av, e.tape.LazyVar) and not av.materialized
    zB = bv.t
    bv.grad = f32(U.r3_f16()['seed']).half() if fp16 else f32(c.seeds(U.BARS[mode])['zB'][0])
    coll = backward(e, tp, defer)
    out = dict(yA=recs[0]['y'], yB=recs[1]['y'], zB=zB, meanA=recs[0]['mean'], invstdA=recs[0]['invstd'], meanB=recs[1]['mean'],
               invstdB=recs[1]['invstd'])
    out.update(param_grads({'A': A, 'B': B}))
    return dict(c=c, fwd=fwd, bwd=e.names(), recs=recs, a_unwritten=a_unwritten, av=av, A=A, B=B, out=out, coll=coll)


R3_NS = {'gammaB': 1, 'betaB': 1, 'wB': 2, 'gammaA': 3, 'betaA': 3, 'wA': 4}       # bn_bwd, conv_wgrad | conv_dgrad, bn_bwd, conv_wgrad


def check_two_units(route, mode, r, ns):
    c = r['c']
    errs = check_first(route, mode, 'A', c.units['A'], r['recs'][0], None, r['A'][1])
    errs.update(check_later(route, mode, 'B', c.units['B'], r['recs'][1], r['out']['zB'], r['B'][1]))
    errs.update(check_grads(route, mode, c.grads(U.BARS[mode]), r['out'], ns))
    return errs


@pytest.mark.parametrize('route_b', [U.R3_B, 'r3_b_1x4x32_t12', 'r3_b_1x1x128_t12'])
@pytest.mark.parametrize('mode', U.MODES)
def test_r3_lazy_producer_consumed_on_the_fly(eng, mode, route_b):
    """R3: A returns a LazyVar; B on a halo forward + temporal32 / temporal64 weight gradient reads (y, scale, shift): bn_finalize,
    conv_fwd_xf, no bn_apply, A never written.  Under f32 conv_xf_ok is false (the weight gradient falls to the gather kernel)
    and A materialises once.  Against LAZY_BN off: the same kernels on the same bits (above 32768 positions bn_train_fwd IS
    bn_finalize + bn_apply, and conv_fwd_xf / conv_wgrad(xf) stage relu(y * scale + shift) as bn_apply stores it,
    test_conv_consumes_producer_batchnorm_relu_on_the_fly), so every output and gradient is torch.equal.
    n: B's dgamma / dbeta 1, dW_B 2; through conv_dgrad and A's bn_bwd: dgamma_A / dbeta_A 3, dW_A 4."""
    eng.set_mode(mode)
    xf = mode != 'f32'
    r = run_r3(eng, route_b=route_b)
    if xf:
        assert r['fwd'] == ['conv_fwd', 'bn_finalize', 'conv_fwd_xf', 'bn_finalize'], r['fwd']
        assert r['a_unwritten'] and not r['av'].materialized
    else:
        assert r['fwd'] == ['conv_fwd', 'bn_finalize', 'bn_apply', 'conv_fwd', 'bn_finalize'], r['fwd']
        assert r['av'].materialized
    assert r['bwd'] == ['bn_bwd:2', 'conv_wgrad:xf' if xf else 'conv_wgrad', 'conv_dgrad:new', 'bn_bwd:2', 'conv_wgrad'], r['bwd']
    check_two_units('R3', mode, r, R3_NS)
    eager = run_r3(eng, lazy=False, route_b=route_b)
    assert eager['fwd'] == ['conv_fwd', 'bn_train_fwd', 'conv_fwd', 'bn_train_fwd'], eager['fwd']
    assert eager['bwd'] == ['bn_bwd:2', 'conv_wgrad', 'conv_dgrad:new', 'bn_bwd:2', 'conv_wgrad'], eager['bwd']
    same_bits(r['out'], eager['out'], ('R3 lazy vs eager', mode, route_b))


@pytest.mark.parametrize('mode', U.MODES)
def test_r9_deferred_reduce_on_r3(eng, mode):
    """R9: the backward of R3 under ops.DEFER: Tape.backward flushes ONE batched reduction; the fold order is the per-layer
    one, so every gradient is bit-identical."""
    eng.set_mode(mode)
    now, later = run_r3(eng), run_r3(eng, defer=True)
    assert later['bwd'] == now['bwd'] and later['coll'].launches == 1
    same_bits(now['out'], later['out'], ('R9 on R3', mode))


def test_r10_fp16_storage_takes_the_eager_route(eng):
    """R10: R3's chain under set_conv_math('fp16'): nothing lazy, no xf, no fused small BatchNorm, the eager backward.
    Reference: units_ref.r3_f16, double arithmetic that rounds to fp16 exactly where the engine stores (y, z, dz, dy of both
    units) -- what the bars of tests/test_gpu_f16.py are declared against.  fp16 outputs (y, z) within 1.5e-3, fp32 outputs
    within 2e-4: statistics, and each gradient at n x 2e-4 with R3's n.  y_A, an fp16 number element for element, is bit-equal.
    The unrounded fp64 chain is held too, on the same seed, at n x 1.5e-3: between the seed and the tensor lie n kernels that
    each read or write an fp16-stored tensor, whose rounding (2^-11 per element; 1.5e-3 is its per-kernel bar) does not
    average out under a random seed.  It cannot be held at n x 2e-4: storage rounding ALONE separates the two references by
    2.9e-4 .. 5.2e-4 (dgamma_B: 5.2e-4 against 1 x 2e-4; tests/test_units_ref.py prints and asserts that gap on the CPU)."""
    eng.set_mode('fp16')
    r = run_r3(eng, fp16=True)
    assert r['fwd'] == ['conv_fwd', 'bn_train_fwd', 'conv_fwd', 'bn_train_fwd'], r['fwd']
    assert r['bwd'] == ['bn_bwd:2', 'conv_wgrad', 'conv_dgrad:new', 'bn_bwd:2', 'conv_wgrad'], r['bwd']
    assert not isinstance(r['av'], eng.tape.LazyVar) and r['av'].t.dtype is torch.float16 and r['out']['zB'].dtype is torch.float16
    ref, (b16, b32) = U.r3_f16(), U.F16_BARS
    assert torch.equal(r['recs'][0]['y'].double().cpu(), ref['A']['y'].detach())
    for tag, rec, bn, z in (('A', r['recs'][0], r['A'][1], r['av'].t), ('B', r['recs'][1], r['B'][1], r['out']['zB'])):
        u = ref[tag]
        check_stats('R10', 'fp16', tag, u, rec, bn, b32)
        for name, got in (('y', rec['y']), ('z', z)):
            assert got.dtype is torch.float16
            assert note('R10', 'fp16', '%s %s' % (tag, name), rel_err(got, u[name]), b16) < b16
    for name, n in R3_NS.items():
        g = r['out'][name]
        assert g.dtype is torch.float32
        e_stored = note('R10', 'fp16', 'd%s vs fp16-storage reference' % name, rel_err(g, ref['grads'][name]), n * b32)
        e_plain = note('R10 vs unrounded', 'fp16', 'd%s' % name, rel_err(g, ref['plain'][name]), n * b16)
        assert e_stored < n * b32, (name, e_stored, n * b32)
        assert e_plain < n * b16, (name, e_plain, n * b16)


# ----------------------------------------------------------------------------- R4: lazy producer that must materialise
@pytest.mark.parametrize('mode', U.MODES)
def test_r4_lazy_producer_into_a_pool(eng, mode):
    """R4, first consumer a max pool: reading `.t` launches bn_apply once.  A is a first unit, so every pool decision is the
    reference's (monotone in y within a channel, exact ties to the first index) and the whole seed is kept.
    n: maxpool_bwd 1, bn_bwd 2 (dgamma / dbeta), conv_wgrad 3."""
    eng.set_mode(mode)
    c = U.chain('r4pool')
    lv, u = c.leaves, c.units['A']
    eng.pin('r3_a')
    A = eng.unit(lv, 'A', U.K133)
    pool = eng.layers.HipMaxPool3d(*U.POOL_122)
    tp = eng.tape.Tape(True)
    eng.reset()
    av = eng.layers.f_conv_bn_act(tp, *A, eng.tape.Var(f32(lv['x']), False))
    assert isinstance(av, eng.tape.LazyVar) and not av.materialized
    pv = eng.layers.f_maxpool(tp, pool, av)
    assert eng.names() == ['conv_fwd', 'bn_finalize', 'bn_apply', 'maxpool_fwd'], eng.names()
    check_first('R4 pool', mode, 'A', u, unit_records(eng.calls)[0], av.t, A[1])
    want = c.outs['pool'][0].detach()
    bound = U.maxpool(U.z_interval(u), U.POOL_122)                 # a pooled value is one z of its window
    assert bool(((pv.t.double().cpu() - want).abs() <= bound).all())
    pv.grad = f32(c.seeds(U.BARS[mode])['pool'][0])
    backward(eng, tp)
    assert eng.names() == ['maxpool_bwd:new', 'bn_bwd:2', 'conv_wgrad'], eng.names()
    check_grads('R4 pool', mode, c.grads(U.BARS[mode]), param_grads({'A': A}), {'gammaA': 2, 'betaA': 2, 'wA': 3})


@pytest.mark.parametrize('mode', U.MODES)
def test_r4_spatial_consumer_cannot_take_xf(eng, mode):
    """R4, a (1,3,3) consumer at W = 68 with the spatial streaming weight-gradient kernel pinned: conv_xf_ok stays false (only
    temporal32 / temporal64 set xf), so A materialises and B reads z through conv_fwd.  n as R3."""
    eng.set_mode(mode)
    c = U.chain('r4conv')
    lv = c.leaves
    eng.pin('r4_a')
    plan_b = eng.pin('r4_b')
    assert not eng.ops.conv_xf_ok(plan_b) and (mode == 'f32' or plan_b.kernel(2) == 'spatial')
    A, B = eng.unit(lv, 'A', U.K133), eng.unit(lv, 'B', U.K133)
    tp = eng.tape.Tape(True)
    eng.reset()
    av = eng.layers.f_conv_bn_act(tp, *A, eng.tape.Var(f32(lv['x']), False))
    bv = eng.layers.f_conv_bn_act(tp, *B, av)
    assert eng.names() == ['conv_fwd', 'bn_finalize', 'bn_apply', 'conv_fwd', 'bn_finalize'], eng.names()
    recs = unit_records(eng.calls)
    assert av.materialized and isinstance(bv, eng.tape.LazyVar)
    zB = bv.t
    bv.grad = f32(c.seeds(U.BARS[mode])['zB'][0])
    backward(eng, tp)
    assert eng.names() == ['bn_bwd:2', 'conv_wgrad', 'conv_dgrad:new', 'bn_bwd:2', 'conv_wgrad'], eng.names()
    out = dict(zB=zB)
    out.update(param_grads({'A': A, 'B': B}))
    r = dict(c=c, recs=recs, A=A, B=B, out=out)
    check_two_units('R4 spatial', mode, r, R3_NS)
    ratio = float(((av.t.double().cpu() - c.units['A']['z'].detach()).abs() / U.z_interval(c.units['A'])).max())
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize('conv_first', [True, False])
@pytest.mark.parametrize('mode', U.MODES)
def test_r4_two_consumers_of_one_lazy_producer(eng, mode, conv_first):
    """R4, one LazyVar read by a temporal conv (through xf while A is unwritten) and by a pool (through `.t`), in both orders:
    bn_apply runs exactly once; A's gradient buffer is allocated by the first writer of the backward and the second accumulates
    (conv_dgrad:acc after maxpool_bwd:new, or maxpool_bwd:acc after conv_dgrad:new); its BatchNorm sees the sum.
    n: A's dgamma / dbeta 3, dW_A 4 (the longer path, through B)."""
    eng.set_mode(mode)
    c = U.chain('r4both')
    lv = c.leaves
    eng.pin('r3_a')
    eng.pin(U.R3_B)
    A, B = eng.unit(lv, 'A', U.K133), eng.unit(lv, 'B', U.K311)
    pool = eng.layers.HipMaxPool3d(*U.POOL_122)
    tp = eng.tape.Tape(True)
    eng.reset()
    av = eng.layers.f_conv_bn_act(tp, *A, eng.tape.Var(f32(lv['x']), False))
    xf = mode != 'f32' and conv_first
    if conv_first:
        bv = eng.layers.f_conv_bn_act(tp, *B, av)
        assert av.materialized == (not xf)
        pv = eng.layers.f_maxpool(tp, pool, av)
        want = (['conv_fwd', 'bn_finalize', 'conv_fwd_xf', 'bn_finalize', 'bn_apply', 'maxpool_fwd'] if xf else
                ['conv_fwd', 'bn_finalize', 'bn_apply', 'conv_fwd', 'bn_finalize', 'maxpool_fwd'])
        bwd = ['maxpool_bwd:new', 'bn_bwd:2', 'conv_wgrad:xf' if xf else 'conv_wgrad', 'conv_dgrad:acc', 'bn_bwd:2', 'conv_wgrad']
    else:
        pv = eng.layers.f_maxpool(tp, pool, av)
        bv = eng.layers.f_conv_bn_act(tp, *B, av)
        want = ['conv_fwd', 'bn_finalize', 'bn_apply', 'maxpool_fwd', 'conv_fwd', 'bn_finalize']
        bwd = ['bn_bwd:2', 'conv_wgrad', 'conv_dgrad:new', 'maxpool_bwd:acc', 'bn_bwd:2', 'conv_wgrad']
    assert eng.names() == want, eng.names()
    assert eng.names().count('bn_apply') == 1 and av.materialized
    recs = unit_records(eng.calls)
    zB = bv.t
    seeds = c.seeds(U.BARS[mode])
    bv.grad, pv.grad = f32(seeds['zB'][0]), f32(seeds['pool'][0])
    backward(eng, tp)
    assert eng.names() == bwd, eng.names()
    out = dict(zB=zB)
    out.update(param_grads({'A': A, 'B': B}))
    check_two_units('R4 both', mode, dict(c=c, recs=recs, A=A, B=B, out=out), R3_NS)
    assert bool(((pv.t.double().cpu() - c.outs['pool'][0].detach()).abs() <= U.maxpool(U.z_interval(c.units['A']), U.POOL_122)).all())


# ----------------------------------------------------------------------------- R5: conv + BatchNorm + ReLU + max pool in one unit
def run_r5(e, lazy=True, dzf=True, defer=False):
    c = U.chain('r5')
    lv, mode = c.leaves, e.mode
    e.flag('LAZY_BN', lazy)
    e.flag('STEM_DZF', dzf)
    e.pin('r5_stem')
    e.pin('r5_t')
    A, B = e.unit(lv, 'A', U.STEM), e.unit(lv, 'B', U.K311)
    pool = e.layers.HipMaxPool3d(3, 2, 1)
    tp = e.tape.Tape(True)
    e.reset()
    av = e.layers.f_conv_bn_act(tp, *A, e.tape.Var(f32(lv['x']), False))
    pv = e.layers.f_conv_bn_relu_maxpool(tp, *B, pool, av)
    fwd, recs = e.names(), unit_records(e.calls)
    unwritten = isinstance(av, e.tape.LazyVar) and not av.materialized
    pv.grad = f32(c.seeds(U.BARS[mode])['pool'][0])
    coll = backward(e, tp, defer)
    out = dict(yA=recs[0]['y'], yB=recs[1]['y'], pool=pv.t, meanB=recs[1]['mean'], invstdB=recs[1]['invstd'])
    out.update(param_grads({'A': A, 'B': B}))
    return dict(c=c, fwd=fwd, bwd=e.names(), recs=recs, unwritten=unwritten, A=A, B=B, out=out, coll=coll)


R5_NS = {'gammaB': 2, 'betaB': 2, 'wB': 3, 'gammaA': 4, 'betaA': 4, 'wA': 5}       # maxpool_bwd, bn_bwd, wgrad | dgrad, bn_bwd(_sums), wgrad(_dzf)


def check_r5(route, mode, r):
    c = r['c']
    errs = check_first(route, mode, 'A', c.units['A'], r['recs'][0], None, r['A'][1])
    errs.update(check_later(route, mode, 'B', c.units['B'], r['recs'][1], None, r['B'][1]))
    errs['pool'] = note(route, mode, 'pool', rel_err(r['out']['pool'], c.outs['pool'][0]), U.BARS[mode])
    assert errs['pool'] < U.BARS[mode]
    errs.update(check_grads(route, mode, c.grads(U.BARS[mode]), r['out'], R5_NS))
    return errs


@pytest.mark.parametrize('mode', U.MODES)
def test_r5_stem_chain_into_the_pooling_unit(eng, mode):
    """R5: the lazy stem (2, 3, 4, 144, 144) -> 16 channels, then f_conv_bn_relu_maxpool on a (3,1,1) conv and a 3/2/1 pool: the
    BatchNorm + ReLU is evaluated inside the pool, backward is maxpool_bwd, bn_bwd(z = None, mode 2), conv_wgrad, conv_dgrad,
    then the stem's bn_bwd_sums + conv_wgrad_dzf (split modes; under f32 neither the stem kernel nor xf exists).
    Against LAZY_BN off: same kernels, same bits -> torch.equal.  Against STEM_DZF off: other kernels for the stem's backward,
    so the dzf route's fp64 error of dW_A is at most 1.5 x that of bn_bwd + conv_wgrad; its BatchNorm gradients come from the
    same sums kernel and are bit-equal (test_layer_takes_the_fused_route).
    Under a DeferredReduce (R9), in every mode: one batched reduction, every gradient bit-identical.
    n: pool 1, B's bn_bwd 2, dW_B 3; conv_dgrad, stem BatchNorm 4, dW_A 5."""
    eng.set_mode(mode)
    split = mode != 'f32'
    r = run_r5(eng)
    tail = ['bn_bwd_sums', 'conv_wgrad_dzf'] if split else ['bn_bwd:2', 'conv_wgrad']
    if split:
        assert r['fwd'] == ['conv_fwd', 'bn_finalize', 'conv_fwd_xf', 'bn_finalize', 'maxpool_fwd'] and r['unwritten'], r['fwd']
    else:
        assert r['fwd'] == ['conv_fwd', 'bn_finalize', 'bn_apply', 'conv_fwd', 'bn_finalize', 'maxpool_fwd'], r['fwd']
    assert r['bwd'] == ['maxpool_bwd:own', 'bn_bwd:2', 'conv_wgrad:xf' if split else 'conv_wgrad', 'conv_dgrad:new'] + tail, r['bwd']
    errs = check_r5('R5', mode, r)
    eager = run_r5(eng, lazy=False)
    assert eager['fwd'] == ['conv_fwd', 'bn_train_fwd', 'conv_fwd', 'bn_finalize', 'maxpool_fwd'], eager['fwd']
    assert eager['bwd'] == ['maxpool_bwd:own', 'bn_bwd:2', 'conv_wgrad', 'conv_dgrad:new'] + tail, eager['bwd']
    same_bits(r['out'], eager['out'], ('R5 lazy vs eager', mode))
    if split:
        plain = run_r5(eng, dzf=False)
        assert plain['bwd'][-2:] == ['bn_bwd:2', 'conv_wgrad'], plain['bwd']
        e2 = check_r5('R5 no dzf', mode, plain)
        assert errs['wA'] <= 1.5 * e2['wA'], (errs['wA'], e2['wA'])
        for name in ('gammaA', 'betaA', 'gammaB', 'betaB', 'wB', 'pool'):
            assert torch.equal(r['out'][name], plain['out'][name]), name
    later = run_r5(eng, defer=True)                                      # R9 on R5, in every mode
    assert later['bwd'] == r['bwd'] and later['coll'].launches == 1
    same_bits(r['out'], later['out'], ('R9 on R5', mode))


@pytest.mark.parametrize('mode', U.MODES)
def test_r5_pooling_unit_on_a_plain_var(eng, mode):
    """R5, direct: one dyadic unit at R1's size into the 3/2/1 pool, input a plain Var that needs its gradient.
    n: dgamma / dbeta 2, dW and dx 3."""
    eng.set_mode(mode)
    c = U.chain('r5small')
    lv, u = c.leaves, c.units['A']
    eng.pin('r5_small')
    A = eng.unit(lv, 'A', U.K311)
    xv = eng.tape.Var(f32(lv['x']), True)
    tp = eng.tape.Tape(True)
    eng.reset()
    pv = eng.layers.f_conv_bn_relu_maxpool(tp, *A, eng.layers.HipMaxPool3d(3, 2, 1), xv)
    assert eng.names() == ['conv_fwd', 'bn_finalize', 'maxpool_fwd'], eng.names()
    check_first('R5 direct', mode, 'A', u, unit_records(eng.calls)[0], None, A[1])
    assert bool(((pv.t.double().cpu() - c.outs['pool'][0].detach()).abs() <= U.maxpool(U.z_interval(u), U.POOL_321)).all())
    pv.grad = f32(c.seeds(U.BARS[mode])['pool'][0])
    backward(eng, tp)
    assert eng.names() == ['maxpool_bwd:own', 'bn_bwd:2', 'conv_wgrad', 'conv_dgrad:new'], eng.names()
    got = param_grads({'A': A})
    got['x'] = xv.grad
    check_grads('R5 direct', mode, c.grads(U.BARS[mode]), got, {'gammaA': 2, 'betaA': 2, 'wA': 3, 'x': 3})


# ----------------------------------------------------------------------------- R6: residual and fan-out
def run_r6(e, prefill, defer=False):
    c = U.chain('r6')
    lv, mode = c.leaves, e.mode
    e.pin('r6_a')
    A, B = e.unit(lv, 'A', U.K333), e.unit(lv, 'B', U.K333)
    xv = e.tape.Var(f32(lv['x']), True)
    g0 = f32(U.randn64(U.R6_X, 977)) if prefill else None
    if prefill:
        xv.grad = g0.clone()                     # an earlier consumer of x has already written its gradient
    tp = e.tape.Tape(True)
    e.reset()
    av = e.layers.f_conv_bn_act(tp, *A, xv)
    bv = e.layers.f_conv_bn_act(tp, *B, av, relu=True, residual=xv)
    fwd, recs = e.names(), unit_records(e.calls)
    bv.grad = f32(c.seeds(U.BARS[mode])['zB'][0])
    coll = backward(e, tp, defer)
    out = dict(zA=av.t, zB=bv.t, x=xv.grad)
    out.update(param_grads({'A': A, 'B': B}))
    return dict(c=c, fwd=fwd, bwd=e.names(), recs=recs, A=A, B=B, out=out, g0=g0, coll=coll)


R6_NS = {'gammaB': 1, 'betaB': 1, 'wB': 2, 'gammaA': 3, 'betaA': 3, 'wA': 4, 'x': 4}


@pytest.mark.parametrize('prefill', [False, True])
@pytest.mark.parametrize('mode', U.MODES)
def test_r6_residual_block(eng, mode, prefill):
    """R6: z = relu(BN_B(conv_B(relu(BN_A(conv_A x)))) + x).  B's mask is read from z (mode 1); x.grad is the residual gradient
    written fresh by B's bn_bwd and THEN A's dgrad accumulating -- or, with x.grad pre-filled by an earlier consumer, both add
    (dres_accumulate).  n: B 1 / 2; dgrad, A's bn_bwd 3, dW_A and dx 4.  Deferred reduce (R9): bit-identical."""
    eng.set_mode(mode)
    r = run_r6(eng, prefill)
    assert r['fwd'] == ['conv_fwd', 'bn_train_fwd', 'conv_fwd', 'bn_train_fwd'], r['fwd']
    assert r['bwd'] == ['bn_bwd:1+res' + (':acc' if prefill else ''), 'conv_wgrad', 'conv_dgrad:new', 'bn_bwd:2', 'conv_wgrad', 'conv_dgrad:acc'], r['bwd']
    c = r['c']
    check_first('R6', mode, 'A', c.units['A'], r['recs'][0], r['out']['zA'], r['A'][1])
    check_later('R6', mode, 'B', c.units['B'], r['recs'][1], r['out']['zB'], r['B'][1])
    want = dict(c.grads(U.BARS[mode]))
    if prefill:
        want['x'] = want['x'] + r['g0'].double().cpu()
    check_grads('R6', mode, want, r['out'], R6_NS)
    later = run_r6(eng, prefill, defer=True)
    assert later['bwd'] == r['bwd']
    same_bits(r['out'], later['out'], ('R9 on R6', mode))


def run_basic_block(e, fuse):
    c = U.chain('r6s')
    lv, mode = c.leaves, e.mode
    e.flag('FUSE_SPLITK_BN', fuse)
    for route in ('r6s_a', 'r6s_b', 'r6s_s'):
        e.pin(route)
    L = e.layers
    blk = e.pkg.lib.modeling.backbone.backbone_3d.resnet.BasicBlock(
        16, 32, 2, nn.Sequential(L.HipConv3d(16, 32, 1, 2, 0), L.HipBatchNorm3d(32))).to(DEV)
    units = {'A': (blk.conv1, blk.bn1), 'B': (blk.conv2, blk.bn2), 'S': (blk.downsample[0], blk.downsample[1])}
    for tag, (conv, bn) in units.items():
        load(conv, bn, lv, tag)
    xv = e.tape.Var(f32(lv['x']), True)
    tp = e.tape.Tape(True)
    e.reset()
    bv = blk.fwd(tp, xv)
    fwd, recs = e.names(), unit_records(e.calls)
    bv.grad = f32(c.seeds(U.BARS[mode])['zB'][0])
    backward(e, tp)
    out = dict(zB=bv.t, x=xv.grad)
    out.update(param_grads(units))
    return dict(c=c, fwd=fwd, bwd=e.names(), recs=recs, units=units, out=out)


@pytest.mark.parametrize('mode', U.MODES)
def test_r6_basic_block_with_strided_shortcut(eng, mode):
    """R6 through the real resnet.BasicBlock(16, 32, stride=2, downsample): main branch strided (dgrad in the merged launch), the
    residual a relu=False 1x1x1 stride-2 unit (mask mode 0, its gradient written by B's bn_bwd), x.grad = shortcut dgrad fresh,
    then A's accumulating.  Both 3x3x3 convs split: fused small BatchNorm vs FUSE_SPLITK_BN off are different kernels, so the
    fused route's fp64 errors of dW_A, dW_S, dW_B and dx are at most 1.5 x the eager route's (the rest: bars on both routes).
    Order of units: A, S, B.
    n: B 1 / 2; S: bn_bwd 2, dW_S 3; A: dgrad, bn_bwd 3, dW_A 4; dx 4."""
    eng.set_mode(mode)
    ns = {'gammaB': 1, 'betaB': 1, 'wB': 2, 'gammaS': 2, 'betaS': 2, 'wS': 3, 'gammaA': 3, 'betaA': 3, 'wA': 4, 'x': 4}
    errs = {}
    for fuse in (True, False):
        r = run_basic_block(eng, fuse)
        small, eager = ['conv_bn_small_fwd'], ['conv_fwd', 'bn_train_fwd']
        assert r['fwd'] == (small + eager + small if fuse else eager * 3), (fuse, r['fwd'])
        assert r['bwd'] == ['bn_bwd:1+res', 'conv_wgrad', 'conv_dgrad:new', 'bn_bwd:0', 'conv_wgrad', 'conv_dgrad:new',
                            'bn_bwd:2', 'conv_wgrad', 'conv_dgrad:acc'], r['bwd']
        c, route = r['c'], 'R6 block' if fuse else 'R6 block eager'
        e1 = check_first(route, mode, 'A', c.units['A'], r['recs'][0], None, r['units']['A'][1])
        e1.update({'S ' + k: v for k, v in check_first(route, mode, 'S', c.units['S'], r['recs'][1], None, r['units']['S'][1]).items()})
        e1.update({'B ' + k: v for k, v in check_later(route, mode, 'B', c.units['B'], r['recs'][2], r['out']['zB'], r['units']['B'][1]).items()})
        e1.update(check_grads(route, mode, c.grads(U.BARS[mode]), r['out'], ns))
        errs[fuse] = e1
    no_worse(errs[True], errs[False], ['wA', 'wS', 'wB', 'x'], ('R6 block', mode))


# ----------------------------------------------------------------------------- R7: channel slices and f_concat
def run_mixed(e, splits, off4, prefill):
    c = U.chain('mixed')
    lv, mode = c.leaves, e.mode
    geoms = U.MIXED_GEOMS
    for tag in geoms:
        e.pin('r7_%s_s%d' % (tag, splits))
    units = {tag: e.unit(lv, tag, ksp) for tag, (_, _, ksp) in geoms.items()}
    xv = e.tape.Var(f32(lv['x']), True)
    g0 = f32(U.randn64(U.R1_X, 978)) if prefill else None
    if prefill:
        xv.grad = g0.clone()
    N, _, D, Hh, W = U.R1_X
    widths, offs = U.MIXED_WIDTHS, (0, 6, 15)
    buf = nan_like((N, sum(widths), D, Hh, W), off4)
    sl = [buf[:, o:o + w] for o, w in zip(offs, widths)]
    L, tp = e.layers, e.tape.Tape(True)
    e.reset()
    v0 = L.f_conv_bn_act(tp, *units['b0'], xv, out=sl[0])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:, 6:]).all()) and not bool(torch.isnan(sl[0]).any())
    s0 = sl[0].clone()
    v1a = L.f_conv_bn_act(tp, *units['b1a'], xv)
    v1 = L.f_conv_bn_act(tp, *units['b1b'], v1a, out=sl[1])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:, 15:]).all()) and torch.equal(sl[0], s0) and not bool(torch.isnan(sl[1]).any())
    s1 = sl[1].clone()
    pv = L.f_maxpool(tp, L.HipMaxPool3d(3, 1, 1), xv)
    v2 = L.f_conv_bn_act(tp, *units['b2'], pv, out=sl[2])
    torch.cuda.synchronize()
    assert torch.equal(sl[0], s0) and torch.equal(sl[1], s1) and not bool(torch.isnan(buf).any())
    outv = L.f_concat(tp, buf, [v0, v1, v2], list(offs))
    fwd, recs = e.names(), unit_records(e.calls)
    seed = nan_like(buf.shape, off4)
    seed.copy_(f32(c.seeds(U.BARS[mode])['buf'][0]))
    outv.grad = seed
    backward(e, tp)
    out = dict(buf=buf, z1a=v1a.t, x=xv.grad)
    out.update(param_grads(units))
    return dict(c=c, fwd=fwd, bwd=e.names(), recs=recs, units=units, out=out, g0=g0)


@pytest.mark.parametrize('prefill', [False, True])
@pytest.mark.parametrize('off4', [False, True])
@pytest.mark.parametrize('splits', [1, 2])
@pytest.mark.parametrize('mode', U.MODES)
def test_r7_branches_into_channel_slices(eng, mode, splits, off4, prefill):
    """R7: 1x1x1 | 1x1x1 -> (1,3,3) | max pool 3/1/1 -> 1x1x1 over one input, widths 6 / 9 / 7 written into slices of ONE
    buffer (eager bn_train_fwd(out=) with one split pinned, conv_bn_small_fwd(out=) with two), then f_concat.  The buffer starts
    as NaN and every byte outside a unit's slice is untouched by that unit's write; off4 puts buffer and seed 4 bytes off
    16-byte alignment (the per-element forms of the BatchNorm kernels).  On the way back the slices of d(buf) arrive as strided
    dz; x.grad collects the pool's, b1a's and b0's contributions (maxpool_bwd, conv_dgrad), on top of a pre-filled buffer when
    `prefill`.  n: each slice unit 1 / 2; b1a behind b1b: 3 / 4; dx 4."""
    eng.set_mode(mode)
    r = run_mixed(eng, splits, off4, prefill)
    if splits == 1:
        w, p = ['conv_fwd', 'bn_train_fwd:out'], ['conv_fwd', 'bn_train_fwd']
    else:
        w, p = ['conv_bn_small_fwd:out'], ['conv_bn_small_fwd']
    assert r['fwd'] == w + p + w + ['maxpool_fwd'] + w, r['fwd']
    one = ['bn_bwd:2', 'conv_wgrad']
    assert r['bwd'] == (one + ['conv_dgrad:new', 'maxpool_bwd:acc' if prefill else 'maxpool_bwd:new'] + one + ['conv_dgrad:new'] +
                        one + ['conv_dgrad:acc'] + one + ['conv_dgrad:acc']), r['bwd']
    c, buf = r['c'], r['out']['buf']
    route = 'R7 s%d%s' % (splits, ' off4' if off4 else '')
    order = ('b0', 'b1a', 'b1b', 'b2')                                     # forward order of the units = order of recs
    zs = {'b0': buf[:, 0:6], 'b1a': r['out']['z1a'], 'b1b': buf[:, 6:15], 'b2': buf[:, 15:22]}
    for rec, tag in zip(r['recs'], order):
        (check_later if tag == 'b1b' else check_first)(route, mode, tag, c.units[tag], rec, zs[tag], r['units'][tag][1])
    ns = {'x': 4}
    for tag in order:
        k = 2 if tag == 'b1a' else 0
        ns.update({'gamma' + tag: 1 + k, 'beta' + tag: 1 + k, 'w' + tag: 2 + k})
    want = dict(c.grads(U.BARS[mode]))
    if prefill:
        want['x'] = want['x'] + r['g0'].double().cpu()
    check_grads(route, mode, want, r['out'], ns)


# ----------------------------------------------------------------------------- R8: a training-mode lazy producer in front of an eval unit
@pytest.mark.parametrize('mode', U.MODES)
def test_r8_lazy_producer_in_front_of_an_eval_unit(eng, mode):
    """R8: A trains (lazy), B is in eval mode: the `xf is not None and not train` branch takes A's tensor (bn_apply once), B
    folds its running statistics.  Under f32 _conv_input has already materialised A; the call sequence is the same."""
    eng.set_mode(mode)
    c = U.chain('r3')
    lv = c.leaves
    eng.pin('r3_a')
    eng.pin(U.R3_B)
    A, B = eng.unit(lv, 'A', U.K133), eng.unit(lv, 'B', U.K311)
    g = torch.Generator().manual_seed(5)
    rmean, rvar = (torch.randn(24, generator=g) * 0.5).double(), (torch.rand(24, generator=g) + 0.5).double()
    with torch.no_grad():
        B[1].running_mean.copy_(f32(rmean))
        B[1].running_var.copy_(f32(rvar))
    B[1].eval()
    ref = U.eval_unit(c.units['A']['z'].detach(), lv['wB'].detach(), lv['gammaB'].detach(), lv['betaB'].detach(), rmean, rvar, U.K311)
    tp = eng.tape.Tape(False)
    eng.reset()
    av = eng.layers.f_conv_bn_act(tp, *A, eng.tape.Var(f32(lv['x']), False))
    assert isinstance(av, eng.tape.LazyVar)
    bv = eng.layers.f_conv_bn_act(tp, *B, av)
    torch.cuda.synchronize()
    assert eng.names() == ['conv_fwd', 'bn_finalize', 'bn_apply', 'conv_fwd', 'bn_fold_eval', 'bn_apply'], eng.names()
    assert av.materialized and not isinstance(bv, eng.tape.LazyVar)
    recs = unit_records(eng.calls)
    check_first('R8 lazy->eval', mode, 'A', c.units['A'], recs[0], av.t, A[1])
    for name, got in (('y', recs[1]['y']), ('z', bv.t)):
        assert note('R8 lazy->eval', mode, 'B ' + name, rel_err(got, ref[name]), U.BARS[mode]) < U.BARS[mode]
    assert int(B[1].num_batches_tracked) == 0 and torch.equal(B[1].running_mean, f32(rmean))


# ----------------------------------------------------------------------------- a real SepConv3d at a lazy size
def run_sep(e, lazy):
    c = U.chain('sep')
    lv, mode = c.leaves, e.mode
    e.flag('LAZY_BN', lazy)
    e.pin('r3_a')
    e.pin('sep_t')
    sep = e.pkg.lib.modeling.backbone.backbone_3d.s3d_1.SepConv3d(8, 16, 3, 1, 1).to(DEV)
    units = {'A': (sep.conv_s, sep.bn_s), 'B': (sep.conv_t, sep.bn_t)}
    for tag, (conv, bn) in units.items():
        load(conv, bn, lv, tag)
    assert sep.bn_s.eps == U.SEP_BN['eps'] and sep.bn_t.momentum == U.SEP_BN['momentum']
    tp = e.tape.Tape(True)
    e.reset()
    bv = sep.fwd(tp, e.tape.Var(f32(lv['x']), False))
    fwd, recs = e.names(), unit_records(e.calls)
    zB = bv.t
    bv.grad = f32(c.seeds(U.BARS[mode])['zB'][0])
    backward(e, tp)
    out = dict(yA=recs[0]['y'], yB=recs[1]['y'], zB=zB, meanB=recs[1]['mean'], invstdB=recs[1]['invstd'],
               rmA=sep.bn_s.running_mean.clone(), rvB=sep.bn_t.running_var.clone())
    out.update(param_grads(units))
    return dict(c=c, fwd=fwd, bwd=e.names(), recs=recs, A=units['A'], B=units['B'], out=out)


@pytest.mark.parametrize('mode', U.MODES)
def test_sepconv3d_block_across_its_routes(eng, mode):
    """s3d_1.SepConv3d(8, 16, 3, 1, 1) at (2, 8, 4, 64, 65) (eps 1e-3, momentum 1e-3): conv_s lazy, conv_t through xf on the
    temporal64 kernel (split modes) -- against LAZY_BN off: same kernels, same bits, torch.equal for every output, statistic
    and parameter gradient; and both against fp64 (n as R3)."""
    eng.set_mode(mode)
    xf = mode != 'f32'
    r = run_sep(eng, True)
    assert r['fwd'] == (['conv_fwd', 'bn_finalize', 'conv_fwd_xf', 'bn_finalize'] if xf else
                        ['conv_fwd', 'bn_finalize', 'bn_apply', 'conv_fwd', 'bn_finalize']), r['fwd']
    assert r['bwd'] == ['bn_bwd:2', 'conv_wgrad:xf' if xf else 'conv_wgrad', 'conv_dgrad:new', 'bn_bwd:2', 'conv_wgrad'], r['bwd']
    check_two_units('SepConv3d', mode, r, R3_NS)
    eager = run_sep(eng, False)
    assert eager['fwd'] == ['conv_fwd', 'bn_train_fwd', 'conv_fwd', 'bn_train_fwd'], eager['fwd']
    same_bits(r['out'], eager['out'], ('SepConv3d lazy vs eager', mode))


