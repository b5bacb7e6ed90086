"""Every launch code of profiles/tune_cache.json on its own layer: bit for bit on dyadic operands, and against fp64 on float
operands.  One case per (arithmetic prefix, geometry) of the cache -- 165 cases for its 487 entries, built and explained by
tests/tuned_cases.py, their launches and operand preconditions asserted on the CPU by tests/test_tuned_cases.py.

A case whose layer is small runs as bench.py runs it: at the key's geometry, the committed cache loaded, the autotuner on, a
fresh conv_plan, the codes adopted by the tuner (w_raw passed so that it can re-pack).  A large layer runs on the shrunken
geometry of tuned_cases.build -- same channels, kernel, stride, padding and storage, fewer positions -- with its codes
pinned by plan.set_code.  In both, the device plan must resolve to the kernel and configuration the CPU plan of the same
codes resolves to before a number counts: a fallback to another kernel fails the test.

(a) Dyadic operands (tests/exact.py): y, the BatchNorm partials summed (sum y always; sum y^2 where the case's budget allows),
    dx, dw into a zeroed buffer and 2 dw after a second accumulate must equal the fp64 answer bit for bit; fp16 outputs must
    equal exact.to_f16 of it.  A wrong tile, split, box, tail or class index fails here whatever the arithmetic.
(b) Float operands (randn; weights scaled by sqrt(2 / (C taps)); fp16 numbers for the fp16-storage path), truth in fp64.  On
    dyadic data the mid / lo parts of a bf16 split are zero, so a wrong part index in a packed layout shows only here.  Errors
    are per element, relative to the sum of |terms| of that element.  Bars, derived and not tuned: f32 and bf16x6 1e-5 (the bar
    test_bf16x6_on_wide_range_tiny_and_cancelling_operands holds on this scale); bf16x3 5e-5 (the dropped lo x lo term is at
    most 2^-16 = 1.5e-5 of each product, the rest is margin for the fp32 accumulation); fp16 storage 1e-5 of the sum of
    |terms| (products of fp16 operands are exact in fp32), plus 2^-11 |ref| for the one rounding of an fp16 output.  Where a
    bar fails, the same operands run under the all-zero heuristic code and both figures are reported: a difference is a
    launch bug, equal errors are an arithmetic finding.

References: tuned_cases.conv_sums in fp64 (one matrix product per tap plane; equal to ATen in double bit for bit on dyadic
operands, tests/test_tuned_cases.py), on the CPU for small cases and on the device otherwise; shared by the arithmetic
prefixes that run the same geometry.

MEASURED on an MI355X (worst over the cases of a prefix, relative to the sum of |terms|; every case passes (a) and (b)):
  MEASURED tuned v15  (f32)    worst fwd 5.00e-07 @ v15-n32-c230-8x14x14-k128-311-s211-p100 / dgrad 3.71e-07 @
                               v15-n32-c64-8x28x28-k230-133-s122-p011 / wgrad 2.36e-07 @ v15-n32-c512-1x1x1-k128-111-s111-p000
  MEASURED tuned v15b (bf16x3) worst fwd 5.15e-06 @ v15b-n32-c3-16x112x112-k110-177-s122-p033 / dgrad 3.42e-06 @
                               v15b-n32-c144-8x28x28-k64-311-s111-p100 / wgrad 3.85e-06 @ v15b-n32-c512-1x4x4-k1152-133-s111-p011
  MEASURED tuned v15c (bf16x6) worst fwd 3.66e-07 @ v15c-n4-c64-8x56x56-k192-133-s111-p011 / dgrad 4.43e-07 @
                               v15c-n32-c144-8x28x28-k64-311-s111-p100 / wgrad 3.11e-07 @ v15c-n16-c2048-1x1x1-k2048-111-s111-p000
  MEASURED tuned v15h (fp16)   worst fwd 2.89e-08 @ v15h-n16-c128-8x28x28-k512-111-s111-p000 / dgrad 3.31e-08 @
                               v15h-n16-c512-4x14x14-k512-333-s222-p111 / wgrad 1.13e-07 @ v15h-n16-c512-4x14x14-k512-333-s222-p111
  (fp16 outputs: after the 2^-11 |ref| of their one rounding is taken off).  165 cases in 29 s, the longest (the 7x7x7 stem of
  the 3D-ResNet, 343 taps in the fp64 reference) a few seconds.
"""
import os

import pytest
import torch

import exact
import tuned_cases as tc
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CPU = torch.device('cpu')
F64 = torch.float64
ENTRIES = {e.id: e for e in tc.entries()}
BARS = {'f32': 1e-5, 'bf16x6': 1e-5, 'bf16x3': 5e-5, 'fp16': 1e-5}
PASSES = ('fwd', 'dgrad', 'wgrad')
WORST = {}              # prefix -> {pass: (error, case id)}
CPU_REFERENCE_MACS = 1 << 26


@pytest.fixture
def tuned(pkg):
    """bench.py's configuration (committed cache, autotuner on), everything restored afterwards."""
    ops = pkg.engine.ops
    saved = (ops.AUTOTUNE, dict(ops._TUNE_CACHE), ops._TUNE_DIRTY[0], ops.get_conv_math(), ops.DEFER[0])
    ops.AUTOTUNE, ops.DEFER[0] = True, None
    ops._TUNE_CACHE.clear()
    ops.load_tune_cache(os.path.join(ROOT, 'profiles', 'tune_cache.json'))
    ops._conv_plan.cache_clear()
    try:
        yield ops
    finally:
        ops.AUTOTUNE, ops.DEFER[0] = saved[0], saved[4]
        ops._TUNE_CACHE.clear()
        ops._TUNE_CACHE.update(saved[1])
        ops._TUNE_DIRTY[0] = saved[2]
        ops.set_conv_math(saved[3])
        ops._conv_plan.cache_clear()


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
    """A device fault is sticky: nothing of this module may go on launching on a faulted device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit('device fault, stopping the session: %s' % err, returncode=3)


def _ref_device(run):
    return CPU if tc.macs(run.geom) <= CPU_REFERENCE_MACS else DEV


def _on_device(ref):
    return {k: v.to(DEV) for k, v in ref.items()}


def _x_view(run, x64, half):
    """x on the device in the plan's storage type; where the key has a batch stride, the last C channels of a wider batch
    whose other channels hold other clips' values (reading the wrong slice is a wrong answer, not a zero)."""
    t = x64.to(DEV).half() if half else x64.float().to(DEV)
    xbs = run.geom[15]
    if not xbs:
        return t.contiguous()
    N, C, D, H, W = t.shape
    ctot = xbs // (D * H * W)
    assert ctot * D * H * W == xbs and ctot > C
    big = t.flip(0).repeat(1, -(-ctot // C), 1, 1, 1)[:, :ctot].contiguous()
    big[:, ctot - C:] = t
    view = big[:, ctot - C:]
    assert view.stride(0) == xbs
    return view


def _plan(ops, run):
    g = run.geom
    if run.shrunken:
        return tc.make_plan(g, run.entry.f16, DEV, run.codes)
    ops._conv_plan.cache_clear()
    plan = ops.conv_plan(g[:5], g[5], g[6:9], g[9:12], g[12:15], DEV, g[15], act_f16=run.entry.f16)
    assert plan.tuned == [False] * 3
    return plan


def _check_plan(ops, plan, run):
    """The device plan runs what the CPU plan of the same codes resolves to, under the codes of the cache."""
    for which, code in run.codes.items():
        got = [getattr(plan.g, 'tune_%s_%s' % (PASSES[which], f)) for f in code._fields]
        assert plan.tuned[which] and got == list(code), (which, got, code)
    want = tc.describe(tc.make_plan(run.geom, run.entry.f16, CPU, run.codes), run.geom, run.codes)
    assert tc.describe(plan, run.geom, run.codes) == want


def _passes(ops, plan, run, x, w, dy):
    """-> y, sum y, sum y^2 (partials folded in fp64), dx (None where the cache holds no dgrad code), dw, dw after a second
    accumulate."""
    y, (ss, sq) = ops.conv_fwd(plan, x, ops.conv_pack(plan, 0, w), None, stats=True, w_raw=w)
    dx = ops.conv_dgrad(plan, dy, ops.conv_pack(plan, 1, w), w_raw=w) if 1 in run.codes else None
    dw = torch.zeros_like(w)
    ops.conv_wgrad(plan, x, dy, dw, accumulate=True)
    dw1 = dw.clone()
    ops.conv_wgrad(plan, x, dy, dw, accumulate=True)
    return dict(y=y, sy=ss.double().sum(1), sq=sq.double().sum(1), dx=dx, dw=dw1, dw2=dw)


def _operands(run, c):
    half = run.entry.f16
    return _x_view(run, c['x'], half), c['w'].float().to(DEV), (c['dy'].to(DEV).half() if half else c['dy'].float().to(DEV))


def _eq(got, want, half=False):
    """Bit for bit: `got` holds exactly the fp64 values `want` (the one rounding to fp16 applied where the output is fp16)."""
    return torch.equal(got.double(), exact.to_f16(want).double() if half else want)


def _float_errors(run, out, ref, a):
    half = run.entry.f16

    def worst(got, r, s, f16_out):
        err = (got.double() - r).abs()
        if f16_out:
            err = (err - 2.0 ** -11 * r.abs()).clamp_min(0)
        return float((err / s.clamp_min(1e-300)).max())
    e = dict(fwd=worst(out['y'], ref['y'], a['y'], half), wgrad=worst(out['dw'], ref['dw'], a['dw'], False))
    if out['dx'] is not None:
        e['dgrad'] = worst(out['dx'], ref['dx'], a['dx'], half)
    return e


@pytest.mark.parametrize('cid', sorted(ENTRIES, key=lambda i: (ENTRIES[i].geom, i)))
def test_cached_launch_codes_exact_and_vs_fp64(pkg, tuned, cid):
    ops = tuned
    e = ENTRIES[cid]
    run = tc.build(e)
    ops.set_conv_math(e.mode)
    half = e.f16
    plan = _plan(ops, run)
    if run.shrunken:
        _check_plan(ops, plan, run)
    # ---- (a) dyadic operands: bit for bit
    main, stats = tc.pick_sets(run)
    c = tc.dyadic_case(run.geom, main, _ref_device(run))
    ref, b = _on_device(c['ref']), c['budgets']
    assert b['y'] < 1 and b['dx'] < 1 and 2 * b['dw'] < 1
    x, w, dy = _operands(run, c)
    out = _passes(ops, plan, run, x, w, dy)
    _check_plan(ops, plan, run)                     # (as cached: the tuner has adopted the entries by now)
    assert _eq(out['y'], ref['y'], half), ('y', cid, plan.cfg(0))
    if b['sy'] < 1:
        assert torch.equal(out['sy'], ref['sy']), ('sum y', cid, plan.cfg(0))
    if b['sq'] < 1:
        assert torch.equal(out['sq'], ref['sq']), ('sum y^2', cid, plan.cfg(0))
    if out['dx'] is not None:
        assert _eq(out['dx'], ref['dx'], half), ('dx', cid, plan.cfg(1))
    assert _eq(out['dw'], ref['dw']), ('dw', cid, plan.cfg(2))
    assert _eq(out['dw2'], 2 * ref['dw']), ('dw += dw', cid, plan.cfg(2))
    if stats != main:                               # the statistics, on operands whose per-channel sums stay exact
        c2 = tc.dyadic_case(run.geom, stats, _ref_device(run))
        ref2, b2 = _on_device(c2['ref']), c2['budgets']
        assert b2['y'] < 1 and b2['sy'] < 1
        x2, w2, _ = _operands(run, c2)
        y2, (ss, sq) = ops.conv_fwd(plan, x2, ops.conv_pack(plan, 0, w2), None, stats=True, w_raw=w2)
        assert _eq(y2, ref2['y'], half), ('y', stats, cid)
        assert torch.equal(ss.double().sum(1), ref2['sy']), ('sum y', stats, cid)
        if b2['sq'] < 1:
            assert torch.equal(sq.double().sum(1), ref2['sq']), ('sum y^2', stats, cid)
    # ---- (b) float operands against fp64, relative to the sum of |terms| per element
    f = tc.float_case(run.geom, half, _ref_device(run))
    fref, fabs = _on_device(f['ref']), _on_device(f['abs'])
    x, w, dy = _operands(run, f)
    errs = _float_errors(run, _passes(ops, plan, run, x, w, dy), fref, fabs)
    print('MEASURED tuned %s %s @ %s' % (e.prefix, ' '.join('%s %.2e' % (k, errs[k]) for k in PASSES if k in errs), cid))
    for k, v in errs.items():
        if v > WORST.setdefault(e.prefix, {}).get(k, (-1.0, ''))[0]:
            WORST[e.prefix][k] = (v, cid)
    bar = BARS[e.mode]
    if max(errs.values()) >= bar:
        heur = tc.make_plan(run.geom, half, DEV)                 # all-zero codes: the library's own heuristic launch
        herrs = _float_errors(run, _passes(ops, heur, run, x, w, dy), fref, fabs)
        pytest.fail('%s: bar %.0e missed under the cached codes %r, the heuristic launch gives %r (cfg %r / %r / %r)' % (
            cid, bar, errs, herrs, plan.cfg(0), plan.cfg(1), plan.cfg(2)))


def test_zz_worst_errors_per_prefix():
    """Prints the figures the module docstring records (runs last: after every case of the module)."""
    for prefix in sorted(WORST):
        print('MEASURED tuned %s worst %s' % (prefix, ' / '.join('%s %.2e @ %s' % ((k,) + WORST[prefix][k]) for k in PASSES
                                                                 if k in WORST[prefix])))
