"""CPU checks of tests/exact.py: every precondition the bit-exact GPU tests (tests/test_gpu_exact.py) rely on holds for
the seeded operands they use -- the sums stay inside fp32's integer range in any order, the rounding cases really hold
thousands of values fp16 cannot represent and hundreds of exact ties -- and the expected fp16 value (`to_f16`) agrees with
round-to-nearest-even done in integer arithmetic."""
import pytest
import torch
import torch.nn.functional as F

import exact
from exact import F64


@pytest.mark.parametrize('name', sorted(exact.CASES))
def test_case_is_exact_in_fp32_in_any_summation_order(name):
    c = exact.case(name)
    b = c.budgets()
    y, dx = c.ref['y'], c.ref['dx']
    counts = [(exact.n_inexact(t), exact.n_ties(t)) for t in (y, dx)]
    print('EXACT %-4s %-6s per-element y %.2e dx %.2e dw %.2e | per-channel sum|y| %.2e sum y^2 %.2e | inexact / ties: y %d / %d, dx %d / %d'
          % ((name, c.set, b['y'], b['dx'], b['dw'], b['sy'], b['sq']) + counts[0] + counts[1]))
    assert b['y'] < 1 and b['dx'] < 1 and b['dw'] < 1 and b['sy'] < 1
    if c.sq_exact:
        assert b['sq'] < 1
    if name in exact.ROUND_CASES:
        for n_in, n_tie in counts:                              # y and dx each, never pooled
            assert n_in >= exact.MIN_INEXACT and n_tie >= exact.MIN_TIES
        assert bool(torch.isfinite(exact.to_f16(y)).all()) and bool(torch.isfinite(exact.to_f16(dx)).all())
    # accumulate=True: the sum onto the live buffer must be exact too (dx onto dgrad_base, dw onto a constant)
    for half in ((False, True) if c.set != 'SUBN' else ()):          # (the subnormal cases are never accumulated)
        base = exact.dgrad_base(c, half)
        if half:
            assert torch.equal(base.half().double(), base)
        assert exact.exact_in_fp32(c.abs['dx'] + base.abs(), min(c.udy * c.uw, 1 / 32)) < 1
    assert exact.exact_in_fp32(c.abs['dw'] + max(exact.WGRAD_BASES), min(c.ux * c.udy, 1 / 4)) < 1
    if name in exact.ROUND_CASES:
        acc = exact.dgrad_base(c, True) + dx
        assert exact.n_inexact(acc) >= exact.MIN_INEXACT and exact.n_ties(acc) >= exact.MIN_TIES
    # the operands themselves: at most 6 significant bits (the hi part of a bf16 split holds 8) and fp16 numbers.
    # (A batch-strided view changes only what lies BETWEEN the clips of x: the same operands, the same budgets.)
    for t in (c.x, c.w, c.dy):
        assert torch.equal(t.bfloat16().double(), t)
    assert torch.equal(c.x.half().double(), c.x) and torch.equal(c.w.half().double(), c.w) and torch.equal(c.dy.half().double(), c.dy)


@pytest.mark.parametrize('name', ['xf0', 'xf1'])
def test_fused_producer_operands_stay_dyadic(name):
    y_in, scale, shift, c = exact.xf_case(name)
    b = c.budgets()
    print('EXACT xf %s per-element y %.2e dw %.2e | sum|y| %.2e' % (name, b['y'], b['dw'], b['sy']))
    assert b['y'] < 1 and b['dw'] < 1 and b['sy'] < 1
    z32 = torch.relu(y_in.float() * scale.float().view(1, -1, 1, 1, 1) + shift.float().view(1, -1, 1, 1, 1))
    assert torch.equal(z32.double(), c.x) and torch.equal(c.x.bfloat16().double(), c.x)      # no rounding, fits one bf16 part
    assert float((c.x == 0).double().mean()) > 0.2 and set(scale.tolist()) == {0.5, 1.0, 2.0} and set(shift.tolist()) == {-0.5, 0.25}


def test_subnormal_cases_hold_subnormal_operands_and_sub_quantum_products():
    """dy = k 2^-22 (|k| <= 4) are fp16 subnormals; times w = k / 8 the products are multiples of 2^-25, half the
    smallest subnormal (2^-24): sums land on ties and on values below the quantum."""
    for name in ('sub', 'subp'):
        c = exact.case(name)
        nz = c.dy[c.dy != 0].abs()
        assert float(nz.max()) < 2.0 ** -14 and torch.equal(c.dy.half().double(), c.dy)
        dx = c.ref['dx']
        assert float(dx.abs().max()) < 2.0 ** -14 * 64
        assert exact.n_inexact(dx) >= 100 and exact.n_ties(dx) >= 100
        assert int(((dx != 0) & (exact.to_f16(dx) == 0)).sum()) >= 1          # some round to zero (the 2^-25 tie goes to even)


@pytest.mark.parametrize('name', ['fr', 'f9', 'sub'])
def test_to_f16_is_one_rounding_to_nearest_even(name):
    c = exact.case(name)
    for r in (c.ref['y'], c.ref['dx']):
        flat = r.flatten()
        idx = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(1))[:1000]
        want = torch.tensor([exact.rne_f16_integer(float(v)) for v in flat[idx]], dtype=F64)
        assert torch.equal(exact.to_f16(flat[idx]).double(), want)


def test_rne_boundaries():
    for v, want in ((65504.0, 65504.0), (65512.0, 65504.0), (65519.99, 65504.0), (65520.0, float('inf')), (-65520.0, -float('inf')),
                    (2.0 ** -25, 0.0), (3 * 2.0 ** -25, 2.0 ** -23), (2.0 ** -24, 2.0 ** -24), (2049.0, 2048.0), (2051.0, 2052.0),
                    (1 + 2.0 ** -11, 1.0), (1 + 3 * 2.0 ** -11, 1 + 2.0 ** -9)):
        assert exact.rne_f16_integer(v) == want, v
        assert float(exact.to_f16(torch.tensor([v], dtype=F64)).double()) == want, v
    r = torch.tensor([2049.0, 2050.0, 2049.5, 0.5, 2.0 ** -25, 65520.0], dtype=F64)
    assert exact.n_inexact(r) == 3 and exact.n_ties(r) == 3


def test_conv_ref_against_a_direct_sum():
    """conv_ref (ATen in double) against the definition written out, on one small padded, strided case."""
    x, w, b = exact.grid((1, 2, 3, 4, 5), 8, 0.25, 1), exact.grid((3, 2, 2, 3, 2), 8, 0.125, 2), exact.grid((3,), 8, 1 / 32, 3)
    s, p = (1, 2, 1), (1, 1, 0)
    r = exact.conv_ref(x, w, b, s, p)
    xp = F.pad(x, (p[2], p[2], p[1], p[1], p[0], p[0]))
    want = torch.zeros_like(r['y'])
    for od in range(want.shape[2]):
        for oh in range(want.shape[3]):
            for ow in range(want.shape[4]):
                win = xp[0, :, od * s[0]:od * s[0] + 2, oh * s[1]:oh * s[1] + 3, ow * s[2]:ow * s[2] + 2]
                want[0, :, od, oh, ow] = (w * win).sum((1, 2, 3, 4)) + b
    assert torch.equal(r['y'], want)
    assert torch.equal(r['sy'], (want - b.view(1, -1, 1, 1, 1)).sum((0, 2, 3, 4)))


@pytest.mark.parametrize('shape', exact.ELEMENTWISE_SHAPES)
def test_elementwise_operands_are_exact_in_fp32_and_exercise_the_fp16_rounding(shape):
    e = exact.elementwise_operands(shape)
    v = lambda t: t.view(1, -1, 1, 1, 1)
    for t in (e['x'], e['res']):
        assert torch.equal(t.half().double(), t)
    want = e['x'] * v(e['scale']) + v(e['shift']) + e['res']
    got = (e['x'].float() * v(e['scale']).float() + v(e['shift']).float()) + e['res'].float()           # every step in fp32
    assert torch.equal(got.double(), want) and exact.exact_in_fp32(want, 2.0 ** -12) < 1
    assert torch.equal((e['x'].float() + 0.5 * e['res'].float()).double(), e['x'] + 0.5 * e['res'])
    print('EXACT elementwise %s: inexact %d ties %d of %d' % (shape, exact.n_inexact(want), exact.n_ties(want), want.numel()))
    assert exact.n_inexact(want) >= want.numel() // 4 and exact.n_ties(want) >= 100


def test_overflow_operands_sit_on_the_fp16_boundary():
    o = exact.overflow_operands()
    assert exact.exact_in_fp32(o['x'].abs().max() + o['bias'].abs().max(), 1 / 4) < 1          # one product + bias per output
    assert torch.equal(o['x'].half().double(), o['x'])
    y = o['y'][0, :4, 0, 0, :4]
    assert y[0].tolist() == [65512.0, -65496.0, 65512.0, -65496.0] and y[2].tolist() == [65520.0, -65488.0, 65520.0, -65488.0]
    assert y[1].tolist() == [65496.0, -65512.0, 65496.0, -65512.0] and y[3].tolist() == [65488.0, -65520.0, 65488.0, -65520.0]
    want = exact.to_f16(o['y'])
    assert int(torch.isinf(want).sum()) == 4 and int((o['y'].abs() >= 65520).sum()) == 4


@pytest.mark.parametrize('shape,k', exact.AVGPOOL_CASES)
def test_avgpool_operands_are_exact_in_fp32(shape, k):
    o = exact.avgpool_operands(shape, k)
    win = k[0] * k[1] * k[2]
    assert win in (4, 8)                                                                # power of two: the division is exact
    assert exact.exact_in_fp32(F.avg_pool3d(o['x'].abs(), k) * win, 1 / 8) < 1         # the window sums
    assert exact.exact_in_fp32(o['dx'].abs() + o['base'].abs(), 1 / 64) < 1            # accumulate=True
    got = F.avg_pool3d(o['x'].float(), k)
    assert torch.equal(got.double(), o['y'])                                            # fp32 arithmetic reproduces fp64
    dropped = any(shape[2 + i] % k[i] for i in range(3))
    cover = torch.zeros(shape, dtype=torch.bool)
    cover[:, :, :o['y'].shape[2] * k[0], :o['y'].shape[3] * k[1], :o['y'].shape[4] * k[2]] = True
    assert (int((~cover).sum()) > 0) == dropped and bool((o['dx'][~cover] == 0).all())


def test_zero_window_case_has_weights_of_both_signs():
    """The signed-zero test zeroes clip 0 of case f6: its products are then +0 and -0 in about equal numbers."""
    w = exact.case('f6').w
    assert int((w > 0).sum()) > w.numel() // 3 and int((w < 0).sum()) > w.numel() // 3
