"""Bit-exact checks of the conv kernels, their BatchNorm statistics and the fp16-storage path on dyadic operands
(tests/exact.py; every precondition is asserted on the CPU by tests/test_exact.py).

On these operands the fp64 reference is the exact answer and every fp32 partial sum in any order is exact, so each kernel
family, tile shape, split count and arithmetic mode must return the reference BIT FOR BIT: y, dx, dw, the per-channel sum of
y, and (on the NARROW operands) the per-channel sum of y^2.  An fp16 output must be the round-to-nearest-even cast of the
exact answer -- one rounding, also under accumulate=True, bias and split-K -- while the statistics of an fp16 layer must be
those of the unrounded accumulators.  The fp16 element-wise kernels (BatchNorm, pools) are held per element to an interval
derived from their own fp32 operation count, and to equality where their arithmetic is exact."""
import pytest
import torch
import torch.nn.functional as F

import exact
import ref64
from exact import F64, to_f16

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F16, F32 = torch.float16, torch.float32


@pytest.fixture(scope='module')
def ops(pkg):
    return pkg.engine.ops


@pytest.fixture(params=['f32', 'bf16x6', 'bf16x3'])
def mode(request, ops):
    """Every arithmetic mode of the fp32-storage kernels: on dyadic operands all three are exact."""
    default = ops.get_conv_math()
    ops.set_conv_math(request.param)
    yield request.param
    ops.set_conv_math(default)


@pytest.fixture
def split_mode(ops):
    """The default arithmetic restored after a test that switches it itself."""
    default = ops.get_conv_math()
    yield
    ops.set_conv_math(default)


def eq(got, want):
    """Bit for bit: the fp32 / fp16 tensor `got` holds exactly the fp64 values `want` (inf included, no NaN)."""
    return torch.equal(got.detach().cpu().double(), want.double())


def is_pos_zero(t):
    """Every element is +0 (bit pattern 0), not -0."""
    return bool((t.contiguous().view(torch.int16 if t.dtype is F16 else torch.int32) == 0).all())


def dev(t, half=False):
    return None if t is None else (t.to(DEV).half() if half else t.float().to(DEV))


def stat(ss):
    """Per-channel fold of the epilogue's partial sums, in fp64 (never an fp32 sum of the parts)."""
    return ss.double().sum(1).cpu()


def box_code(b):
    return b[0] | (b[1] << 8) | (b[2] << 16)


def _boxes(bn, q, m, k):
    """Every power-of-two box of bn positions whose halo fits the LDS-halo kernels (as tests/test_gpu_ops.py)."""
    out = []
    d = 1
    while d <= bn:
        h = 1
        while d * h <= bn:
            b = (d, h, bn // (d * h))
            P = 1
            for i in range(3):
                P *= (b[i] - 1) * m[i] + k[i]
            if P <= 384 and all(b[i] <= 4 * q[i] for i in range(3)):
                out.append(b)
            h *= 2
        d *= 2
    return out


def _plan(ops, c, **kw):
    plan = ops.ConvPlan(*c.shape, c.K, c.k, c.s, c.p, DEV, **kw)
    plan.tuned = [True, True, True]
    return plan


def _fwd_exact(ops, plan, c, xd, wd, tag, bias=None):
    y, (ss, sq) = ops.conv_fwd(plan, xd, ops.conv_pack(plan, 0, wd), bias, stats=True)
    want = c.ref['y'] if bias is not None else c.ref['y'] - (0 if c.bias is None else c.bias.view(1, -1, 1, 1, 1))
    assert eq(y, want), ('y', tag)
    assert torch.equal(stat(ss), c.ref['sy']), ('sum y', tag)
    if c.sq_exact:
        assert torch.equal(stat(sq), c.ref['sq']), ('sum y^2', tag)
    return y


# ============================================================================= fp32 storage: gather kernels
@pytest.mark.parametrize('name', ['g0', 'g1', 'g2', 'g3', 'g0n', 'g1n', 'g2n', 'g3n'])
def test_gather_kernels_every_launch_configuration_bit_exact(ops, mode, name):
    """Every tile height, the float4 variant, splits 1 and 3, two-phase launches and the wgrad tiles 1..10 (accumulate both
    ways) on the shapes of test_conv_every_launch_configuration.  The NARROW twins run the forward only: they are there for
    the sum of y^2."""
    c = exact.case(name)
    full = not c.sq_exact
    xd, wd, dyd = dev(c.x), dev(c.w), dev(c.dy)
    plan = _plan(ops, c)
    seen = set()
    for code in (32, 64, 96, 128, 160, 1024 + 32, 1024 + 64, 1024 + 128):
        for sp in (1, 3):
            plan.g.tune_fwd_bm = plan.g.tune_dgrad_bm = code
            plan.g.tune_fwd_splits = plan.g.tune_dgrad_splits = sp
            plan.refresh()
            seen.add((plan.cfg(0), plan.cfg(1)))
            assert plan.kernel(0) == 'gather' and plan.kernel(1) == 'gather'
            _fwd_exact(ops, plan, c, xd, wd, (code, sp, plan.cfg(0)))
            if full:
                assert eq(ops.conv_dgrad(plan, dyd, ops.conv_pack(plan, 1, wd)), c.ref['dx']), ('dx', code, sp, plan.cfg(1))
    assert len(seen) >= 8
    N = c.shape[0]
    for which, Ntot in ((0, c.ref['y'].numel() // c.K), (1, c.x.numel() // c.shape[1])):
        tilesN = -(-Ntot // 128)
        if tilesN < 2 or (which == 1 and (tuple(c.s) != (1, 1, 1) or not full)):
            continue
        # the seven (tall, short) pairs that run as one launch, then two that take one launch per phase
        for bm, tail in ((64, 1), (96, 1), (96, 2), (128, 1), (128, 2), (160, 1), (160, 2), (160, 3), (128, 3)):
            for mc in sorted({1, tilesN // 2, tilesN - 1}):
                if mc < 1:
                    continue
                plan.g.tune_fwd_bm = plan.g.tune_dgrad_bm = bm
                plan.g.tune_fwd_splits = plan.g.tune_dgrad_splits = 1
                plan.g.tune_fwd_tail = plan.g.tune_dgrad_tail = tail | (mc << 8)
                plan.refresh()
                if which == 0:
                    _fwd_exact(ops, plan, c, xd, wd, ('two-phase', bm, tail, mc))
                else:
                    assert eq(ops.conv_dgrad(plan, dyd, ops.conv_pack(plan, 1, wd)), c.ref['dx']), ('two-phase dx', bm, tail, mc)
    plan.g.tune_fwd_tail = plan.g.tune_dgrad_tail = 0
    if not full:
        return
    seen_w = set()
    for idx in range(1, 11):
        for sp in (1, 5):
            plan.g.tune_wgrad_tile, plan.g.tune_wgrad_splits = idx, sp
            plan.refresh()
            seen_w.add(plan.cfg(2)[:2])
            assert plan.kernel(2) == 'gather'
            dw = torch.full_like(wd, 0.5)
            ops.conv_wgrad(plan, xd, dyd, dw, accumulate=True)
            assert eq(dw, c.ref['dw'] + 0.5), ('dw +=', idx, sp, plan.cfg(2))
            ops.conv_wgrad(plan, xd, dyd, dw, accumulate=False)
            assert eq(dw, c.ref['dw']), ('dw', idx, sp, plan.cfg(2))
    assert len(seen_w) >= 6


# ============================================================================= fp32 storage: LDS-halo kernels
@pytest.mark.parametrize('name', ['h0', 'g1', 'h2', 'g2', 'h0n', 'g1n', 'h2n', 'g2n'])
def test_halo_kernels_every_configuration_bit_exact(ops, mode, name):
    """conv3d_halo.hip forward (y, sum y, sum y^2 on the NARROW twins) and dgrad (plain and += onto a dyadic base) over tile
    heights, boxes and splits as test_conv_halo_kernels_every_configuration thins them: a ragged box, a strided temporal
    window, 27 taps padded on all axes, four dgrad classes."""
    c = exact.case(name)
    full = not c.sq_exact
    xd, wd, dyd = dev(c.x), dev(c.w), dev(c.dy)
    base = exact.dgrad_base(c, False)
    plan = _plan(ops, c)
    k, s = c.k, c.s
    unit = tuple(s) == (1, 1, 1)
    qf, qd = tuple(c.out_shape[2:]), tuple(c.shape[2:])
    kd_cls = tuple(-(-k[i] // s[i]) for i in range(3))
    ran = [0, 0]
    for bn, rows_list in ((128, (32, 64, 96, 128, 160)), (256, (32, 64, 96, 128))):
        boxes_f = _boxes(bn, qf, s, k)
        boxes_d = _boxes(bn, qd if unit else tuple(-(-qd[i] // s[i]) for i in range(3)), (1, 1, 1), kd_cls)
        for bi, box in enumerate(sorted(set(boxes_f) | set(boxes_d))):
            for rows in (rows_list if bi % 3 == 0 else rows_list[bi % len(rows_list):][:1]):
                for sp in ((1, 2) if bi % 2 == 0 else (1,)):
                    plan.g.tune_fwd_bm = plan.g.tune_dgrad_bm = rows | 2048
                    plan.g.tune_fwd_box = plan.g.tune_dgrad_box = box_code(box)
                    plan.g.tune_fwd_splits = plan.g.tune_dgrad_splits = sp
                    plan.refresh()
                    if plan.kernel(0) == 'halo':
                        assert plan.cfg(0)[:2] == (rows, bn)
                        _fwd_exact(ops, plan, c, xd, wd, ('halo fwd', rows, box, sp))
                        ran[0] += 1
                    if plan.kernel(1) == 'halo' and full:
                        wt = ops.conv_pack(plan, 1, wd)
                        assert eq(ops.conv_dgrad(plan, dyd, wt), c.ref['dx']), ('halo dx', rows, box, sp)
                        acc = dev(base)
                        ops.conv_dgrad(plan, dyd, wt, acc, accumulate=True)
                        assert eq(acc, base + c.ref['dx']), ('halo dx +=', rows, box, sp)
                        ran[1] += 1
    assert (ran[0] >= 8 or not _boxes(128, qf, s, k)) and (ran[1] >= 8 or not full), ran
    if c.bias is None or not _boxes(128, qf, s, k):
        return
    # bias in the epilogue, the second view of a (b, 2C, T, H, W) batch read in place through the batch stride
    both = dev(torch.cat((exact.grid(c.shape, 8, 1 / 4, 98), c.x), dim=1))
    xv = torch.chunk(both, 2, dim=1)[1]
    pv = _plan(ops, c, x_batch_stride=xv.stride(0))
    pv.g.tune_fwd_bm, pv.g.tune_fwd_box = 64 | 2048, box_code(_boxes(128, qf, s, k)[0])
    pv.refresh()
    assert pv.kernel(0) == 'halo'
    _fwd_exact(ops, pv, c, xv, wd, 'view + bias', bias=dev(c.bias))


# ============================================================================= fp32 storage: stem forward kernel
@pytest.mark.parametrize('name', ['st0', 'st1'])
def test_stem_forward_kernel_bit_exact(ops, mode, name):
    """conv3d_stem.hip on the bias case and the one-channel case of test_conv_stem_kernel_vs_gather_and_aten: y (with bias),
    and the statistics of the conv proper, sum y^2 included (NARROW operands)."""
    c = exact.case(name)
    xd, wd, bd = dev(c.x), dev(c.w), dev(c.bias)
    plan = _plan(ops, c)
    for label, code in (('default', 0), ('stem', 4096 | 64), ('gather', 64)):
        plan.g.tune_fwd_bm = code
        plan.refresh()
        assert (plan.kernel(0) == 'stem') == (label != 'gather' and mode != 'f32'), (label, plan.kernel(0))
        _fwd_exact(ops, plan, c, xd, wd, label, bias=bd)


# ============================================================================= fp32 storage: temporal convs, tap dropping
@pytest.mark.parametrize('name', ['t0', 't1', 't2', 't3'])
def test_temporal_convs_that_drop_padding_taps_bit_exact(ops, mode, name):
    c = exact.case(name)
    xd, wd, dyd = dev(c.x), dev(c.w), dev(c.dy)
    plan = _plan(ops, c)
    _fwd_exact(ops, plan, c, xd, wd, name)
    assert eq(ops.conv_dgrad(plan, dyd, ops.conv_pack(plan, 1, wd)), c.ref['dx'])
    dw = torch.zeros_like(wd)
    ops.conv_wgrad(plan, xd, dyd, dw, accumulate=True)
    assert eq(dw, c.ref['dw'])


# ============================================================================= fp32 storage: streaming weight gradients
STREAMING = [(n, (11, 12)) for n in ('wt0', 'wt1', 'wt2', 'wt3')] + [(n, (13,)) for n in ('ws0', 'ws1', 'ws2', 'ws3')] + \
            [(n, (14,)) for n in ('wm0', 'wm1', 'wm2')]


@pytest.mark.parametrize('name,tiles', STREAMING, ids=[n for n, _ in STREAMING])
def test_streaming_weight_gradient_kernels_bit_exact(ops, mode, name, tiles):
    """conv3d_wgrad_ts.hip (tiles 11, 12, 13) and conv3d_wgrad_stem.hip (14): every split count of the existing tests, +=
    onto 0.5 and plain, a dense x and the second view of a clip pair read through the batch stride.  fp32-MFMA mode has no
    streaming kernel: it must fall back, and be exact there as well."""
    c = exact.case(name)
    N, C, D, Hh, W = c.shape
    big = dev(torch.cat((exact.grid(c.shape, 8, 1 / 4, 97), c.x), dim=1))
    dyd = dev(c.dy)
    units = {11: N * (Hh * W // 16), 12: N * (Hh * W // 16), 13: N * D * -(-W // 16), 14: N * c.out_shape[2]}
    for view in (False, True):
        xin = big[:, C:] if view else big[:, C:].contiguous()
        plan = _plan(ops, c, x_batch_stride=xin.stride(0) if view else 0)
        for tile in tiles:
            u = units[tile]
            for sp in sorted({1, 2, u, 4 * u} if tile == 14 else {1, 2, max(1, u // 8), max(1, u // 4)}):
                plan.g.tune_wgrad_tile, plan.g.tune_wgrad_splits = tile, sp
                plan.refresh()
                assert (plan.kernel(2) == ops.ConvPlan.WGRAD_KERNELS[tile]) == (mode != 'f32'), (tile, plan.cfg(2))
                dw = torch.full((c.K, C) + tuple(c.k), 0.5, device=DEV)
                ops.conv_wgrad(plan, xin, dyd, dw, accumulate=True)
                assert eq(dw, c.ref['dw'] + 0.5), ('dw +=', view, tile, sp, plan.cfg(2))
                ops.conv_wgrad(plan, xin, dyd, dw, accumulate=False)
                assert eq(dw, c.ref['dw']), ('dw', view, tile, sp, plan.cfg(2))


# ============================================================================= fp32 storage: fused BatchNorm+ReLU producer
@pytest.mark.parametrize('name', ['xf0', 'xf1'])
@pytest.mark.parametrize('math', ['bf16x6', 'bf16x3'])
def test_conv_on_a_fused_producer_bit_exact(ops, split_mode, math, name):
    """conv_fwd_xf / conv_wgrad(xf=...) with dyadic per-channel scale in {0.5, 1, 2} and shift in {-0.5, 0.25}: the conv of
    relu(y_in * scale + shift), its statistics and its weight gradient, also through the DeferredReduce collector."""
    y_in, scale, shift, c = exact.xf_case(name)
    ops.set_conv_math(math)
    N, C, D, Hh, W = c.shape
    kd = c.k[0]
    plan = _plan(ops, c)
    box = None
    for bd in (1, 2, 4, 8):
        for bh in (1, 2, 4, 8):
            bw = 128 // (bd * bh)
            if bd * bh * bw == 128 and bd <= 2 * D and bh <= 2 * Hh and bw <= 2 * W and (bd + kd - 1) * bh * bw <= 384:
                box = box or (bd, bh, bw)
    plan.g.tune_fwd_bm, plan.g.tune_fwd_box = 64 | 2048, box_code(box)
    plan.g.tune_wgrad_tile, plan.g.tune_wgrad_splits = 11, 2
    plan.refresh()
    assert plan.kernel(0) == 'halo' and plan.kernel(2) == 'temporal32' and ops.conv_xf_ok(plan)
    Cp = -(-C // 16) * 16 + 16                                   # padded rows, as bn_finalize hands them over
    sc, sf = torch.zeros(Cp, device=DEV), torch.zeros(Cp, device=DEV)
    sc[:C], sf[:C] = dev(scale), dev(shift)
    yd, wd, dyd = dev(y_in), dev(c.w), dev(c.dy)
    y, (ss, sq) = ops.conv_fwd_xf(plan, yd, sc[:C], sf[:C], ops.conv_pack(plan, 0, wd), stats=True)
    assert eq(y, c.ref['y']) and torch.equal(stat(ss), c.ref['sy'])
    dw = torch.full_like(wd, 0.5)
    ops.conv_wgrad(plan, yd, dyd, dw, accumulate=True, xf=(sc[:C], sf[:C]))
    assert eq(dw, c.ref['dw'] + 0.5)
    ops.conv_wgrad(plan, yd, dyd, dw, accumulate=False, xf=(sc[:C], sf[:C]))
    assert eq(dw, c.ref['dw'])
    coll = ops.DeferredReduce()
    g3 = torch.full_like(wd, 0.25)
    ops.DEFER[0] = coll
    try:
        ops.conv_wgrad(plan, yd, dyd, g3, accumulate=True, xf=(sc[:C], sf[:C]))
        coll.flush()
    finally:
        ops.DEFER[0] = None
    assert coll.launches == 1 and eq(g3, c.ref['dw'] + 0.25)


def test_deferred_reduce_collector_bit_exact(ops, mode):
    """Two layers' split-K weight gradients folded by ONE batched reduce launch, accumulate both ways."""
    ca, cb = exact.case('g0'), exact.case('g2')
    coll = ops.DeferredReduce()
    outs = []
    ops.DEFER[0] = coll
    try:
        for c, acc in ((ca, True), (cb, False)):
            plan = _plan(ops, c)
            plan.g.tune_wgrad_splits = 5
            plan.refresh()
            dw = torch.full((c.K, c.shape[1]) + tuple(c.k), 0.5, device=DEV)
            ops.conv_wgrad(plan, dev(c.x), dev(c.dy), dw, accumulate=acc)
            outs.append((dw, c.ref['dw'] + (0.5 if acc else 0.0)))
        coll.flush()
    finally:
        ops.DEFER[0] = None
    assert coll.launches == 1
    for dw, want in outs:
        assert eq(dw, want)


# ============================================================================= fp32 storage: split-K conv into a small BatchNorm
@pytest.mark.parametrize('name,halo', [('sk0', False), ('sk1', True), ('sk2', False)])
def test_conv_bn_small_fwd_y_and_folded_statistics_bit_exact(ops, name, halo):
    """gca_conv_fwd_slabs + gca_bn_train_fwd_slabs: y must be the exact conv; the mean the BatchNorm kernel folds from the
    slabs must be the exact sum over the count rounded ONCE to fp32, invstd the exact (sum y^2 / n - mean^2 + eps)^-1/2 to
    two fp32 roundings (eps crosses the ABI as a float; the kernel's own double arithmetic is below 1e-15)."""
    c = exact.case(name)
    N, K = c.shape[0], c.K
    plan = _plan(ops, c)
    xd, wd = dev(c.x), dev(c.w)
    gam, bet = torch.ones(K, device=DEV), torch.zeros(K, device=DEV)
    for sp in (2, 3, 5):
        plan.g.tune_fwd_bm, plan.g.tune_fwd_splits = (2048 + 64 if halo else 64), sp
        if halo:
            plan.g.tune_fwd_box = box_code(_boxes(128, tuple(c.out_shape[2:]), c.s, c.k)[0])
        plan.refresh()
        if plan.cfg(0)[2] < 2:
            continue
        assert plan.kernel(0) == ('halo' if halo else 'gather')
        SP = c.ref['y'][0, 0].numel()
        rm, rv, nb = torch.zeros(K, device=DEV), torch.ones(K, device=DEV), torch.zeros((), dtype=torch.long, device=DEV)
        y, z, mean, invstd, scale, shift = ops.conv_bn_small_fwd(plan, xd, ops.conv_pack(plan, 0, wd), N * SP, gam, bet, 1e-5, 0.1,
                                                                 rm, rv, nb, None, False)
        assert eq(y, c.ref['y']), (sp, plan.cfg(0))
        n = float(N * SP)
        m64 = c.ref['sy'] / n
        assert torch.equal(mean.cpu(), m64.float()), sp
        is64 = 1.0 / torch.sqrt(c.ref['sq'] / n - m64 * m64 + ref64.f32(1e-5))
        assert float(((invstd.cpu().double() - is64).abs() / is64).max()) <= 2.0 ** -23
        # running mean from the same fold: (1 - 0.1) * 0 + 0.1 * mean, one more fp32 rounding
        assert float((rm.cpu().double() - ref64.f32(0.1) * m64).abs().max()) <= 2.0 ** -23 * float(m64.abs().max()) and int(nb) == 1
        return
    pytest.fail('no launch shape with a split reduction was available')


# ============================================================================= fp32 storage: bias, Linear, strided 1x1x1
def test_linear_bias_dgrad_accumulate_and_bias_gradient_bit_exact(ops, mode):
    c = exact.case('lin')
    plan = _plan(ops, c)
    xd, wd, dyd = dev(c.x), dev(c.w), dev(c.dy)
    assert eq(ops.conv_fwd(plan, xd, ops.conv_pack(plan, 0, wd), dev(c.bias)), c.ref['y'])
    base = exact.dgrad_base(c, False)
    dx = dev(base)
    ops.conv_dgrad(plan, dyd, ops.conv_pack(plan, 1, wd), dx, accumulate=True)
    assert eq(dx, base + c.ref['dx'])
    db = torch.full((c.K,), 0.25, device=DEV)
    ops.bias_grad(dyd, c.shape[0], c.K, 1, db, True)
    assert eq(db, c.dy.sum((0, 2, 3, 4)) + 0.25)
    dw = torch.zeros_like(wd)
    ops.conv_wgrad(plan, xd, dyd, dw, accumulate=True)
    assert eq(dw, c.ref['dw'])


def test_strided_pointwise_dgrad_leaves_exact_positive_zeros(ops, mode):
    """A 1x1x1 stride-2 conv reaches one input position in eight; the others must be written as +0 (not left alone, not -0)."""
    c = exact.case('p2')
    plan = _plan(ops, c)
    xd, wd, dyd = dev(c.x), dev(c.w), dev(c.dy)
    _fwd_exact(ops, plan, c, xd, wd, 'p2')
    dx = torch.full(c.shape, float('nan'), device=DEV)
    ops.conv_dgrad(plan, dyd, ops.conv_pack(plan, 1, wd), dx, accumulate=False)
    assert eq(dx, c.ref['dx'])
    reached = torch.zeros(c.shape, dtype=torch.bool)
    reached[:, :, ::2, ::2, ::2] = True
    assert is_pos_zero(dx.cpu()[~reached]) and float((~reached).double().mean()) == 0.875
    dw = torch.zeros_like(wd)
    ops.conv_wgrad(plan, xd, dyd, dw, accumulate=True)
    assert eq(dw, c.ref['dw'])


@pytest.mark.parametrize('half', [False, True])
def test_all_zero_windows_give_positive_zero(ops, half):
    """Clip 0 is all zero: every product is a signed zero (the weights have both signs); the stored sum must be +0 in both
    storage types, forward and dgrad."""
    c = exact.case('f6')
    x, dy = c.x.clone(), c.dy.clone()
    x[0], dy[0] = 0.0, 0.0
    plan = _plan(ops, c, act_f16=half)
    y = ops.conv_fwd(plan, dev(x, half), ops.conv_pack(plan, 0, dev(c.w)))
    dx = ops.conv_dgrad(plan, dev(dy, half), ops.conv_pack(plan, 1, dev(c.w)))
    assert y.dtype is (F16 if half else F32)
    assert is_pos_zero(y.cpu()[0]) and is_pos_zero(dx.cpu()[0])


# ============================================================================= fp16 storage: one rounding, statistics unrounded
def _f16_all(ops, plan, c, tag, wgrad=True):
    """y == RNE(exact), sum y == exact sum (the statistics see the accumulators, not the stored values), dx == RNE(exact),
    dx += onto a dyadic fp16 base == RNE(base + exact): ONE rounding; dw (fp32) exact."""
    xh, dyh, wd, bd = dev(c.x, True), dev(c.dy, True), dev(c.w), dev(c.bias)
    y, (ss, sq) = ops.conv_fwd(plan, xh, ops.conv_pack(plan, 0, wd), bd, stats=True)
    assert y.dtype is F16
    assert torch.equal(y.cpu(), to_f16(c.ref['y'])), ('y', tag)
    assert torch.equal(stat(ss), c.ref['sy']), ('sum y', tag)
    wt = ops.conv_pack(plan, 1, wd)
    dx = ops.conv_dgrad(plan, dyh, wt)
    assert dx.dtype is F16 and torch.equal(dx.cpu(), to_f16(c.ref['dx'])), ('dx', tag)
    base = exact.dgrad_base(c, True)
    acc = dev(base, True)
    ops.conv_dgrad(plan, dyh, wt, acc, accumulate=True)
    assert torch.equal(acc.cpu(), to_f16(base + c.ref['dx'])), ('dx +=', tag)
    if wgrad:
        dw = torch.full_like(wd, 0.5)
        ops.conv_wgrad(plan, xh, dyh, dw, accumulate=True)
        assert dw.dtype is F32 and eq(dw, c.ref['dw'] + 0.5), ('dw', tag)


F16_KERNELS = {'f2': ('gather', 'gather'), 'f6': ('gather', 'gather'), 'f7': ('gather', 'gather'), 'f9': ('pw', 'pw'), 'f10': ('pw', 'pw'),
               'fst': ('stem', 'gather'), 'fp2': ('gather', 'gather'), 'fr': ('gather', 'gather')}


@pytest.mark.parametrize('name', sorted(F16_KERNELS))
def test_f16_storage_is_one_rounding_of_the_exact_answer(ops, name):
    """The layer kinds of tests/test_gpu_f16.py CONV_CASES (2, 6, 7, 9, 10, the strided 1x1x1 and the stem case) at one clip
    (the stem case whole), under the heuristic launch shapes (the halo kernels are forced in the next test): the kernel family each one runs on is asserted."""
    c = exact.case(name)
    plan = _plan(ops, c, act_f16=True)
    assert (plan.kernel(0), plan.kernel(1)) == F16_KERNELS[name]
    _f16_all(ops, plan, c, name)


def test_f16_storage_every_kernel_family_and_split_k(ops):
    """One layer (the ROUND reference shape) forced through the gather kernels (splits 1 and 3: the split-K finish does the
    rounding), the halo kernels (every candidate box, splits 1 and 2) and the wgrad tiles 1..10 with splits 1 and 5."""
    c = exact.case('fr')
    plan = _plan(ops, c, act_f16=True)
    fams = set()
    cands = [(cc.bm, cc.box) for which in (0, 1) for cc in ops.tune.halo_boxes(which, plan.g)]
    for code, box, sp in [(64, 0, 1), (64, 0, 3), (128, 0, 1), (1024 + 64, 0, 1)] + [(cd, bx, sp) for cd, bx in sorted(set(cands))[::3] for sp in (1, 2)]:
        plan.g.tune_fwd_bm = plan.g.tune_dgrad_bm = code
        plan.g.tune_fwd_box = plan.g.tune_dgrad_box = box
        plan.g.tune_fwd_splits = plan.g.tune_dgrad_splits = sp
        plan.refresh()
        fams.add((plan.kernel(0), plan.cfg(0)[2] > 1))
        _f16_all(ops, plan, c, (code, box, sp, plan.cfg(0), plan.cfg(1)), wgrad=False)
    assert {('gather', False), ('gather', True), ('halo', False), ('halo', True)} <= fams, fams
    xh, dyh = dev(c.x, True), dev(c.dy, True)
    for idx in range(1, 11):
        for sp in (1, 5):
            plan.g.tune_wgrad_tile, plan.g.tune_wgrad_splits = idx, sp
            plan.refresh()
            dw = torch.full((c.K, c.shape[1]) + tuple(c.k), 0.5, device=DEV)
            ops.conv_wgrad(plan, xh, dyh, dw, accumulate=True)
            assert eq(dw, c.ref['dw'] + 0.5), (idx, sp, plan.cfg(2))
            ops.conv_wgrad(plan, xh, dyh, dw, accumulate=False)
            assert eq(dw, c.ref['dw']), (idx, sp, plan.cfg(2))


@pytest.mark.parametrize('name', ['f9', 'f10'])
def test_f16_pointwise_and_gather_kernels_agree_bit_for_bit(ops, name):
    c = exact.case(name)
    plan = _plan(ops, c, act_f16=True)
    plan.g.tune_fwd_bm = plan.g.tune_dgrad_bm = 64
    plan.refresh()
    assert plan.kernel(0) == 'gather' and plan.kernel(1) == 'gather'
    _f16_all(ops, plan, c, name + ' gather', wgrad=False)


@pytest.mark.parametrize('name', ['fw0', 'fw2'])
def test_f16_stem_weight_gradient_kernel_bit_exact(ops, split_mode, name):
    c = exact.case(name)
    ops.set_conv_math('fp16')
    plan = _plan(ops, c, act_f16=True)
    xh, dyh = dev(c.x, True), dev(c.dy, True)
    units = c.shape[0] * c.out_shape[2]
    for sp in sorted({1, 2, units, 4 * units}):
        plan.g.tune_wgrad_tile, plan.g.tune_wgrad_splits = 14, sp
        plan.refresh()
        assert plan.kernel(2) == 'stem', plan.cfg(2)
        dw = torch.full((c.K, c.shape[1]) + tuple(c.k), 0.5, device=DEV)
        ops.conv_wgrad(plan, xh, dyh, dw, accumulate=True)
        assert eq(dw, c.ref['dw'] + 0.5), (sp, plan.cfg(2))
        ops.conv_wgrad(plan, xh, dyh, dw, accumulate=False)
        assert eq(dw, c.ref['dw']), (sp, plan.cfg(2))


# ============================================================================= fp16 edges
@pytest.mark.parametrize('kernel', ['pw', 'gather'])
def test_f16_store_overflows_to_inf_exactly_at_the_rounding_boundary(ops, kernel):
    """A pointwise conv whose weight rows are one-hot stores x[c] + bias.  Output channels 0..3 read input channel 0, where
    +-65504 are planted, with bias 8, -8, 16, -16: 65512 must store as 65504 (no early saturation to inf), 65520 -- the tie
    between 65504 and the first value fp16 cannot hold -- as +inf (no clamping: the loss-scale logic counts on inf), and the
    negatives likewise.  Everything else stays finite and exact."""
    c, o = exact.case('f9'), exact.overflow_operands()
    x, w, bias, want = o['x'], o['w'], o['bias'], to_f16(o['y'])
    plan = _plan(ops, c, act_f16=True)
    if kernel == 'gather':
        plan.g.tune_fwd_bm = 64
        plan.refresh()
    assert plan.kernel(0) == kernel
    y = ops.conv_fwd(plan, dev(x, True), ops.conv_pack(plan, 0, dev(w)), dev(bias)).cpu()
    got = y[0, :4, 0, 0, :4].double()
    inf = float('inf')
    assert got[0].tolist() == [65504.0, -65504.0, 65504.0, -65504.0]           # 65512 -> 65504, -65496 -> -65504
    assert got[1].tolist() == [65504.0, -65504.0, 65504.0, -65504.0]           # 65496 -> 65504, -65512 -> -65504
    assert got[2].tolist() == [inf, -65472.0, inf, -65472.0]                   # 65520 -> inf, -65488 (tie) -> even
    assert got[3].tolist() == [65472.0, -inf, 65472.0, -inf]
    assert torch.equal(y, want) and int(torch.isinf(y).sum()) == 4 and not bool(torch.isnan(y).any())


# What v_mfma_f32_32x32x16_f16 does with fp16 SUBNORMAL operands on gfx950: True = keeps them (IEEE), False = flushes them
# to zero.  Measured by the test below on an MI355X: kept (the IEEE expectation holds for dx and dw on the gather and the
# pointwise kernels); DESIGN.md, "what the exact-operand tests pin", records it.
MFMA_F16_KEEPS_SUBNORMAL_OPERANDS = True


@pytest.mark.parametrize('name', ['sub', 'subp'])
def test_f16_subnormal_gradients(ops, name):
    """dy = k 2^-22 are fp16 subnormals, w = k / 8: the exact dx holds odd multiples of 2^-25 -- below the smallest subnormal,
    ties -- and must be stored with one IEEE rounding (gradual underflow, no flush of the RESULT); dw (fp32) must be exact."""
    c = exact.case(name)
    plan = _plan(ops, c, act_f16=True)
    xh, dyh, wd = dev(c.x, True), dev(c.dy, True), dev(c.w)
    assert bool((dyh.cpu().double() == c.dy).all()) and float(c.dy.abs().max()) < 2.0 ** -14
    want_dx, want_dw = (c.ref['dx'], c.ref['dw']) if MFMA_F16_KEEPS_SUBNORMAL_OPERANDS else (torch.zeros_like(c.ref['dx']), torch.zeros_like(c.ref['dw']))
    dx = ops.conv_dgrad(plan, dyh, ops.conv_pack(plan, 1, wd)).cpu()
    dw = torch.zeros_like(wd)
    ops.conv_wgrad(plan, xh, dyh, dw, accumulate=True)
    ieee = torch.equal(dx, to_f16(c.ref['dx'])), eq(dw, c.ref['dw'])
    flushed = not bool(dx.any()), not bool(dw.any())
    print('MEASURED %s (%s dgrad, %s wgrad): IEEE dx %s dw %s; all-zero dx %s dw %s' % ((name, plan.kernel(1), plan.kernel(2)) + ieee + flushed))
    assert torch.equal(dx, to_f16(want_dx)) and eq(dw, want_dw)


# ============================================================================= fp16 element-wise kernels: derived interval
def within(out, r, E):
    """to_f16(r - E) <= out <= to_f16(r + E), element by element (fp16 rounding is monotonic)."""
    o = out.detach().cpu().double()
    return bool(((o >= to_f16(r - E).double()) & (o <= to_f16(r + E).double())).all())


U = 2.0 ** -23          # per fp32 operation: covers a truncating step as well as a rounding one


@pytest.mark.parametrize('shape,res', [((3, 6, 2, 5, 7), True), ((2, 8, 2, 4, 4), False), ((2, 5, 4, 50, 52), True)])
def test_bn_f16_kernels_per_element_against_fp64(ops, shape, res):
    """bn_apply / bn_train_fwd / bn_bwd on fp16 maps (shapes of test_bn_f16_storage_vs_f32_kernels: scalar and float4 paths,
    the one-launch small form and the three-pass form), every element inside the interval its fp32 expression allows.
      apply:  relu(x * scale + shift [+ res])                m = 3 (mul, add, add), operands |x scale|, |shift|, |res|
      bwd dx: A (d - B - (x - mu) is Cc)                     m = 10: sub, mul, mul, sub, sub, mul, the fp32 cast of B, and
              for Cc two roundings inside its terms ((x - mu) is in fp32) and its cast (the three-pass form also rounds its
              partial sums to fp32: inside the same count); operands |A| (|d|, mean |d| >= |B|, |xhat| mean |d xhat| >= |xhat Cc|)
      dres:   d, or old + d                                  m = 1
    The kernel's own fp32 scale / shift, and its stored z as the ReLU mask, are taken as given."""
    torch.manual_seed(2)
    N, Cc = shape[:2]
    SP = shape[2] * shape[3] * shape[4]
    x = (torch.randn(shape) * 1.5 + 0.3).half().to(DEV)
    r = torch.randn(shape).half().to(DEV) if res else None
    dz = torch.randn(shape).half().to(DEV)
    gam, bet = torch.rand(Cc, device=DEV) + 0.5, torch.randn(Cc, device=DEV)
    rm, rv, nbt = torch.zeros(Cc, device=DEV), torch.ones(Cc, device=DEV), torch.zeros((), dtype=torch.long, device=DEV)
    ss, sq = ops.bn_stats(x, N, Cc, SP)
    z, mean, invstd, scale, shift = ops.bn_train_fwd(ss, sq, N * SP, gam, bet, 1e-5, 0.1, rm, rv, nbt, x, r, True, N, Cc, SP)
    z2 = ops.bn_apply(x, scale, shift, r, True, N, Cc, SP)
    v = lambda t: ref64.d(t).view(1, -1, 1, 1, 1)
    x64, r64, d64 = ref64.d(x), ref64.d(r), ref64.d(dz)
    lin = x64 * v(scale) + v(shift) + (0 if r is None else r64)
    E = 3 * U * ((x64 * v(scale)).abs() + v(shift).abs() + (0 if r is None else r64.abs()))
    for out in (z, z2):
        assert out.dtype is F16
        o = out.cpu().double()
        assert bool(((o >= to_f16(torch.relu(lin - E)).double()) & (o <= to_f16(torch.relu(lin + E)).double())).all())
    assert torch.equal(z, z2)
    mask = (ref64.d(z) > 0).double()
    sv = ref64.bn_bwd_saved(dz.reshape(N, Cc, -1), x.reshape(N, Cc, -1), gam, mean, invstd, mask.reshape(N, Cc, -1))
    dm = d64 * mask
    xhat = (x64 - v(mean)) * v(invstd)
    n = float(N * SP)
    S = (dm * xhat).abs().sum((0, 2, 3, 4)) / n
    A = (ref64.d(gam) * ref64.d(invstd)).view(1, -1, 1, 1, 1)
    Bs = dm.abs().sum((0, 2, 3, 4)) / n
    Eb = 10 * U * A.abs() * (dm.abs() + Bs.view(1, -1, 1, 1, 1) + xhat.abs() * S.view(1, -1, 1, 1, 1))
    dg, db = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    dres = torch.empty_like(z) if res else None
    dx = ops.bn_bwd(dz, z, x, gam, mean, invstd, 1, N, Cc, SP, dg, db, dres, False)
    assert dx.dtype is F16 and within(dx, sv['dx'].reshape(shape), Eb)
    if res:
        assert torch.equal(dres.cpu().double(), dm)                                 # a masked copy
        acc = dz.clone()
        ops.bn_bwd(dz, z, x, gam, mean, invstd, 1, N, Cc, SP, torch.zeros_like(dg), torch.zeros_like(db), acc, True)
        assert within(acc, d64 + dm, U * (d64.abs() + dm.abs()))
    else:
        dg2, db2 = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
        dx2 = ops.bn_bwd(dz, None, x, gam, mean, invstd, 2, N, Cc, SP, dg2, db2, None, False, scale, shift)
        assert torch.equal(dx2, dx)                                                  # the mask recomputed from x is the same mask


def test_wavgpool_bwd_and_fused_maxpool_f16_per_element_against_fp64(ops):
    """wavgpool_bwd(float16): dy * norm * wt[d], m = 2, one operand.  maxpool_fwd with the fused BatchNorm+ReLU producer on an
    fp16 map: max over the window of relu(x * scale + shift), m = 2 (mul, add), operands |x scale|, |shift|; max and relu are
    monotonic, so the bound of a window is the largest bound in it."""
    torch.manual_seed(4)
    shape = (3, 7, 4, 5, 6)
    wt = torch.tensor([1., 2., 2., 1.], device=DEV)
    dy = torch.randn(3, 7, device=DEV)
    for w_, norm in ((None, 1.0 / 120), (wt, 1.0 / 180)):
        dx = ops.wavgpool_bwd(dy, w_, norm, shape, F16)
        r = ref64.d(dy).view(3, 7, 1, 1, 1) * ref64.f32(norm) * (1.0 if w_ is None else ref64.d(w_).view(1, 1, 4, 1, 1)) * torch.ones(shape, dtype=F64)
        assert dx.dtype is F16 and within(dx, r, 2 * U * r.abs())
    for shp, k, s, p in (((2, 5, 8, 18, 18), (3, 3, 3), (2, 2, 2), (1, 1, 1)), ((2, 4, 3, 9, 10), (1, 3, 3), (1, 2, 2), (0, 1, 1)),
                         ((1, 2, 5, 7, 9), (3, 2, 1), (1, 1, 1), (1, 1, 0))):
        x = torch.randn(shp).half().to(DEV)
        sc, sh = torch.rand(shp[1], device=DEV) + 0.5, torch.randn(shp[1], device=DEV)
        plan = ops.pool_plan(shp, k, s, p)
        y, _ = ops.maxpool_fwd(plan, x, scale=sc, shift=sh)
        v = lambda t: ref64.d(t).view(1, -1, 1, 1, 1)
        lin = ref64.d(x) * v(sc) + v(sh)
        E = 2 * U * ((ref64.d(x) * v(sc)).abs() + v(sh).abs())
        lo, hi = F.max_pool3d(torch.relu(lin - E), k, s, p), F.max_pool3d(torch.relu(lin + E), k, s, p)
        o = y.cpu().double()
        assert y.dtype is F16 and bool(((o >= to_f16(lo).double()) & (o <= to_f16(hi).double())).all())


def test_f16_elementwise_kernels_are_equalities_on_dyadic_operands(ops):
    """Dyadic scale / shift / residual / dy (tests/exact.py elementwise_operands): every fp32 step is exact, so bn_apply,
    maxpool_bwd (accumulate included) and axpy must store exactly RNE of the fp64 value."""
    v = lambda t: t.view(1, -1, 1, 1, 1)
    for shape in exact.ELEMENTWISE_SHAPES:
        e = exact.elementwise_operands(shape)
        N, Cc = shape[:2]
        SP = shape[2] * shape[3] * shape[4]
        xh, rh = dev(e['x'], True), dev(e['res'], True)
        sc, sf = dev(e['scale']), dev(e['shift'])
        for res in (None, rh):
            for relu in (False, True):
                z = ops.bn_apply(xh, sc, sf, res, relu, N, Cc, SP)
                want = e['x'] * v(e['scale']) + v(e['shift']) + (0 if res is None else e['res'])
                assert torch.equal(z.cpu(), to_f16(torch.relu(want) if relu else want)), (shape, res is not None, relu)
    e = exact.elementwise_operands(exact.ELEMENTWISE_SHAPES[0])
    shape = e['shape']
    xh, rh = dev(e['x'], True), dev(e['res'], True)
    a = xh.clone()
    ops.axpy(a, rh, 0.5)
    assert torch.equal(a.cpu(), to_f16(e['x'] + 0.5 * e['res']))
    for k, s, p in (((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((1, 3, 3), (1, 2, 2), (0, 1, 1)), ((2, 2, 2), (2, 2, 2), (0, 0, 0))):
        plan = ops.pool_plan(shape, k, s, p)
        xr = e['x'].clone().requires_grad_(True)
        yr = F.max_pool3d(xr, k, s, p)
        dy = exact.grid(yr.shape, 512, 1 / 64, 93)
        yr.backward(dy)
        y, am = ops.maxpool_fwd(plan, xh)
        assert torch.equal(y.cpu().double(), yr.detach())
        dx = ops.maxpool_bwd(plan, dev(dy, True), am)
        assert dx.dtype is F16 and torch.equal(dx.cpu(), to_f16(xr.grad)), (k, 'dx')
        acc = rh.clone()
        ops.maxpool_bwd(plan, dev(dy, True), am, acc, True)
        assert torch.equal(acc.cpu(), to_f16(e['res'] + xr.grad)), (k, 'dx +=')


# ============================================================================= gca_avgpool3d_*
@pytest.mark.parametrize('shape,k', exact.AVGPOOL_CASES)
def test_avgpool_fwd_bwd_against_aten_fp64(ops, shape, k):
    """nn.AvgPool3d(kernel_size=k): dyadic input and power-of-two windows make every result an equality.  Trailing rows /
    columns / frames that fill no window are dropped and their gradient is an exact +0; accumulate=True adds to a live buffer."""
    o = exact.avgpool_operands(shape, k)
    plan = ops.pool_plan(shape, k, k, (0, 0, 0))
    assert tuple(plan.out_shape) == tuple(o['y'].shape)
    assert eq(ops.avgpool_fwd(plan, dev(o['x'])), o['y'])
    dx = torch.full(shape, float('nan'), device=DEV)
    ops.avgpool_bwd(plan, dev(o['dy']), dx, False)
    assert eq(dx, o['dx'])
    cover = torch.zeros(shape, dtype=torch.bool)
    cover[:, :, :o['y'].shape[2] * k[0], :o['y'].shape[3] * k[1], :o['y'].shape[4] * k[2]] = True
    assert is_pos_zero(dx.cpu()[~cover])
    acc = dev(o['base'])
    ops.avgpool_bwd(plan, dev(o['dy']), acc, True)
    assert eq(acc, o['base'] + o['dx'])
    assert eq(ops.avgpool_bwd(plan, dev(o['dy'])), o['dx'])
