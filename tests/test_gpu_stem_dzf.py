"""Fused stem backward on the GPU: gca_bn_bwd_sums + gca_conv_wgrad_dzf (the stem weight-gradient kernel forming
dy = BatchNorm-backward(dz, y) in registers) against tests/ref64.py in fp64 and against the unfused path (gca_bn_bwd, then
gca_conv_wgrad) on the same inputs, through the C ABI.

Shapes.  The stem kernel takes OW % 8 == 0 only (tests/test_host_logic.py pins that refusal), so the smallest maps with an odd
OH and a partial 16-position step are 34 x 48 inputs (OH = 17, OW = 24: the second step of a row is half valid, and with one
split per 8-row chunk the last chunk holds one row); 34 x 38 (OW = 19) and 34 x 34 (OW = 17) are refused, which
tests/test_stem_dzf_host.py asserts.  N * SP = 2448 / 1632 here, below the one-workgroup threshold of gca_bn_bwd: the unfused
path then takes its sums in bn_bwd_small_kernel, so "same kernels, same bits" for dgamma / dbeta holds by construction only in
the layer-level case (N * SP = 41472); on the small maps the two routes fold one fp32 partial per channel through fp64 and
agree to the bit unless an fp64 sum lands within 2^-53 of an fp32 rounding boundary.

Bars.  dW against fp64: the bars of tests/test_gpu_ops.py::test_conv_wgrad_stem_kernel -- 1e-5 bf16x6, 5e-5 bf16x3, and for
fp16 storage its 2e-3 (the reference here is fp64 throughout, it does not round dy to fp16 as both GPU paths do; that test's
1e-5 is for a reference differentiated on rounded tensors).  And never worse than 1.5 x the unfused path's error on the same
inputs.  On dyadic operands (tests/exact.py's recipe: every sum of the BatchNorm exact, mean / invstd / gamma powers of two or
quarter integers) both routes see the same B and Cc, so dy and dW must agree bit for bit."""
import ctypes as C

import pytest
import torch

import exact
import ref64
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BARS = {'bf16x6': 1e-5, 'bf16x3': 5e-5, 'fp16': 2e-3}

# id -> (x shape, K, kernel, padding, arithmetic modes)
SHAPES = {
    'r2p1d': ((2, 3, 3, 34, 48), 110, (1, 7, 7), (0, 3, 3), ('bf16x6', 'bf16x3')),      # four row tiles, rows 110..127 dead
    's3d': ((2, 3, 3, 34, 48), 64, (1, 7, 7), (0, 3, 3), ('bf16x6', 'bf16x3')),         # two row tiles, two waves share the steps
    'r3d': ((1, 3, 4, 34, 48), 64, (7, 7, 7), (3, 3, 3), ('fp16',)),                    # two tap planes per workgroup, fp16 storage
}
CASES = [(sid, mode) for sid, v in SHAPES.items() for mode in v[4]]


@pytest.fixture(scope='module')
def ops(pkg):
    return pkg.engine.ops


def _out_shape(shape, K, k, p):
    N, _, D, Hh, W = shape
    return (N, K, D + 2 * p[0] - k[0] + 1, (Hh + 2 * p[1] - k[1]) // 2 + 1, (W + 2 * p[2] - k[2]) // 2 + 1)


_INPUTS = {}


def _inputs(sid, dyadic, half):
    """Seeded CPU operands of one shape + the fp64 reference per ReLU mode, built once and shared.  y is drawn so that the ReLU
    mask is mixed; channel 1 has a shift that masks every position (its dz contributes nothing, its dy is constant zero)."""
    key = (sid, dyadic, half)
    if key in _INPUTS:
        return _INPUTS[key]
    shape, K, k, p, _ = SHAPES[sid]
    osh = _out_shape(shape, K, k, p)
    g = torch.Generator().manual_seed(len(sid) * 100 + K + dyadic)
    if dyadic:
        x, y, dz = exact.grid(shape, 8, 1 / 4, 11).float(), exact.grid(osh, 8, 1 / 4, 12).float(), exact.grid(osh, 8, 1 / 4, 13).float()
        pick = lambda vals: torch.tensor(vals)[torch.randint(0, len(vals), (K,), generator=g)]
        gamma, invstd, mean = pick([0.5, 1.0, 2.0]), pick([0.5, 1.0, 2.0]), pick([-0.5, -0.25, 0.0, 0.25, 0.5])
        beta = pick([-0.5, 0.0, 0.25])
    else:
        x, y, dz = torch.randn(shape, generator=g), torch.randn(osh, generator=g) * 1.5 + 0.3, torch.randn(osh, generator=g)
        gamma, beta = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.3
    cast = (lambda t: t.half()) if half else (lambda t: t)
    x, y, dz = cast(x), cast(y), cast(dz)
    if not dyadic:                                     # the batch statistics of the tensor the kernels read, as the forward saves them
        y3 = y.double().reshape(osh[0], K, -1)
        mean = y3.mean((0, 2)).float()
        invstd = (1.0 / torch.sqrt(y3.var((0, 2), unbiased=False) + 1e-5)).float()
    scale = gamma * invstd
    shift = beta - mean * scale
    shift[1] = -64.0                                   # |y * scale| stays far below: the mask of channel 1 is all zero
    out = dict(shape=shape, K=K, k=k, p=p, osh=osh, x=x, y=y, dz=dz, gamma=gamma, mean=mean, invstd=invstd, scale=scale, shift=shift)
    for relu in (0, 2):
        mask = None
        if relu == 2:
            mask = (ref64.d(y) * ref64.d(scale).view(1, -1, 1, 1, 1) + ref64.d(shift).view(1, -1, 1, 1, 1) > 0).double()
            assert 0.2 < float(mask.mean()) < 0.8 and float(mask[:, 1].sum()) == 0
        bn = ref64.bn_bwd_saved(dz, y, gamma, mean, invstd, mask)
        dw = torch.nn.grad.conv3d_weight(ref64.d(x), (K, shape[1]) + tuple(k), bn['dx'], stride=(1, 2, 2), padding=p)
        out[relu] = dict(dw=dw, dgamma=bn['dgamma'], dbeta=bn['dbeta'])
    _INPUTS[key] = out
    return out


def _plan(ops, c, half, splits):
    N, Cin, D, Hh, W = c['shape']
    plan = ops.ConvPlan(N, Cin, D, Hh, W, c['K'], c['k'], (1, 2, 2), c['p'], DEV, act_f16=half)
    plan.tuned = [True, True, True]
    plan.g.tune_wgrad_tile, plan.g.tune_wgrad_splits = 14, splits
    plan.refresh()
    assert plan.kernel(2) == 'stem' and ops.conv_dzf_ok(plan), plan.cfg(2)
    return plan


def _both(ops, c, relu, half, splits, accumulate, partial=False):
    """-> (dW, dgamma, dbeta) of the fused route and of the unfused route, dW pre-filled with 0.5 when accumulating."""
    H = ops.H
    K, osh = c['K'], c['osh']
    N, SP = osh[0], osh[2] * osh[3] * osh[4]
    plan = _plan(ops, c, half, splits)
    x, y, dz = (c[n].to(DEV) for n in ('x', 'y', 'dz'))
    gamma, mean, invstd, scale, shift = (c[n].to(DEV) for n in ('gamma', 'mean', 'invstd', 'scale', 'shift'))
    res = []
    for fused in (True, False):
        dw = torch.full((K, c['shape'][1]) + tuple(c['k']), 0.5 if accumulate else float('nan'), device=DEV)
        dg, db = torch.full((K,), 0.25, device=DEV), torch.full((K,), -0.25, device=DEV)
        if fused:
            consts = ops.bn_bwd_sums(dz, y, gamma, mean, invstd, relu, N, K, SP, dg, db, scale, shift)
            if partial:
                slab = torch.empty(max(int(plan.wgrad_ws), 16), dtype=torch.uint8, device=DEV)
                nsp = C.c_int32(0)
                H.call('gca_conv_wgrad_dzf_partial', plan.gp, ops.aptr(x), ops.aptr(dz), ops.aptr(y), ops.ptr(consts), relu, None,
                       slab.data_ptr(), C.addressof(nsp), ops.stream())
                job = (H.ReduceJob * 1)()
                job[0].slabs, job[0].dw, job[0].n, job[0].splits, job[0].accumulate = slab.data_ptr(), dw.data_ptr(), dw.numel(), nsp.value, accumulate
                blocks = H.lib.gca_reduce_jobs_finalize_host(C.addressof(job), 1)
                assert blocks > 0 and nsp.value == plan.cfg(2)[2]
                jd = torch.frombuffer(bytearray(bytes(job)), dtype=torch.uint8).to(DEV)
                H.call('gca_splitk_reduce_batched', jd.data_ptr(), 1, blocks, ops.stream())
            else:
                ops.conv_wgrad_dzf(plan, x, dz, y, consts, relu, dw, accumulate=bool(accumulate))
        else:
            dy = ops.bn_bwd(dz, None, y, gamma, mean, invstd, relu, N, K, SP, dg, db, scale=scale, shift=shift)
            ops.conv_wgrad(plan, x, dy, dw, accumulate=bool(accumulate))
        torch.cuda.synchronize()
        res.append((dw - 0.5 if accumulate else dw, dg - 0.25, db + 0.25, dg, db))
    return res


@pytest.mark.parametrize('relu', [0, 2])
@pytest.mark.parametrize('sid,mode', CASES)
def test_fused_stem_backward_vs_fp64_and_unfused(ops, sid, mode, relu):
    """Every split count from one workgroup per tap-plane group to one per 8-row chunk (the last chunk: one row), += and =,
    the _partial form with the batched reduction; dgamma / dbeta bit-equal to the unfused path, dW within the bar of its
    arithmetic and within 1.5 x the unfused error."""
    half = mode == 'fp16'
    c = _inputs(sid, False, half)
    units = c['osh'][0] * c['osh'][2]
    default = ops.get_conv_math()
    try:
        ops.set_conv_math(mode)
        ref = c[relu]
        for splits, accumulate, partial in ((1, 0, False), (2, 1, False), (units, 1, True), (4 * units, 0, False), (4 * units, 1, True)):
            (fw, fg, fb, fg_raw, fb_raw), (uw, ug, ub, ug_raw, ub_raw) = _both(ops, c, relu, half, splits, accumulate, partial)
            ef, eu = rel_err(fw, ref['dw']), rel_err(uw, ref['dw'])
            eg, eb = rel_err(fg, ref['dgamma']), rel_err(fb, ref['dbeta'])
            print('%s %s relu=%d splits=%d acc=%d partial=%d: dW err fused %.3e unfused %.3e, dgamma %.3e dbeta %.3e'
                  % (sid, mode, relu, splits, accumulate, partial, ef, eu, eg, eb))
            assert torch.equal(fg_raw, ug_raw) and torch.equal(fb_raw, ub_raw)
            assert eg < 1e-5 and eb < 1e-5
            assert ef < BARS[mode], (ef, eu)
            assert ef <= 1.5 * eu, (ef, eu)
            assert float(fw[1].abs().max()) == 0.0 or relu == 0            # the all-masked channel: dy = A * (0 - 0 - xhat * 0)
    finally:
        ops.set_conv_math(default)


@pytest.mark.parametrize('relu', [0, 2])
@pytest.mark.parametrize('sid,mode', CASES)
def test_fused_stem_backward_bit_equal_on_dyadic_operands(ops, sid, mode, relu):
    """Dyadic dz, y, x, mean, invstd, gamma: every BatchNorm sum is exact, so both routes hold the same B = S1 / M and Cc = S2 / M
    and the fused kernel must feed the MFMAs the bits the unfused path stored: dW, dgamma, dbeta identical."""
    half = mode == 'fp16'
    c = _inputs(sid, True, half)
    units = c['osh'][0] * c['osh'][2]
    M = c['osh'][0] * c['osh'][2] * c['osh'][3] * c['osh'][4]
    assert exact.exact_in_fp32(M * 2.0 * 8.0, 1 / 32) < 1           # sum |dz * xhat| <= M * 2 * (2 + 0.5) * 2 in units of 1/32
    default = ops.get_conv_math()
    try:
        ops.set_conv_math(mode)
        for splits, accumulate, partial in ((1, 0, False), (units, 1, False), (4 * units, 1, True)):
            (fw, fg, fb, _, _), (uw, ug, ub, _, _) = _both(ops, c, relu, half, splits, accumulate, partial)
            assert torch.equal(fg, ug) and torch.equal(fb, ub)
            assert torch.equal(fg.double().cpu(), c[relu]['dgamma']) and torch.equal(fb.double().cpu(), c[relu]['dbeta'])
            assert torch.equal(fw, uw), (splits, accumulate, partial, float((fw - uw).abs().max()))
            assert rel_err(fw, c[relu]['dw']) < BARS[mode]
    finally:
        ops.set_conv_math(default)


def test_layer_takes_the_fused_route(pkg, ops, monkeypatch):
    """f_conv_bn_act on a first-layer unit at N = 2, T = 4, 144 x 144 (N * SP = 41472 > 32768) with the stem kernel pinned:
    with STEM_DZF (what GCA_STEM_DZF sets) the backward runs bn_bwd_sums + conv_wgrad_dzf and never bn_bwd; without it the
    reverse; the BatchNorm gradients come from the same kernels (bit-equal), the weight gradient agrees within the bf16x6 bar."""
    layers, tape = pkg.engine.layers, pkg.engine.tape
    default = ops.get_conv_math()
    ops.set_conv_math('bf16x6')
    try:
        torch.manual_seed(7)
        conv, bn = layers.HipConv3d(3, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3)).to(DEV), layers.HipBatchNorm3d(64).to(DEV)
        x = torch.randn(2, 3, 4, 144, 144, device=DEV)
        dz = torch.randn(2, 64, 4, 72, 72, device=DEV)
        plan = conv.plan(x)
        plan.tuned = [True, True, True]
        plan.g.tune_wgrad_tile, plan.g.tune_wgrad_splits = 14, 0
        plan.refresh()
        assert plan.kernel(2) == 'stem'
        calls = []
        for name in ('bn_bwd', 'bn_bwd_sums', 'conv_wgrad', 'conv_wgrad_dzf'):
            real = getattr(ops, name)
            monkeypatch.setattr(ops, name, (lambda real, name: lambda *a, **k: (calls.append(name), real(*a, **k))[1])(real, name))
        grads = {}
        for arm in (False, True):
            monkeypatch.setattr(ops, 'STEM_DZF', arm)
            for prm in (conv.weight, bn.weight, bn.bias):
                prm.grad = None
            bn.running_mean.zero_(); bn.running_var.fill_(1.0)
            del calls[:]
            tp = tape.Tape(True)
            zv = layers.f_conv_bn_act(tp, conv, bn, tape.Var(x, False))
            zv.grad = dz.clone()
            tp.backward()
            torch.cuda.synchronize()
            assert calls == (['bn_bwd_sums', 'conv_wgrad_dzf'] if arm else ['bn_bwd', 'conv_wgrad']), (arm, calls)
            grads[arm] = [prm.grad.clone() for prm in (conv.weight, bn.weight, bn.bias)]
        assert torch.equal(grads[True][1], grads[False][1]) and torch.equal(grads[True][2], grads[False][2])
        err = rel_err(grads[True][0], grads[False][0])
        print('layer: dW fused vs unfused %.3e' % err)
        assert err < BARS['bf16x6']
    finally:
        ops.set_conv_math(default)
        plan.g.tune_wgrad_tile = 0
        plan.refresh()
