"""The conv, BatchNorm and pool kernels on ONE tensor of 2 to 4 GiB (tests/large_cases.py; every precondition is asserted on the
CPU by tests/test_large_cases.py): byte offsets at and above 2^31 through every kernel family, up to the last bytes a buffer
resource can address.

Every comparison is equality.  Periodic content: every output clip equals output clip n mod 7 (compared on the device over the
whole tensor) and the first 7 equal the fp64 reference.  Sparse content: zero except in clip 0, the clip holding byte 2^31, one
beyond it and the last -- or the two beyond 2^31 alone -- so that every reduction over the batch has an fp64 reference over
those clips.  Outputs are pre-filled with NaN: a dropped store cannot pass.

Band H (fp32 tensors of more than 2^30 - 1024 elements: below the element limit, their tail beyond the last addressable byte):
an entry must refuse -- ValueError from the plan, GCA_EINVAL from the C entry, outputs untouched -- or be exact.

Each test prints one row: case, family, pass, elements of the large tensor, peak device memory, seconds."""
import ctypes as C
import gc
import time

import pytest
import torch

import exact
import large_cases as lc
from large_cases import PERIOD

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F16, F32 = torch.float16, torch.float32
EINVAL = -1
NAN = float('nan')
NEED_GIB = 14               # the large tensor, a second one of its size (slabs, a gradient, a residual), the partner, compare scratch


def _id(c):
    return c.id


@pytest.fixture(scope='module')
def ops(pkg):
    return pkg.engine.ops


@pytest.fixture
def row(ops, request):
    """Default arithmetic and merged dgrads for the test; afterwards the scratch lane (a split-K forward leaves 8 GiB there) and
    the allocator's cache are released, and the test's row is printed."""
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_GIB * 2 ** 30:
        pytest.skip('%.1f GiB of device memory free, the case needs %d GiB' % (free / 2 ** 30, NEED_GIB))
    math, merge = ops.get_conv_math(), ops.set_dgrad_merge(True)
    ops.set_conv_math('bf16x6')
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    info = {}
    t0 = time.perf_counter()
    yield info
    torch.cuda.synchronize()
    dt, peak = time.perf_counter() - t0, torch.cuda.max_memory_allocated() / 2 ** 30
    ops.set_conv_math(math)
    ops.set_dgrad_merge(merge)
    ops.WS.buf.clear()
    gc.collect()
    torch.cuda.empty_cache()
    print('LARGE-GPU | %s | %s | %s | %d | %.2f GiB | %.2f s' % (request.node.name, info.get('family', '-'), info.get('pas', '-'),
                                                               info.get('elems', 0), peak, dt))


def dev(t, half=False):
    return None if t is None else (t.to(DEV).half() if half else t.float().to(DEV))


def eq(got, want, half=False):
    """The device tensor holds exactly the fp64 values `want` (fp16 storage: their round-to-nearest-even cast)."""
    if half:
        return got.dtype is F16 and torch.equal(got.cpu(), exact.to_f16(want))
    return got.dtype is not F16 and torch.equal(got.cpu().double(), want.double())


def stat(ss):
    return ss.double().sum(1).cpu()


def _plan(ops, c, info):
    plan = lc.plan_for(ops, c, DEV)
    got, want = lc.resolved(plan, c)
    assert got == want, (c.id, got)
    info.update(family='%s%s' % (c.family, '+' + c.extra if c.extra else ''), pas=c.pas, elems=lc.large_elems(c))
    return plan


def _xf_rows(o, C_):
    """(scale, shift) as bn_finalize hands them over: rows padded to a multiple of 16 + 16 floats."""
    Cp = -(-C_ // 16) * 16 + 16
    sc, sf = torch.zeros(Cp, device=DEV), torch.zeros(Cp, device=DEV)
    sc[:C_], sf[:C_] = dev(o['scale']), dev(o['shift'])
    return sc[:C_], sf[:C_]


def _forward(ops, plan, c, x, wpack, y, xf=None):
    """The forward of the case into the caller's (NaN-filled) y, BatchNorm sums included.  -> (sum y, sum y^2) per channel."""
    H = ops.H
    ss, sq = ops._stat_pair(plan, DEV)
    if xf is not None:
        ws = ops.WS.get(plan.fwd_ws, DEV) if plan.fwd_ws else None
        H.call('gca_conv_fwd_xf', plan.gp, H.ptr(x), H.ptr(xf[0]), H.ptr(xf[1]), H.ptr(wpack), H.ptr(plan.table(0)), None, H.ptr(y),
               H.ptr(ss), H.ptr(sq), H.ptr(ws), H.stream())
    else:
        ops._conv_fwd_launch(plan, x, wpack, None, y, ss, sq)
    return stat(ss), stat(sq)


def _forward_case(ops, c, info, variants=('all', 'beyond')):
    plan = _plan(ops, c, info)
    o = lc.periodic(c.id)
    wpack = ops.conv_pack(plan, 0, dev(o['w']))
    xf = _xf_rows(o, c.clip[0]) if c.extra == 'xf' else None
    dt = F16 if c.half else F32
    # periodic content: y, clip by clip
    x = lc.tile(dev(o['x'], c.half), c.N)
    y = torch.full(plan.out_shape, NAN, dtype=dt, device=DEV)
    _forward(ops, plan, c, x, wpack, y, xf)
    del x
    assert eq(y[:PERIOD], o['ref']['y'], c.half), 'the first clips'
    assert lc.is_periodic(y), lc.mismatch(y)
    # sparse content: the BatchNorm sums of the epilogue (of the split-K finish), and zeros everywhere else
    for variant in variants:
        s = lc.sparse(c.id, variant)
        x = lc.scatter(dev(s['x'], c.half), s['ids'], c.N, s.get('fill', 0.0))
        y.fill_(NAN)
        sy, sq = _forward(ops, plan, c, x, wpack, y, xf)
        del x
        assert eq(y[torch.as_tensor(s['ids'], device=DEV)], s['ref']['y'], c.half), variant
        assert lc.only_in(y, s['ids']), variant
        assert torch.equal(sy, s['ref']['sy']) and bool(sy.any()), ('sum y', variant)
        if c.set == 'NARROW':
            assert torch.equal(sq, s['ref']['sq']) and bool(sq.any()), ('sum y^2', variant)


@pytest.mark.parametrize('c', [c for c in lc.CONV_CASES if c.pas == 'fwd'], ids=_id)
def test_forward_on_a_large_tensor(ops, row, c):
    _forward_case(ops, c, row)


def _dgrad_case(ops, c, info):
    plan = _plan(ops, c, info)
    o = lc.periodic(c.id)
    if c.extra == 'merged':
        assert ops.H.lib.gca_conv_dgrad_merged(plan.gp, C.c_int64(max(plan.dgrad_ws, plan.dgrad_ws_merged))) == 1
    wt = ops.conv_pack(plan, 1, dev(o['w']))
    dy = lc.tile(dev(o['dy'], c.half), c.N)
    dx = torch.full(plan.in_shape, NAN, dtype=F16 if c.half else F32, device=DEV)
    ops.conv_dgrad(plan, dy, wt, dx, accumulate=False)
    del dy
    assert eq(dx[:PERIOD], o['ref']['dx'], c.half), 'the first clips'
    assert lc.is_periodic(dx), lc.mismatch(dx)


@pytest.mark.parametrize('c', [c for c in lc.CONV_CASES if c.pas == 'dgrad'], ids=_id)
def test_dgrad_on_a_large_tensor(ops, row, c):
    _dgrad_case(ops, c, row)


def _wgrad_case(ops, c, info, variants=('all', 'beyond')):
    plan = _plan(ops, c, info)
    v = lambda t: dev(t)
    for variant in variants:
        s = lc.sparse(c.id, variant)
        x = lc.scatter(dev(s['x'], c.half), s['ids'], c.N)
        accumulate = variant == 'all'
        dw = torch.full(tuple(s['w'].shape), 0.5 if accumulate else NAN, device=DEV)
        want = s['ref']['dw'] + (0.5 if accumulate else 0.0)
        if c.extra == 'dzf':
            assert ops.conv_dzf_ok(plan)
            K, SP = c.K, lc.prod(lc.out_clip(c)[1:])
            dz, yb = lc.scatter(dev(s['dz']), s['ids'], c.N), lc.scatter(dev(s['y']), s['ids'], c.N)
            dg, db = torch.full((K,), 0.25, device=DEV), torch.full((K,), -0.25, device=DEV)
            consts = ops.bn_bwd_sums(dz, yb, v(s['gamma']), v(s['mean']), v(s['invstd']), 2, c.N, K, SP, dg, db, v(s['scale']), v(s['shift']))
            Cp = consts.numel() // 7
            assert not bool(consts[Cp:3 * Cp].any()), 'B = S1 / M and Cc = S2 / M of cancelling sums'
            assert bool((dg == 0.25).all()) and bool((db == -0.25).all())
            ops.conv_wgrad_dzf(plan, x, dz, yb, consts, 2, dw, accumulate=accumulate)
            del dz, yb
        else:
            dy = lc.scatter(dev(s['dy'], c.half), s['ids'], c.N)
            ops.conv_wgrad(plan, x, dy, dw, accumulate=accumulate)
            del dy
        del x
        assert eq(dw, want), (variant, plan.cfg(2), 'max |dw - exact| = %g' % float((dw.cpu().double() - want).abs().max()))


@pytest.mark.parametrize('c', lc.WGRAD_CASES, ids=_id)
def test_weight_gradient_on_a_large_tensor(ops, row, c):
    _wgrad_case(ops, c, row)


# ============================================================================= band H
@pytest.mark.parametrize('c', lc.H_CASES, ids=_id)
def test_band_h_is_refused_or_exact(ops, row, c):
    """2^30 - 512 fp32 elements: the last clip lies wholly beyond 0xfffff000.  Before geom_ok refused such a tensor the entries
    returned status 0 with the last clip read as zeros (a large source: y of that clip all zero, dw without its term) or never
    written (a large destination: the NaN pre-fill still there)."""
    H = ops.H
    try:
        lc.plan_for(ops, c, DEV)
        refused = False
    except ValueError:
        refused = True
    if not refused:
        # accepted: then the answer must be exact, the last clip included
        if c.pas == 'fwd':
            _forward_case(ops, c, row, variants=('all',))
        else:
            _wgrad_case(ops, c, row, variants=('all',))
        return
    row.update(family='refused', pas=c.pas, elems=lc.large_elems(c))
    with pytest.raises(ValueError):
        ops.conv_plan((c.N,) + c.clip, c.K, c.k, c.s, c.p, DEV)
    # the C entry: real operands of the case's sizes, zeroed stand-ins for the packed weights and the table (no size query
    # answers for a refused geometry; 1 MiB is far above what either needs)
    out = lc.out_clip(c)
    g = H.ConvGeom(c.N, *c.clip, c.K, *c.k, *c.s, *c.p, *out[1:], 0)
    for field, val in c.tune.items():
        setattr(g, 'tune_' + field, val)
    gp = C.byref(g)
    blob = torch.zeros(1 << 18, dtype=F32, device=DEV)
    table = torch.zeros(1 << 18, dtype=torch.int32, device=DEV)
    x = torch.zeros((c.N,) + c.clip, device=DEV)
    if c.pas == 'fwd':
        y = torch.full((c.N,) + out, NAN, device=DEV)
        rc = H.lib.gca_conv_fwd(gp, H.ptr(x), H.ptr(blob), H.ptr(table), None, H.ptr(y), None, None, None, H.stream())
        torch.cuda.synchronize()
        assert rc == EINVAL and bool(y.isnan().all())
        rc = H.lib.gca_conv_dgrad_ws(gp, H.ptr(y), H.ptr(blob), H.ptr(table), H.ptr(x), 0, None, C.c_int64(0), H.stream())
        torch.cuda.synchronize()
        assert rc == EINVAL and not bool(x.any())
    else:
        dy = torch.zeros((c.N,) + out, device=DEV)
        dw = torch.full((c.K, c.clip[0]) + tuple(c.k), NAN, device=DEV)
        rc = H.lib.gca_conv_wgrad(gp, H.ptr(x), H.ptr(dy), H.ptr(table), H.ptr(dw), 0, H.ptr(blob), H.stream())
        torch.cuda.synchronize()
        assert rc == EINVAL and bool(dw.isnan().all())


# ============================================================================= BatchNorm
@pytest.mark.parametrize('c', lc.BN_CASES, ids=_id)
def test_batchnorm_on_a_large_tensor(ops, row, c):
    """bn_stats (sparse), bn_apply with residual and ReLU (periodic), bn_bwd on its three-pass path (periodic dx on cancelling
    sums, then dgamma / dbeta from the sparse content, by bn_bwd and by bn_bwd_sums): float4 and scalar forms."""
    o = lc.bn_operands(c.id)
    N, Cc, SP = c.N, c.C, lc.prod(c.sp)
    row.update(family='bn_%s VEC %d' % (c.op, c.vec), pas=c.op, elems=lc.large_elems(c))
    gam, mean, invstd, scale, shift = (dev(o[n]) for n in ('gamma', 'mean', 'invstd', 'scale', 'shift'))
    if c.op == 'stats':
        for variant in ('all', 'beyond'):
            ids = lc.named_clips(c, variant)
            xs = o['xs'][-len(ids):]
            x = lc.scatter(dev(xs), ids, N)
            ss, sq = ops.bn_stats(x, N, Cc, SP)
            del x
            assert torch.equal(stat(ss), xs.sum((0, 2, 3, 4))) and torch.equal(stat(sq), (xs ** 2).sum((0, 2, 3, 4))) and bool(stat(sq).all())
    elif c.op == 'apply':
        x, res = lc.tile(dev(o['x']), N), lc.tile(dev(o['res']), N)
        z = torch.full_like(x, NAN)
        ops.bn_apply(x, scale, shift, res, True, N, Cc, SP, out=z)
        del x, res
        assert eq(z[:PERIOD], o['z'])
        assert lc.is_periodic(z), lc.mismatch(z)
    else:
        whole = N // PERIOD * PERIOD
        dz, x = lc.tile(dev(o['dz']), N), lc.tile(dev(o['x']), N)
        dz[whole:] = 0                                               # the clips past the last whole period: the sums stay zero
        dg, db = torch.full((Cc,), 0.25, device=DEV), torch.full((Cc,), -0.25, device=DEV)
        dx = ops.bn_bwd(dz, None, x, gam, mean, invstd, 2, N, Cc, SP, dg, db, None, False, scale, shift)
        del dz, x
        assert bool((dg == 0.25).all()) and bool((db == -0.25).all())
        assert eq(dx[:PERIOD], o['dx']) and not bool(dx[whole:].any())
        assert lc.is_periodic(dx[:whole]), lc.mismatch(dx[:whole])
        del dx
        for variant in ('all', 'beyond'):
            ids = lc.named_clips(c, variant)
            k = len(ids)
            xs, dzs, ms, xhat = (o[n][-k:] for n in ('xs', 'dzs', 'ms', 'xhat'))
            x, dz = lc.scatter(dev(xs), ids, N), lc.scatter(dev(dzs), ids, N)
            dg, db = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
            if variant == 'all':
                ops.bn_bwd(dz, None, x, gam, mean, invstd, 2, N, Cc, SP, dg, db, None, False, scale, shift)
            else:
                ops.bn_bwd_sums(dz, x, gam, mean, invstd, 2, N, Cc, SP, dg, db, scale, shift)
            del x, dz
            assert eq(db, (ms * dzs).sum((0, 2, 3, 4))) and eq(dg, (ms * dzs * xhat).sum((0, 2, 3, 4))) and bool(dg.any()), variant


def test_bias_grad_on_a_large_tensor(ops, row):
    """gca_bias_grad over a (N, K, SP) gradient of 2^30 - 2048 elements, sparse content, += onto 0.25."""
    c = lc.BN_CASES[0]
    o = lc.bn_operands(c.id)
    N, K, SP = c.N, c.C, lc.prod(c.sp)
    row.update(family='bias_grad', pas='bias_grad', elems=lc.large_elems(c))
    for variant in ('all', 'beyond'):
        ids = lc.named_clips(c, variant)
        dzs = o['dzs'][-len(ids):]
        dy = lc.scatter(dev(dzs), ids, N)
        db = torch.full((K,), 0.25, device=DEV)
        ops.bias_grad(dy, N, K, SP, db, True)
        del dy
        assert eq(db, dzs.sum((0, 2, 3, 4)) + 0.25) and bool((db != 0.25).any()), variant


# ============================================================================= pools
@pytest.mark.parametrize('c', lc.POOL_CASES, ids=_id)
def test_pool_on_a_large_tensor(ops, row, c):
    """Forward (y, argmax) on a large input and backward into a large dx: the paired / brick 3x3x3 stride-2 kernels, an unrolled
    generic pair, the run-time-window pair, and the average pool -- against ATen in double."""
    o = lc.pool_operands(c.id)
    row.update(family=c.id, pas='fwd+bwd', elems=lc.large_elems(c))
    plan = ops.pool_plan((c.N,) + c.clip, c.k, c.s, c.p)
    assert tuple(plan.out_shape[1:]) == tuple(o['y'].shape[1:])
    x = lc.tile(dev(o['x']), c.N)
    dx = torch.full(plan.in_shape, NAN, device=DEV)
    dy = lc.tile(dev(o['dy']), c.N)
    if c.kind == 'max':
        y, am = ops.maxpool_fwd(plan, x)
        del x
        assert eq(y[:PERIOD], o['y']) and torch.equal(am[:PERIOD].cpu().long(), o['argmax'])
        assert lc.is_periodic(y), lc.mismatch(y)
        assert lc.is_periodic(am), lc.mismatch(am)
        ops.maxpool_bwd(plan, dy, am, dx, False)
    else:
        y = ops.avgpool_fwd(plan, x)
        del x
        assert eq(y[:PERIOD], o['y'])
        assert lc.is_periodic(y), lc.mismatch(y)
        ops.avgpool_bwd(plan, dy, dx, False)
    assert eq(dx[:PERIOD], o['dx'])
    assert lc.is_periodic(dx), lc.mismatch(dx)
