"""CPU checks of tests/large_cases.py, the cases tests/test_gpu_large.py runs on tensors of 2 to 4 GiB: every case's large tensor
sits in the band it claims, the clip holding byte offset 2^31 is the one the sparse content names, every sum a case compares
stays inside the fp32 integer range (exact.exact_in_fp32 < 1: the fp64 reference IS the answer), the reference is not zero in
the clips beyond 2^31, and under its pinned launch codes every case resolves to the kernel family it names (plans on
torch.device('cpu'): host logic only).  Band H -- fp32 tensors below 2^30 elements whose tail lies beyond the last byte a
buffer resource can address -- must be refused by the plan and by the C entries' geometry check."""
import ctypes as C

import pytest
import torch

import exact
import large_cases as lc

CPU = torch.device('cpu')
EINVAL = -1


@pytest.fixture
def ops(pkg):
    """The default arithmetic (bf16x6: the stem and streaming kernels exist for the bf16 modes only), restored afterwards."""
    H = pkg._hip
    prev = H.lib.gca_get_conv_math()
    H.lib.gca_set_conv_math(2)
    yield pkg.engine.ops
    H.lib.gca_set_conv_math(prev)


def _ids(c):
    return c.id


def test_case_ids_are_unique_and_cover_the_issue():
    allc = lc.CONV_CASES + lc.WGRAD_CASES + lc.H_CASES
    assert len({c.id for c in allc}) == len(allc) == len(lc.ALL_CONV)
    have = {(c.family, c.pas, c.big) for c in lc.CONV_CASES if not c.extra and c.band == 'T'}
    assert sum(c.family == 'vec' and c.k == (1, 1, 1) for c in lc.CONV_CASES) == 4            # the pointwise conv on fp32 tensors
    for fam in ('gather', 'vec', 'halo'):                       # large source and large destination, forward and dgrad
        assert {(fam, 'fwd', 'x'), (fam, 'fwd', 'y'), (fam, 'dgrad', 'dy'), (fam, 'dgrad', 'dx')} <= have
    # the pointwise GEMM kernel exists for fp16 storage only: its four cases are band T16, next to one fp16 gather case
    t16 = {(c.family, c.pas, c.big) for c in lc.CONV_CASES if c.band == 'T16'}
    assert {('pw', 'fwd', 'x'), ('pw', 'fwd', 'y'), ('pw', 'dgrad', 'dy'), ('pw', 'dgrad', 'dx'), ('gather', 'fwd', 'x')} == t16
    assert {c.extra for c in lc.CONV_CASES} == {'', 'xf', 'merged', 'splitk'} and ('stem', 'fwd', 'x') in have
    assert {(c.family, c.extra, c.big) for c in lc.WGRAD_CASES} == {(f, e, b) for f, e in (('gather', ''), ('temporal32', ''), ('spatial', ''),
                                                                                           ('stem', ''), ('stem', 'dzf')) for b in ('x', 'dy')}
    assert {(c.op, c.vec) for c in lc.BN_CASES} == {(op, v) for op in ('stats', 'apply', 'bwd') for v in (4, 1)}
    assert all((lc.prod(c.sp) % 4 == 0) == (c.vec == 4) for c in lc.BN_CASES)
    assert [(c.pas, c.big) for c in lc.H_CASES] == [('fwd', 'x'), ('fwd', 'y'), ('wgrad', 'x')]


@pytest.mark.parametrize('c', lc.CONV_CASES + lc.WGRAD_CASES + lc.H_CASES + lc.BN_CASES + lc.POOL_CASES, ids=_ids)
def test_large_tensor_sits_in_its_band(c):
    """Element count and byte size of the large tensor; the partner tensors are small; which clip holds byte 2^31."""
    n, es = lc.large_elems(c), lc.elem_size(c)
    band = getattr(c, 'band', 'T')
    lo, hi = lc.BANDS[band]
    assert lo <= n <= hi, (n, band)
    ids = lc.named_clips(c)
    ce = lc.clip_elems(c) * es
    if band == 'T16':
        assert 2 ** 31 - 2 ** 17 <= n * es < 2 ** 31
    else:
        at = lc.clip_at_byte(c, 2 ** 31)
        assert n * es > 2 ** 31 and ids[1] == at and at * ce <= 2 ** 31 < (at + 1) * ce
        assert ids[2] * ce > 2 ** 31 and ids[3] == c.N - 1                    # wholly beyond, and the last clip
        assert (n * es <= lc.BUF_MAX_BYTES) == (band == 'T')
        assert n * es > lc.BUF_MAX_BYTES - 2 ** 18                            # ends within 256 KiB of the clamp
        if band == 'H':                                                       # the last clip starts at or past the clamp
            assert (c.N - 1) * ce >= lc.BUF_MAX_BYTES
    assert len(set(ids)) == 4 and ids == sorted(ids) and lc.named_clips(c, 'beyond') == ids[2:]
    assert c.N // lc.PERIOD >= 2 and (c.N % lc.PERIOD != 0 or band == 'H')    # whole periods and a remainder (2^21 - 1 = 7 * 299593)
    assert all(2 ** j % lc.PERIOD for j in range(40))                         # no power-of-two wrap keeps the phase
    if isinstance(c, lc.Conv):
        small = c.N * lc.prod(c.clip if c.big in ('y', 'dy') else lc.out_clip(c))
        assert small * 2 <= n                                                 # exactly one tensor is large
    print('LARGE %-22s band %-3s elements 2^30 - %-6d bytes %d clip of byte 2^31: %d of %d'
          % (c.id, band, 2 ** 30 - n, n * es, lc.clip_at_byte(c, 2 ** 31), c.N))


@pytest.mark.parametrize('c', lc.CONV_CASES + lc.WGRAD_CASES, ids=_ids)
def test_case_resolves_to_the_kernel_family_it_names(ops, c):
    plan = lc.plan_for(ops, c, CPU)
    got, want = lc.resolved(plan, c)
    assert got == want, (c.id, plan.cfg({'fwd': 0, 'dgrad': 1, 'wgrad': 2}[c.pas]))
    which = {'fwd': 0, 'dgrad': 1, 'wgrad': 2}[c.pas]
    if c.extra == 'splitk':
        assert plan.cfg(0)[2] == 2 and plan.fwd_ws == 2 * 4 * lc.large_elems(c)                 # two slabs of the output's size
    elif which < 2:
        assert plan.cfg(which)[2] == 1
    if c.extra == 'merged':
        assert ops.H.lib.gca_conv_dgrad_merged(plan.gp, C.c_int64(0)) == 1 and plan.cfg(1)[3] & 255 == 4      # four stride classes, one launch
    if c.extra == 'xf':
        assert plan.math(0) in (1, 2)
    if c.extra == 'dzf':
        assert ops.conv_dzf_ok(plan)
    if c.half:
        assert plan.cfg(which)[3] >> 15 & 1
    print('LARGE %-22s resolves to %s, launch %s' % (c.id, got, plan.cfg(which)))


@pytest.mark.parametrize('c', lc.CONV_CASES, ids=_ids)
def test_periodic_content_is_exact_and_differs_from_clip_to_clip(c):
    o = lc.periodic(c.id)
    what = ('y',) if c.pas == 'fwd' else ('dx',)
    b = lc.budgets(c, o, what)
    assert max(b.values()) < 1, b
    r = o['ref'][what[0]]
    assert all(bool(r[i].any()) for i in range(lc.PERIOD))                                 # non-zero in every phase: beyond 2^31 too
    assert all(not torch.equal(r[i], r[j]) for i in range(lc.PERIOD) for j in range(i))    # a clip of another phase is another answer
    if c.half:
        assert torch.equal(o['x'].half().double(), o['x']) and torch.equal(o['dy'].half().double(), o['dy'])
    print('LARGE %-22s periodic budget %s' % (c.id, {k: '%.2e' % v for k, v in b.items()}))


@pytest.mark.parametrize('variant', ['all', 'beyond'])
@pytest.mark.parametrize('c', [c for c in lc.CONV_CASES if c.pas == 'fwd'] + lc.WGRAD_CASES, ids=_ids)
def test_sparse_content_is_exact_and_not_zero_beyond_2_31(c, variant):
    o = lc.sparse(c.id, variant)
    what = ('dw',) if c.pas == 'wgrad' else (('y', 'sy', 'sq') if c.set == 'NARROW' else ('y', 'sy'))
    b = lc.budgets(c, o, what)
    assert max(b.values()) < 1, b
    beyond = lc.sparse(c.id, 'beyond')
    for n in what:
        assert bool(beyond['ref'][n].any()), n                     # the clips beyond 2^31 alone give an answer that is not zero
    if c.pas == 'wgrad':
        assert float((beyond['ref']['dw'] != 0).double().mean()) > 0.5
        assert not torch.equal(beyond['ref']['dw'], lc.sparse(c.id, 'all')['ref']['dw'])
    if c.extra == 'dzf':
        # the BatchNorm sums of the paired clips cancel: S1 = sum m dz = 0, S2 = sum m dz xhat = 0 per channel, so B = Cc = 0
        v = lambda t: t.view(1, -1, 1, 1, 1)
        xhat = (o['y'] - v(o['mean'])) * v(o['invstd'])
        md = o['mask'] * o['dz']
        assert float(md.sum((0, 2, 3, 4)).abs().max()) == 0 and float((md * xhat).sum((0, 2, 3, 4)).abs().max()) == 0
        assert 0.2 < float(o['mask'].mean()) < 0.8 and bool(o['dy_eff'].any())
        assert exact.exact_in_fp32(md.abs().sum((0, 2, 3, 4)), 1 / 4) < 1 and exact.exact_in_fp32((md * xhat).abs().sum((0, 2, 3, 4)), 1 / 32) < 1
    if c.extra == 'xf':
        v = lambda t: t.view(1, -1, 1, 1, 1)
        assert float(torch.relu(o['fill'] * v(o['scale']) + v(o['shift'])).abs().max()) == 0      # the filler is neutral
    print('LARGE %-22s sparse(%s) clips %s budget %s' % (c.id, variant, o['ids'], {k: '%.2e' % v for k, v in b.items()}))


@pytest.mark.parametrize('c', lc.BN_CASES, ids=_ids)
def test_batchnorm_content_is_exact(c):
    o = lc.bn_operands(c.id)
    v = lambda t: t.view(1, -1, 1, 1, 1)
    # bn_apply: x * scale + shift + res in units of 1/16, below 2^24 of them by far; every step exact in fp32
    lin = (o['x'] * v(o['scale'])).abs() + v(o['shift']).abs() + o['res'].abs()
    assert exact.exact_in_fp32(lin, 1 / 16) < 1 and bool((o['z'] > 0).any()) and bool((o['z'] == 0).any())
    # bn_bwd: the sums of one period cancel exactly, per channel; any run of consecutive elements sums to less than one
    # period's absolute sum (what a part of the reduction holds before it is rounded to fp32)
    mask = (o['x'] * v(o['scale']) + v(o['shift']) > 0).double()
    md = mask * o['dz']
    xhat = (o['x'] - v(o['mean'])) * v(o['invstd'])
    assert float(md.sum((0, 2, 3, 4)).abs().max()) == 0 and float((md * xhat).sum((0, 2, 3, 4)).abs().max()) == 0
    assert exact.exact_in_fp32(md.abs().sum((0, 2, 3, 4)), 1 / 4) < 1 and exact.exact_in_fp32((md * xhat).abs().sum((0, 2, 3, 4)), 1 / 32) < 1
    assert all(bool(o['dx'][i].any()) for i in range(6)) and exact.exact_in_fp32(o['dx'], 1 / 16) < 1
    # sums over the named clips: bn_stats (sum x, sum x^2), dbeta = sum m dz, dgamma = sum m dz xhat
    for t, unit in ((o['xs'], 1 / 4), (o['xs'] ** 2, 1 / 16), (o['ms'] * o['dzs'], 1 / 4), (o['ms'] * o['dzs'] * o['xhat'], 1 / 32)):
        assert exact.exact_in_fp32(t.abs().sum((0, 2, 3, 4)), unit) < 1
        assert bool(t[2:].sum((0, 2, 3, 4)).any())                   # not zero from the clips beyond 2^31 alone
    assert 0.2 < float(o['ms'].mean()) < 0.8


@pytest.mark.parametrize('c', lc.POOL_CASES, ids=_ids)
def test_pool_content_has_no_ties_and_is_exact(c):
    o = lc.pool_operands(c.id)
    assert o['x'].unique().numel() == o['x'].numel() and torch.equal(o['x'].float().double(), o['x'])
    assert torch.equal(o['y'].float().double(), o['y']) and torch.equal(o['dx'].float().double(), o['dx'])
    assert all(not torch.equal(o['y'][i], o['y'][j]) for i in range(lc.PERIOD) for j in range(i))
    out = c.N * lc.prod(o['y'].shape[1:])
    assert out < 2 ** 31 and lc.large_elems(c) < 2 ** 31                 # the 32-bit regime of the pool kernels
    if c.kind == 'max':
        assert int(o['argmax'].max()) < lc.prod(c.clip[1:]) and bool((o['dx'] == 0).any()) and bool(o['dx'].any())


@pytest.mark.parametrize('c', lc.H_CASES, ids=_ids)
def test_band_h_is_refused_by_the_plan_and_the_geometry_check(ops, c):
    """A tensor in (2^30 - 1024, 2^30) elements passes the element limit but its last bytes lie outside every buffer range:
    loads there would return 0 and stores would be dropped.  The plan and every size query refuse it; one clip fewer (band T's
    upper edge and below) is accepted."""
    H = ops.H
    with pytest.raises(ValueError):
        lc.plan_for(ops, c, CPU)
    with pytest.raises(ValueError):
        ops.conv_plan((c.N,) + c.clip, c.K, c.k, c.s, c.p, CPU)
    OD, OH, OW = lc.out_clip(c)[1:]
    g = H.ConvGeom(c.N, *c.clip, c.K, *c.k, *c.s, *c.p, OD, OH, OW, 0)
    gp = C.byref(g)
    for fn in ('gca_conv_fwd_stat_parts', 'gca_conv_fwd_ws_bytes', 'gca_conv_dgrad_ws_bytes', 'gca_conv_wgrad_ws_bytes'):
        assert getattr(H.lib, fn)(gp) == EINVAL, fn
    assert H.lib.gca_conv_pack_elems(gp, 0) == EINVAL and H.lib.gca_conv_table_rows(gp, 0) == EINVAL
    g.N = c.N - 1                                               # 2^30 - 1024 elements = BUF_MAX_BYTES bytes exactly: the largest accepted
    assert lc.large_elems(c._replace(N=c.N - 1)) * 4 == lc.BUF_MAX_BYTES
    assert H.lib.gca_conv_fwd_stat_parts(gp) > 0
    g.act_f16 = 1                                               # fp16 storage: 2^30 - 1 elements are 2 GiB - 2 bytes, accepted
    g.N = c.N
    assert H.lib.gca_conv_fwd_stat_parts(gp) > 0
