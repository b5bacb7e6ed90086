"""The cases of tests/test_gpu_large.py: conv, BatchNorm and pool kernels on ONE tensor of 2 to 4 GiB, and the helpers that
build their content.  tests/test_large_cases.py asserts every precondition of every case on the CPU.

Inside the conv kernels every address is a 32-bit byte offset through a buffer resource whose range ends at 0xfffff000
(BUF_MAX_BYTES); the BatchNorm and pool kernels index with 32-bit arithmetic below 2^31 elements.  A case makes exactly one
tensor large -- its element count sits in a BAND -- by stacking many small clips: convolution, pooling and the per-element
BatchNorm passes are independent per clip, so a 4 GiB result is verified against an fp64 reference of a handful of clips.
All operands are the dyadic grids of tests/exact.py: the reference is the answer bit for bit, every comparison is equality.

Two content patterns:
  periodic  clip n holds the content of clip n mod PERIOD.  Every output clip must equal output clip n mod PERIOD (checked
            on the device over the whole tensor) and the first PERIOD output clips must equal the fp64 reference.  PERIOD is
            7: an offset that wraps modulo ANY power of two lands in a clip of another phase (2^j mod 7 is never 0), so a
            wrapped or truncated offset cannot read or write a clip with the same content.
  sparse    the tensor is zero except in the named clips: clip 0, the clip holding byte offset 2^31, one clip wholly beyond
            it and the last clip ('all'), or the two beyond 2^31 alone ('beyond').  Every reduction over the batch (dw, the
            forward's BatchNorm sums, bn_stats, dgamma / dbeta, bias_grad) then has an fp64 reference over those clips.
"""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

import exact
from exact import F64

PERIOD = 7
BUF_MAX_BYTES = 0xfffff000
# band -> (lowest, highest) element count of the large tensor, inclusive
BANDS = {
    'T': (2 ** 30 - 2 ** 16, 2 ** 30 - 1024),       # fp32: crosses 2^31 bytes, ends within 256 KiB below BUF_MAX_BYTES
    'T16': (2 ** 30 - 2 ** 16, 2 ** 30 - 1),        # fp16 storage: just under 2 GiB, the es = 2 byte ranges
    'H': (2 ** 30 - 1023, 2 ** 30 - 1),             # fp32: below the element limit, the tail beyond BUF_MAX_BYTES
}

# family -> (ConvPlan.kernel name, float4-gather bit of gca_conv_kernel_cfg's last word)
FAMILIES = {'gather': ('gather', 0), 'vec': ('gather', 1), 'halo': ('halo', 0), 'stem': ('stem', 0), 'pw': ('pw', 0)}
WGRAD_TILES = {'gather': 1, 'temporal32': 11, 'spatial': 13, 'stem': 14}

Conv = collections.namedtuple('Conv', 'id family pas clip K k s p N big set band half tune extra')
# pas: 'fwd' / 'dgrad' (periodic content; a forward also runs the sparse content for its BatchNorm sums) or 'wgrad' (sparse)
# clip: (C, D, H, W) of one input clip;  big: the large tensor ('x', 'y', 'dy', 'dx');  tune: tune_* fields of the plan
# extra: '' | 'xf' (conv_fwd_xf) | 'merged' (one launch over the stride classes) | 'splitk' | 'dzf' (conv_wgrad_dzf + bn_bwd_sums)

BOX_288 = 2 | 8 << 8 | 8 << 16              # one (2, 8, 8) clip = one 128-position box of the LDS-halo kernels
SRC, DST = dict(clip=(64, 2, 8, 8), K=8), dict(clip=(8, 2, 8, 8), K=64)       # 8192 : 1024 elements per clip, either way round
N64 = 2 ** 17 - 1                           # 8192 * N64 = 2^30 - 8192
K133, K311, K111 = ((1, 3, 3), (1, 1, 1), (0, 1, 1)), ((3, 1, 1), (1, 1, 1), (1, 0, 0)), ((1, 1, 1), (1, 1, 1), (0, 0, 0))
STEM = dict(clip=(3, 2, 8, 16), k=(3, 3, 3), s=(1, 2, 2), p=(1, 1, 1))        # 768 elements in, K * 64 out per clip
N_STEM_X = 1398080                          # 768 * N = 2^30 - 16384


def _conv(cid, family, pas, geo, ksp, big, tune, st=None, band='T', half=False, extra='', N=N64):
    k, s, p = ksp
    return Conv(cid, family, pas, geo['clip'], geo['K'], k, s, p, N, big, st or ('NARROW' if pas == 'fwd' else 'MID'), band, half,
                tune, extra)


def _four(family, ksp, code, band='T', half=False, box=0, tag=None):
    """Forward and dgrad, large source and large destination, of one kernel family."""
    out = []
    for pas, big, geo in (('fwd', 'x', SRC), ('fwd', 'y', DST), ('dgrad', 'dy', DST), ('dgrad', 'dx', SRC)):
        tune = {pas + '_bm': code}
        if box:
            tune[pas + '_box'] = box
        out.append(_conv('%s-%s-%s' % (tag or family, pas, big), family, pas, geo, ksp, big, tune, band=band, half=half))
    return out


CONV_CASES = (
    _four('gather', K133, 64) + _four('vec', K311, 1024 | 64) + _four('halo', K133, 2048 | 64, box=BOX_288) +
    # a pointwise conv: on fp32 tensors the float4 gather kernels run it, on fp16 tensors the pointwise GEMM kernel (which
    # exists for fp16 storage only, hence band T16)
    _four('vec', K111, 1024 | 64, tag='pointwise') + _four('pw', K111, 8192 | 128, band='T16', half=True) + [
        _conv('gather16-fwd-x', 'gather', 'fwd', SRC, K133, 'x', {'fwd_bm': 64}, band='T16', half=True),
        _conv('stem-fwd-x', 'stem', 'fwd', dict(clip=STEM['clip'], K=4), (STEM['k'], STEM['s'], STEM['p']), 'x', {'fwd_bm': 4096 | 64},
              N=N_STEM_X),
        _conv('xf-fwd-x', 'halo', 'fwd', SRC, K311, 'x', {'fwd_bm': 2048 | 64, 'fwd_box': BOX_288}, st='MID', extra='xf'),
        _conv('merged-dgrad-dx', 'gather', 'dgrad', SRC, ((1, 3, 3), (1, 2, 2), (0, 1, 1)), 'dx', {'dgrad_bm': 64}, extra='merged'),
        _conv('splitk-fwd-y', 'gather', 'fwd', DST, K133, 'y', {'fwd_bm': 64, 'fwd_splits': 2}, extra='splitk'),
    ])

WGRAD_CASES = [_conv('w%s-%s' % (fam, big), fam, 'wgrad', geo, ksp, big, {'wgrad_tile': WGRAD_TILES[fam], 'wgrad_splits': sp})
               for fam, ksp, sp in (('gather', K133, 4), ('temporal32', K311, 0), ('spatial', K133, 0))
               for big, geo in (('x', SRC), ('dy', DST))] + \
              [_conv('w%s-%s' % (tag, big), 'stem', 'wgrad', dict(clip=STEM['clip'], K=K), (STEM['k'], STEM['s'], STEM['p']), big,
                     {'wgrad_tile': 14, 'wgrad_splits': 0}, extra=extra, N=N)
               for tag, extra in (('stem', ''), ('dzf', 'dzf')) for big, K, N in (('x', 4, N_STEM_X), ('dy', 128, N64))]

# Band H: 2^21 - 1 clips of 512 elements = 2^30 - 512 elements; the last clip lies wholly beyond BUF_MAX_BYTES
H_SRC, H_DST, N_H = dict(clip=(16, 2, 4, 4), K=2), dict(clip=(2, 2, 4, 4), K=16), 2 ** 21 - 1
H_CASES = [_conv('H-fwd-x', 'gather', 'fwd', H_SRC, K133, 'x', {'fwd_bm': 64}, band='H', N=N_H),
           _conv('H-fwd-y', 'gather', 'fwd', H_DST, K133, 'y', {'fwd_bm': 64}, band='H', N=N_H),
           _conv('H-wgrad-x', 'gather', 'wgrad', H_SRC, K133, 'x', {'wgrad_tile': 1, 'wgrad_splits': 4}, band='H', N=N_H)]

Bn = collections.namedtuple('Bn', 'id op C sp N vec')
# VEC 4: planes of 256 elements (SP % 4 == 0); VEC 1: planes of 135
BN_CASES = [Bn('bn-%s-v%d' % (op, vec), op, 8, sp, N, vec) for op in ('stats', 'apply', 'bwd')
            for vec, sp, N in ((4, (4, 8, 8), 2 ** 19 - 1), (1, (3, 5, 9), 994200))]

Pool = collections.namedtuple('Pool', 'id kind clip k s p N')
# the input (and dx) is the large tensor: 2^19 - 1 clips of (8, 4, 8, 8)
POOL_CASES = [Pool('maxpool-pair333s2', 'max', (8, 4, 8, 8), (3, 3, 3), (2, 2, 2), (1, 1, 1), 2 ** 19 - 1),        # paired fwd / brick bwd
              Pool('maxpool-unrolled133', 'max', (8, 4, 8, 8), (1, 3, 3), (1, 2, 2), (0, 1, 1), 2 ** 19 - 1),      # <1,3,3> fwd, <1,2,2> bwd
              Pool('maxpool-runtime321', 'max', (8, 4, 8, 8), (3, 2, 1), (2, 2, 1), (1, 1, 0), 2 ** 19 - 1),       # run-time window both ways
              Pool('avgpool-222', 'avg', (8, 4, 8, 8), (2, 2, 2), (2, 2, 2), (0, 0, 0), 2 ** 19 - 1)]

ALL_CONV = {c.id: c for c in CONV_CASES + WGRAD_CASES + H_CASES}


# ----------------------------------------------------------------------------- geometry
def prod(v):
    out = 1
    for a in v:
        out *= int(a)
    return out


def out_clip(c):
    """(K, OD, OH, OW) of one output clip."""
    return (c.K,) + tuple((c.clip[1 + i] + 2 * c.p[i] - c.k[i]) // c.s[i] + 1 for i in range(3))


def clip_elems(c):
    """Elements of one clip of the large tensor."""
    if isinstance(c, Bn):
        return c.C * prod(c.sp)
    if isinstance(c, Pool):
        return prod(c.clip)
    return prod(c.clip if c.big in ('x', 'dx') else out_clip(c))


def large_elems(c):
    return c.N * clip_elems(c)


def elem_size(c):
    return 2 if getattr(c, 'half', False) else 4


def clip_at_byte(c, byte):
    """The clip of the large tensor that holds byte offset `byte`."""
    return byte // (clip_elems(c) * elem_size(c))


def named_clips(c, variant='all'):
    """Clip 0, the clip holding byte 2^31, one wholly beyond it (half way to the end), the last.  'beyond': the last two.
    A tensor that ends below 2^31 bytes (fp16 storage) names the clips at the same fractions of its length."""
    mid = clip_at_byte(c, 2 ** 31)
    if mid >= c.N - 2:
        mid = c.N // 2
    ids = [0, mid, (mid + c.N) // 2, c.N - 1]
    return ids if variant == 'all' else ids[2:]


def seed_of(c):
    return zlib.crc32(c.id.encode()) & 0x7fffffff


def grids(c):
    return exact.SETS[c.set]


# ----------------------------------------------------------------------------- content: conv
@functools.lru_cache(maxsize=None)
def weights(cid):
    c = ALL_CONV[cid]
    (_, _), (kw, uw), _ = grids(c)
    return exact.grid((c.K, c.clip[0]) + tuple(c.k), kw, uw, seed_of(c) + 1)


@functools.lru_cache(maxsize=None)
def periodic(cid):
    """PERIOD clips of x and dy, the fp64 reference y / dx per clip and the absolute-value sums behind `exact_in_fp32`.
    'xf' cases: x is y_in, the conv runs on z = relu(y_in * scale + shift) (exact.xf_operands)."""
    c = ALL_CONV[cid]
    (kx, ux), (_, uw), (kdy, udy) = grids(c)
    sd = seed_of(c)
    x = exact.grid((PERIOD,) + c.clip, kx, ux, sd)
    dy = exact.grid((PERIOD,) + out_clip(c), kdy, udy, sd + 3)
    w = weights(cid)
    out = dict(x=x, dy=dy, w=w, ux=ux, uw=uw, udy=udy)
    xe = x
    if c.extra == 'xf':
        out['scale'], out['shift'] = exact.xf_operands(c.clip[0], sd + 5)
        xe = torch.relu(x * out['scale'].view(1, -1, 1, 1, 1) + out['shift'].view(1, -1, 1, 1, 1))
        out['ux'] = 1 / 8
    out['ref'] = exact.conv_ref(xe, w, None, c.s, c.p, dy)
    out['abs'] = exact.conv_abs(xe, w, None, c.s, c.p, dy)
    return out


@functools.lru_cache(maxsize=None)
def sparse(cid, variant):
    """Content of the named clips (x, dy: one row per named clip) and the fp64 reference over them alone: y per clip, its
    per-channel sums sy / sq, dw.  'dzf' cases: dy is the BatchNorm backward of (dz, y) -- see dzf_operands."""
    c = ALL_CONV[cid]
    (kx, ux), (_, uw), (kdy, udy) = grids(c)
    sd = seed_of(c)
    ids = named_clips(c, variant)
    pick = [named_clips(c, 'all').index(i) for i in ids]
    x = exact.grid((4,) + c.clip, kx, ux, sd + 10)[pick]
    dy = exact.grid((4,) + out_clip(c), kdy, udy, sd + 13)[pick]
    w = weights(cid)
    out = dict(ids=ids, x=x, dy=dy, w=w, ux=ux, uw=uw, udy=udy)
    if c.extra == 'xf':
        out['scale'], out['shift'] = exact.xf_operands(c.clip[0], sd + 5)
        # a clip of zeros is NOT neutral behind relu(0 * scale + shift): the zero clips hold -4, which every (scale, shift) of
        # exact.xf_operands maps to relu(<= -1.75) = 0
        out['fill'] = -4.0
        xe = torch.relu(x * out['scale'].view(1, -1, 1, 1, 1) + out['shift'].view(1, -1, 1, 1, 1))
        out['ux'] = 1 / 8
        out['ref'], out['abs'] = exact.conv_ref(xe, w, None, c.s, c.p, dy), exact.conv_abs(xe, w, None, c.s, c.p, dy)
        return out
    if c.extra == 'dzf':
        out.update(dzf_operands(c, x, dy))
        dy = out['dy_eff']
        out['udy'] = udy / 4                                  # A = gamma * invstd is a multiple of 1/4
    out['ref'], out['abs'] = exact.conv_ref(x, w, None, c.s, c.p, dy), exact.conv_abs(x, w, None, c.s, c.p, dy)
    return out


def dzf_operands(c, x, dz):
    """BatchNorm behind the conv, for conv_wgrad_dzf: the kernel forms dy = A (m dz - B - xhat Cc), B = S1 / M, Cc = S2 / M with
    M = N * SP -- not a power of two, so B and Cc are dyadic only when S1 = sum m dz and S2 = sum m dz xhat are ZERO.  The named
    clips therefore come in pairs that share y (hence the mask m and xhat) and hold dz and -dz: the sums cancel exactly in
    the kernel's fp64 accumulators, dy = A m dz, while x differs inside a pair, so dw does not cancel.
    -> dict(y, dz [paired], gamma, mean, invstd, scale, shift, dy_eff)"""
    K = c.K
    g = torch.Generator().manual_seed(seed_of(c) + 21)
    pick = lambda vals: torch.tensor(vals, dtype=F64)[torch.randint(0, len(vals), (K,), generator=g)]
    gamma, invstd, mean, beta = pick([0.5, 1.0, 2.0]), pick([0.5, 1.0, 2.0]), pick([-0.5, -0.25, 0.0, 0.25, 0.5]), pick([-0.5, 0.0, 0.25])
    scale = gamma * invstd
    shift = beta - mean * scale
    y = exact.grid((len(dz),) + out_clip(c), 8, 1 / 4, seed_of(c) + 22)
    y, dz = y.clone(), dz.clone()
    for a in range(0, len(dz), 2):
        y[a + 1], dz[a + 1] = y[a], -dz[a]
    v = lambda t: t.view(1, -1, 1, 1, 1)
    mask = (y * v(scale) + v(shift) > 0).to(F64)
    return dict(y=y, dz=dz, gamma=gamma, mean=mean, invstd=invstd, scale=scale, shift=shift, mask=mask, dy_eff=v(scale) * mask * dz)


def budgets(c, o, what):
    """Shares of 2^24 (exact.exact_in_fp32) of the sums named in `what`, for content `o` of periodic() / sparse()."""
    unit = dict(y=o['ux'] * o['uw'], dx=o['udy'] * o['uw'], dw=o['ux'] * o['udy'], sy=o['ux'] * o['uw'], sq=(o['ux'] * o['uw']) ** 2)
    return {n: exact.exact_in_fp32(o['abs'][n], unit[n]) for n in what}


# ----------------------------------------------------------------------------- content: BatchNorm, pools
@functools.lru_cache(maxsize=None)
def bn_operands(cid):
    """Per-channel dyadic parameters; PERIOD clips of x, a residual and dz; four named clips for the sums.
    bn_apply: relu(x * scale + shift + res) is exact in fp32 (multiples of 1/8 below 64).
    bn_bwd (large path): dx = A (m dz - S1 / M - xhat S2 / M) with M = N * SP not a power of two, so the periodic dz is built to
    make S1 = S2 = 0: clips (0, 1), (2, 3), (4, 5) of a period share x and hold dz and -dz, clip 6 and the clips past the
    last whole period hold dz = 0.  The kernels accumulate in fp64 and round each part to fp32: every part of the cancelling
    sequence sums to less than one period of terms, far below 2^24 units.  Then dx = A m dz exactly.
    dgamma / dbeta come from the sparse content (x, dz in the named clips, zero elsewhere): exact sums, not zero."""
    c = next(b for b in BN_CASES if b.id == cid)
    sd = zlib.crc32(cid.encode()) & 0x7fffffff
    g = torch.Generator().manual_seed(sd)
    pick = lambda vals: torch.tensor(vals, dtype=F64)[torch.randint(0, len(vals), (c.C,), generator=g)]
    gamma, invstd, mean, beta = pick([0.5, 1.0, 2.0]), pick([0.5, 1.0, 2.0]), pick([-0.5, -0.25, 0.0, 0.25, 0.5]), pick([-0.5, 0.0, 0.25])
    scale = gamma * invstd
    shift = beta - mean * scale
    clip = (c.C,) + c.sp
    x, res, dz = (exact.grid((PERIOD,) + clip, 8, 1 / 4, sd + i) for i in (1, 2, 3))
    for a in (0, 2, 4):
        x[a + 1], dz[a + 1] = x[a], -dz[a]
    dz[6] = 0
    v = lambda t: t.view(1, -1, 1, 1, 1)
    mask = (x * v(scale) + v(shift) > 0).to(F64)
    z = torch.relu(x * v(scale) + v(shift) + res)
    xs, dzs = exact.grid((4,) + clip, 8, 1 / 4, sd + 4), exact.grid((4,) + clip, 8, 1 / 4, sd + 5)
    ms = (xs * v(scale) + v(shift) > 0).to(F64)
    xhat = (xs - v(mean)) * v(invstd)
    return dict(gamma=gamma, invstd=invstd, mean=mean, scale=scale, shift=shift, x=x, res=res, dz=dz, z=z, dx=v(scale) * mask * dz,
                xs=xs, dzs=dzs, ms=ms, xhat=xhat)


@functools.lru_cache(maxsize=None)
def pool_operands(cid):
    """PERIOD clips whose values are all different (a permutation of 0 .. n-1 times 1/4: no ties, so the argmax is unique), dy
    on the MID grid, and ATen in double: y, argmax (plane-relative index, as the kernels store it), dx."""
    c = next(p for p in POOL_CASES if p.id == cid)
    sd = zlib.crc32(cid.encode()) & 0x7fffffff
    n = PERIOD * prod(c.clip)
    x = (torch.randperm(n, generator=torch.Generator().manual_seed(sd)).to(F64) - n // 2).view((PERIOD,) + c.clip) / 4
    xr = x.clone().requires_grad_(True)
    if c.kind == 'max':
        y, am = F.max_pool3d(xr, c.k, c.s, c.p, return_indices=True)
    else:
        y, am = F.avg_pool3d(xr, c.k), None
    dy = exact.grid(y.shape, 8, 1 / 4, sd + 1)
    y.backward(dy)
    return dict(x=x, y=y.detach(), argmax=am, dy=dy, dx=xr.grad)


# ----------------------------------------------------------------------------- building and checking the large tensors
def tile(small, N):
    """(P, ...) -> (N, ...) on small's device with clip n = small[n mod P]."""
    P = small.shape[0]
    reps, rem = divmod(N, P)
    big = torch.empty((N,) + tuple(small.shape[1:]), dtype=small.dtype, device=small.device)
    big[:reps * P].view(reps, P, -1).copy_(small.reshape(1, P, -1).expand(reps, P, -1))
    if rem:
        big[reps * P:].copy_(small[:rem])
    return big


def is_periodic(big, P=PERIOD, chunk=1 << 27):
    """Every clip n of `big` equals clip n mod P bit for bit (no NaN anywhere), compared on big's device `chunk` elements at a time."""
    N = big.shape[0]
    head = big[:P].reshape(1, P, -1)
    per = max(1, chunk // head.numel())
    reps, rem = divmod(N, P)
    for r0 in range(0, reps, per):
        r1 = min(reps, r0 + per)
        if not bool((big[r0 * P:r1 * P].view(r1 - r0, P, -1) == head).all()):
            return False
    return rem == 0 or bool((big[reps * P:].reshape(rem, -1) == head[0, :rem]).all())


def mismatch(big, P=PERIOD, chunk=1 << 27):
    """For the message of a failed is_periodic: how many clips differ from their phase, the first and the last of them, and
    what the last one holds."""
    N = big.shape[0]
    head = big[:P].reshape(P, -1)
    per = max(1, chunk // head.numel()) * P
    bad = []
    for n0 in range(0, N, per):
        n1 = min(N, n0 + per)
        want = head.repeat(-(-(n1 - n0) // P), 1)[:n1 - n0]
        bad.append(n0 + (big[n0:n1].reshape(n1 - n0, -1) != want).any(1).nonzero().flatten().cpu())
    bad = torch.cat(bad)
    if not len(bad):
        return 'periodic'
    last = big[int(bad[-1])].reshape(-1)
    return '%d of %d clips differ from their phase, first %d, last %d; the last holds %d NaN, %d non-zero of %d elements' % (
        len(bad), N, int(bad[0]), int(bad[-1]), int(last.isnan().sum()), int(last.count_nonzero()), last.numel())


def scatter(small, ids, N, fill=0.0):
    """(len(ids), ...) -> (N, ...) holding `fill` except clips ids[i] = small[i]."""
    big = torch.full((N,) + tuple(small.shape[1:]), fill, dtype=small.dtype, device=small.device)
    big[torch.as_tensor(ids, device=small.device)] = small
    return big


def only_in(big, ids):
    """No non-zero element of `big` outside clips `ids`."""
    inside = int((big[torch.as_tensor(ids, device=big.device)] != 0).sum())
    step = max(1, (1 << 27) // big[0].numel())            # (count_nonzero would widen the whole tensor to int64 first)
    return sum(int((big[n:n + step] != 0).sum()) for n in range(0, big.shape[0], step)) == inside


def plan_for(ops, c, device):
    """The ConvPlan of a case with its launch codes pinned (the way tests/test_gpu_exact.py forces them)."""
    plan = ops.ConvPlan(c.N, *c.clip, c.K, c.k, c.s, c.p, device, act_f16=c.half)
    plan.tuned = [True, True, True]
    for field, v in c.tune.items():
        setattr(plan.g, 'tune_' + field, v)
    plan.refresh()
    return plan


def resolved(plan, c):
    """-> (family the plan resolves to for the case's pass, what the case names)."""
    if c.pas == 'wgrad':
        return plan.kernel(2), c.family
    which = 0 if c.pas == 'fwd' else 1
    kernel = plan.kernel(which)            # (the float4 bit tells the two gather forms apart; the other kernels do not gather)
    return (kernel, plan.cfg(which)[3] >> 10 & 1 if kernel == 'gather' else 0), FAMILIES[c.family]
