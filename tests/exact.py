"""Operands on which the conv kernels have no rounding to hide behind, shared by the bit-exact GPU tests of the conv kernels,
their BatchNorm statistics and the fp16-storage path (tests/test_gpu_exact.py) and the CPU tests that assert every
precondition of every case (tests/test_exact.py).

The kernels accumulate in fp32.  When x, w and dy are small integers times a power of two (`grid`), every product and every
partial sum of a convolution is an integer multiple of unit_x * unit_w; as long as the sum of the ABSOLUTE values of the
terms stays below 2^24 of those units (`exact_in_fp32`), every partial sum in ANY order -- tile shape, split count, MFMA
order, the hi part of a bf16 split (mid = lo = 0: the operands have at most 6 significant bits, bf16 holds 8) -- is exactly representable,
so the fp64 reference (`conv_ref`) IS the answer and a kernel must reproduce it bit for bit.  An fp16 output must be the
round-to-nearest-even cast of that answer (`to_f16`); `n_inexact` / `n_ties` count how many elements of a reference really
exercise the rounding, so that no rounding test passes on representable values alone.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

F64 = torch.float64
BUDGET = 2.0 ** 24


def grid(shape, kmax, unit, seed):
    """fp64 values k * unit with k uniform in [-kmax, kmax]."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-kmax, kmax + 1, tuple(shape), generator=g).to(F64) * unit


def exact_in_fp32(ref_abs_sum, unit):
    """The share of the fp32 integer range a sum uses: max(sum |terms|) / unit / 2^24.  Below 1, every partial sum of the
    terms (multiples of `unit`) in any order is exact in fp32.  -> the ratio (callers assert < 1)."""
    return float(torch.as_tensor(ref_abs_sum, dtype=F64).abs().max()) / unit / BUDGET


def to_f16(r):
    """The fp16 value a kernel must store for the exact fp64 answer r.  Under `exact_in_fp32` the double -> float step is
    exact, so this is ONE rounding to nearest even (overflow to inf at |r| >= 65520 included)."""
    return r.float().half()


def _f16_quantum(r):
    """Spacing of fp16 around each |r| (fp64): 2^(e - 10) with e = floor(log2 |r|) clamped to the normal range [-14, 15]."""
    a = r.abs().clamp_min(2.0 ** -30)
    e = (torch.frexp(a)[1] - 1).clamp(-14, 15)
    return torch.ldexp(torch.ones_like(a), e - 10)


def n_inexact(r):
    """Elements of r (finite in fp16) that fp16 cannot hold."""
    q = r.abs() / _f16_quantum(r)
    return int(((q != q.floor()) & (r.abs() < 65520)).sum())


def n_ties(r):
    """Elements of r exactly half way between two neighbouring fp16 values."""
    q = r.abs() / _f16_quantum(r)
    return int(((q - q.floor() == 0.5) & (r.abs() <= 65520)).sum())


def rne_f16_integer(v):
    """Round-to-nearest-even of a Python float (a dyadic rational) to fp16 in INTEGER arithmetic, independent of any cast:
    -> the rounded value as a float (+-inf on overflow)."""
    if v == 0:
        return 0.0
    num, den = abs(v).as_integer_ratio()                    # exact: |v| = num / den, den a power of two
    e = num.bit_length() - den.bit_length()                 # floor(log2 |v|), or one more
    if (num << max(-e, 0)) < (den << max(e, 0)):
        e -= 1
    sh = max(e, -14) - 10                                   # quantum 2^sh = qn / qd (subnormals share the quantum 2^-24)
    qn, qd = (1 << sh, 1) if sh >= 0 else (1, 1 << -sh)
    n, rem = divmod(num * qd, den * qn)                     # |v| / quantum = n + rem / (den * qn)
    twice = 2 * rem
    if twice > den * qn or (twice == den * qn and n & 1):
        n += 1
    out = n * qn / qd
    if out >= 65536.0:
        out = float('inf')
    return out if v > 0 else -out


# ----------------------------------------------------------------------------- references
def conv_ref(x, w, bias, s, p, dy=None):
    """ATen in double -> dict(y [with bias], sy, sq [per channel, of the conv proper: the kernels take their BatchNorm
    statistics before the bias] [, dx, dw for the upstream gradient dy])."""
    xr, wr = x.to(F64).clone().requires_grad_(dy is not None), w.to(F64).clone().requires_grad_(dy is not None)
    y0 = F.conv3d(xr, wr, None, s, p)
    out = dict(y=y0.detach() if bias is None else y0.detach() + bias.to(F64).view(1, -1, 1, 1, 1),
               sy=y0.detach().sum((0, 2, 3, 4)), sq=(y0.detach() ** 2).sum((0, 2, 3, 4)))
    if dy is not None:
        y0.backward(dy.to(F64))
        out['dx'], out['dw'] = xr.grad, wr.grad
    return out


def conv_abs(x, w, bias, s, p, dy):
    """The same sums over absolute values: what `exact_in_fp32` is asked about.  -> dict(y, dx, dw, sy, sq)."""
    a = conv_ref(x.abs(), w.abs(), None if bias is None else bias.abs(), s, p, dy.abs())
    r = conv_ref(x, w, None, s, p)
    a['sy'] = r['y'].abs().sum((0, 2, 3, 4))
    a['sq'] = r['sq']
    return a


# ----------------------------------------------------------------------------- operand sets and cases
# name -> (kmax, unit) of x, of w and of dy.  MID, NARROW and ROUND are the sets the kernels are usually asked about; two
# more exist because a case needed them: WIDE, because a layer with few terms per output (24 channels x 9 taps, 40 or 64
# channels x 1 tap) sums ROUND operands to values fp16 still holds exactly, so it needs LARGER integers to reach values fp16
# must round -- all its budgets stay below 2 % of 2^24; SUBN, whose dy are fp16 subnormals.
SETS = {
    'MID': ((8, 1 / 4), (8, 1 / 8), (8, 1 / 4)),
    'NARROW': ((2, 1 / 2), (1, 1 / 2), (2, 1 / 2)),         # narrow enough for sum(y^2) per channel
    'ROUND': ((16, 1 / 4), (16, 1 / 8), (16, 1 / 4)),       # wide enough that thousands of outputs are not fp16 numbers
    'WIDE': ((63, 1 / 4), (63, 1 / 8), (63, 1 / 4)),
    'SUBN': ((8, 1 / 4), (8, 1 / 8), (4, 2.0 ** -22)),      # dy = k 2^-22: fp16 SUBNORMAL gradients
}

# id -> (set, shape, K, k, s, p, bias, sq asserted exactly).  Geometry: the smallest shapes of tests/test_gpu_ops.py and
# tests/test_gpu_f16.py (one clip where the kernel selection survives it); the comment names the test it comes from.
CASES = {
    # test_conv_every_launch_configuration
    'g0': ('MID', (3, 40, 5, 8, 8), 150, (3, 1, 1), (1, 1, 1), (1, 0, 0), False, False),
    'g1': ('MID', (2, 24, 6, 8, 8), 70, (3, 1, 1), (2, 1, 1), (1, 0, 0), False, False),
    'g2': ('MID', (2, 20, 3, 12, 12), 100, (1, 3, 3), (1, 2, 2), (0, 1, 1), False, False),
    'g3': ('MID', (2, 33, 1, 1, 1), 170, (1, 1, 1), (1, 1, 1), (0, 0, 0), False, False),
    'g0n': ('NARROW', (3, 40, 5, 8, 8), 150, (3, 1, 1), (1, 1, 1), (1, 0, 0), False, True),
    'g1n': ('NARROW', (2, 24, 6, 8, 8), 70, (3, 1, 1), (2, 1, 1), (1, 0, 0), False, True),
    'g2n': ('NARROW', (2, 20, 3, 12, 12), 100, (1, 3, 3), (1, 2, 2), (0, 1, 1), False, True),
    'g3n': ('NARROW', (2, 33, 1, 1, 1), 170, (1, 1, 1), (1, 1, 1), (0, 0, 0), False, True),
    # test_conv_halo_kernels_every_configuration, shapes 1, 2, 3 and 5 (h1 = g1, h4 = g2)
    'h0': ('MID', (2, 40, 5, 12, 13), 70, (1, 3, 3), (1, 1, 1), (0, 1, 1), True, False),
    'h2': ('MID', (1, 32, 4, 9, 10), 33, (3, 3, 3), (1, 1, 1), (1, 1, 1), True, False),
    'h0n': ('NARROW', (2, 40, 5, 12, 13), 70, (1, 3, 3), (1, 1, 1), (0, 1, 1), False, True),
    'h2n': ('NARROW', (1, 32, 4, 9, 10), 33, (3, 3, 3), (1, 1, 1), (1, 1, 1), False, True),
    # test_conv_stem_kernel_vs_gather_and_aten
    'st0': ('NARROW', (4, 3, 5, 37, 45), 20, (3, 5, 5), (2, 1, 2), (1, 2, 2), True, True),
    'st1': ('NARROW', (4, 1, 6, 33, 64), 33, (2, 2, 2), (1, 2, 2), (0, 0, 0), False, True),
    # test_temporal_convs_drop_taps_that_only_meet_padding
    't0': ('NARROW', (4, 48, 1, 4, 4), 40, (3, 1, 1), (1, 1, 1), (1, 0, 0), False, True),
    't1': ('NARROW', (3, 32, 2, 5, 5), 24, (3, 1, 1), (2, 1, 1), (1, 0, 0), False, True),
    't2': ('NARROW', (2, 32, 2, 4, 4), 32, (7, 1, 1), (1, 1, 1), (3, 0, 0), False, True),
    't3': ('NARROW', (2, 32, 3, 4, 4), 32, (3, 1, 1), (1, 1, 1), (1, 0, 0), False, True),
    # test_conv_wgrad_streaming_temporal_kernel (tiles 11, 12)
    'wt0': ('MID', (2, 40, 9, 4, 8), 48, (7, 1, 1), (1, 1, 1), (3, 0, 0), False, False),
    'wt1': ('MID', (3, 33, 5, 4, 4), 70, (7, 1, 1), (1, 1, 1), (3, 0, 0), False, False),
    'wt2': ('MID', (2, 32, 6, 4, 4), 40, (3, 1, 1), (1, 1, 1), (0, 0, 0), False, False),
    'wt3': ('MID', (2, 32, 3, 4, 4), 40, (3, 1, 1), (1, 1, 1), (2, 0, 0), False, False),
    # test_conv_wgrad_streaming_spatial_kernel (tile 13)
    'ws0': ('MID', (2, 40, 3, 8, 28), 48, (1, 3, 3), (1, 1, 1), (0, 1, 1), False, False),
    'ws1': ('MID', (2, 64, 1, 9, 4), 32, (1, 3, 3), (1, 1, 1), (0, 1, 1), False, False),
    'ws2': ('MID', (2, 33, 2, 7, 7), 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), False, False),
    'ws3': ('MID', (2, 32, 2, 6, 13), 32, (1, 3, 3), (1, 1, 1), (0, 1, 1), False, False),
    # test_conv_wgrad_stem_kernel (tile 14)
    'wm0': ('MID', (2, 3, 4, 22, 48), 20, (3, 5, 7), (1, 2, 2), (1, 2, 3), False, False),
    'wm1': ('MID', (2, 1, 3, 16, 32), 40, (3, 7, 5), (1, 2, 2), (1, 3, 2), False, False),
    'wm2': ('MID', (1, 3, 3, 40, 16), 33, (1, 7, 7), (1, 2, 2), (0, 3, 3), False, False),
    # test_conv_consumes_producer_batchnorm_relu_on_the_fly (x here is z = relu(y_in * scale + shift), see xf_operands)
    'xf0': ('MID', (3, 40, 6, 4, 8), 48, (3, 1, 1), (1, 1, 1), (1, 0, 0), False, False),
    'xf1': ('MID', (2, 110, 9, 4, 4), 64, (7, 1, 1), (1, 1, 1), (3, 0, 0), False, False),
    # test_conv_splitk_slabs_folded_by_the_batchnorm_kernel
    'sk0': ('NARROW', (4, 96, 2, 7, 7), 80, (3, 1, 1), (1, 1, 1), (1, 0, 0), False, True),
    'sk1': ('NARROW', (3, 64, 2, 6, 6), 48, (1, 3, 3), (1, 1, 1), (0, 1, 1), False, True),
    'sk2': ('NARROW', (2, 256, 1, 4, 4), 130, (1, 1, 1), (1, 1, 1), (0, 0, 0), False, True),
    # test_conv_bias_and_accumulate (a Linear layer with bias)
    'lin': ('MID', (5, 12, 1, 1, 1), 20, (1, 1, 1), (1, 1, 1), (0, 0, 0), True, False),
    # CONV_CASES[4] of tests/test_gpu_f16.py at one clip: 1x1x1 stride 2, dgrad leaves 7 of 8 positions unreached
    'p2': ('MID', (1, 128, 4, 14, 14), 512, (1, 1, 1), (2, 2, 2), (0, 0, 0), False, False),
    # fp16 storage: CONV_CASES 2, 6, 7, 9, 10 of tests/test_gpu_f16.py at one clip, and the stem case st0 (whole: one clip falls back to the gather kernel)
    'f2': ('ROUND', (1, 64, 6, 28, 28), 128, (3, 3, 3), (2, 2, 2), (1, 1, 1), False, False),
    'f6': ('WIDE', (1, 24, 5, 10, 10), 36, (1, 3, 3), (1, 2, 2), (0, 1, 1), True, False),
    'f7': ('WIDE', (4, 64, 1, 1, 1), 24, (1, 1, 1), (1, 1, 1), (0, 0, 0), True, False),
    'f9': ('WIDE', (1, 40, 2, 12, 12), 200, (1, 1, 1), (1, 1, 1), (0, 0, 0), True, False),
    'f10': ('ROUND', (1, 512, 2, 16, 16), 96, (1, 1, 1), (1, 1, 1), (0, 0, 0), False, False),
    'fst': ('ROUND', (4, 3, 5, 37, 45), 20, (3, 5, 5), (2, 1, 2), (1, 2, 2), True, False),
    'fp2': ('ROUND', (1, 128, 4, 14, 14), 512, (1, 1, 1), (2, 2, 2), (0, 0, 0), False, False),
    # the issue's ROUND reference shape (halo and gather kernels, split-K)
    'fr': ('ROUND', (2, 64, 4, 12, 12), 32, (3, 3, 3), (1, 1, 1), (1, 1, 1), False, False),
    # fp16 weight-gradient kernels: the gather tiles on fr, tile 14 on wm0 / wm2
    'fw0': ('ROUND', (2, 3, 4, 22, 48), 20, (3, 5, 7), (1, 2, 2), (1, 2, 3), False, False),
    'fw2': ('ROUND', (1, 3, 3, 40, 16), 33, (1, 7, 7), (1, 2, 2), (0, 3, 3), False, False),
    # fp16 subnormal gradients through dgrad and wgrad (halo / gather / pointwise kernels)
    'sub': ('SUBN', (1, 24, 5, 10, 10), 36, (1, 3, 3), (1, 2, 2), (0, 1, 1), False, False),
    'subp': ('SUBN', (1, 40, 2, 12, 12), 200, (1, 1, 1), (1, 1, 1), (0, 0, 0), False, False),
}
# The cases whose y AND dx each hold what a rounding test needs.  f7 (a Linear layer: 96 outputs, 256 input gradients) is too
# small to hold them; it is there for its kernel path, and the rounding of that path is held by f6 (same gather kernels).
ROUND_CASES = ['f2', 'f6', 'f9', 'f10', 'fst', 'fp2', 'fr']
MIN_INEXACT, MIN_TIES = 1000, 100           # per tensor


class Case:
    """Seeded operands of one CASES entry (fp64, CPU) + the exact reference + the absolute-value sums + the units."""

    def __init__(self, name):
        self.name = name
        st, self.shape, self.K, self.k, self.s, self.p, has_bias, self.sq_exact = CASES[name]
        self.set = st
        (kx, self.ux), (kw, self.uw), (kdy, self.udy) = SETS[st]
        seed = zlib.crc32(name.encode())                      # stable: adding a case reseeds no other
        self.x = grid(self.shape, kx, self.ux, seed)
        self.w = grid((self.K, self.shape[1]) + tuple(self.k), kw, self.uw, seed + 1)
        self.bias = grid((self.K,), 8, self.ux * self.uw, seed + 2) if has_bias else None
        y0 = F.conv3d(self.x[:1], self.w, None, self.s, self.p)
        self.out_shape = (self.shape[0],) + tuple(y0.shape[1:])
        self.dy = grid(self.out_shape, kdy, self.udy, seed + 3)
        self.ref = conv_ref(self.x, self.w, self.bias, self.s, self.p, self.dy)
        self.abs = conv_abs(self.x, self.w, self.bias, self.s, self.p, self.dy)

    def budgets(self):
        """-> dict of the shares of 2^24 every asserted sum uses."""
        u = self.ux * self.uw
        return dict(y=exact_in_fp32(self.abs['y'], u), dx=exact_in_fp32(self.abs['dx'], self.udy * self.uw),
                    dw=exact_in_fp32(self.abs['dw'], self.ux * self.udy), sy=exact_in_fp32(self.abs['sy'], u),
                    sq=exact_in_fp32(self.abs['sq'], u * u))


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ----------------------------------------------------------------------------- fused BatchNorm + ReLU producer
def xf_operands(C, seed):
    """Per-channel dyadic scale in {0.5, 1, 2} and shift in {-0.5, 0.25}: relu(y * scale + shift) of MID values is again a
    multiple of 1/8 below 5 (6 significant bits), computed without rounding by an fma or by a multiply and an add."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 3, (C,), generator=g)]
    shift = torch.tensor([-0.5, 0.25], dtype=F64)[torch.randint(0, 2, (C,), generator=g)]
    return scale, shift


@functools.lru_cache(maxsize=None)
def xf_case(name):
    """-> (y_in, scale, shift, Case-like record whose x is z = relu(y_in * scale + shift))."""
    c = Case(name)
    scale, shift = xf_operands(c.shape[1], 31 + len(name))
    y_in = c.x
    c.x = torch.relu(y_in * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1))
    c.ux = 1 / 8
    c.ref = conv_ref(c.x, c.w, None, c.s, c.p, c.dy)
    c.abs = conv_abs(c.x, c.w, None, c.s, c.p, c.dy)
    return y_in, scale, shift, c


# ----------------------------------------------------------------------------- fp16 element-wise kernels
ELEMENTWISE_SHAPES = [(2, 5, 8, 18, 18), (3, 6, 2, 5, 7)]          # SP % 4 == 0 (float4 path) and SP = 70 (scalar path)


@functools.lru_cache(maxsize=None)
def elementwise_operands(shape=ELEMENTWISE_SHAPES[0]):
    """x = k / 1024 and res = k / 128 with |k| <= 1024 (11 bits: fp16 numbers), per-channel scale in {0.25, 0.5, 1, 2, -1},
    shift = k / 2: x * scale + shift [+ res] is a multiple of 2^-12 below 32 -- exact in fp32 through a multiply and adds or
    an fma, mostly NOT an fp16 number."""
    g = torch.Generator().manual_seed(shape[1] * 13 + shape[4])
    scale = torch.tensor([0.25, 0.5, 1.0, 2.0, -1.0], dtype=F64)[torch.randint(0, 5, (shape[1],), generator=g)]
    return dict(shape=shape, x=grid(shape, 1024, 1 / 1024, 81), res=grid(shape, 1024, 1 / 128, 82), scale=scale,
                shift=grid((shape[1],), 16, 1 / 2, 83))


# ----------------------------------------------------------------------------- fp16 overflow boundary
@functools.lru_cache(maxsize=None)
def overflow_operands():
    """A pointwise conv (the geometry of case f9) whose weight rows are one-hot, so that it stores x[c] + bias[k].  Output
    channels 0..3 read input channel 0, where +-65504 are planted at four positions, with bias 8, -8, 16, -16.
    -> dict(x, w, bias, y = the exact answer)."""
    c = case('f9')
    C = c.shape[1]
    x = c.x.clone()
    x[0, 0, 0, 0, :4] = torch.tensor([65504.0, -65504.0, 65504.0, -65504.0], dtype=F64)
    w = torch.zeros((c.K, C, 1, 1, 1), dtype=F64)
    w[torch.arange(c.K), torch.tensor([0, 0, 0, 0] + [k % C for k in range(4, c.K)])] = 1.0
    bias = grid((c.K,), 8, 1 / 4, 94)
    bias[:4] = torch.tensor([8.0, -8.0, 16.0, -16.0], dtype=F64)
    return dict(x=x, w=w, bias=bias, y=conv_ref(x, w, bias, c.s, c.p)['y'])


# ----------------------------------------------------------------------------- accumulate=True bases, average pooling
def dgrad_base(c, half):
    """The live buffer a dgrad adds to: multiples of 1/32 up to 1/4 (fp32 storage) or of 1/4 up to 16 (fp16 storage, fp16
    numbers).  base + dx is again a multiple of the unit of dx."""
    return grid(c.shape, 64, 1 / 4, 95) if half else grid(c.shape, 8, 1 / 32, 99)


WGRAD_BASES = (0.5, 0.25)           # constants the weight-gradient tests pre-fill dw with before accumulate=True

AVGPOOL_CASES = [((2, 3, 4, 9, 11), (1, 2, 2)), ((1, 2, 5, 6, 7), (2, 2, 2)), ((1, 2, 4, 4, 4), (1, 2, 2))]


def avgpool_operands(shape, k):
    """x, dy, base = k / 8 with |k| <= 64 -> dict(x, dy, base, y, dx) with y / dx from F.avg_pool3d in double.  Windows of 4
    or 8 elements: sums below 2^24 / 8, the division by a power of two exact."""
    x = grid(shape, 64, 1 / 8, 92).requires_grad_(True)
    y = F.avg_pool3d(x, k)
    dy = grid(y.shape, 64, 1 / 8, 91)
    y.backward(dy)
    return dict(x=x.detach(), dy=dy, base=grid(shape, 64, 1 / 8, 90), y=y.detach(), dx=x.grad)
