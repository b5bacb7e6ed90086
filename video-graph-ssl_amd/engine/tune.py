"""Launch codes of the conv passes and the candidates the one-off launch tuning (ConvPlan.search in ops.py) measures: host
arithmetic on a conv geometry `g` (any object with the gca_conv_geom fields N, C, D, H, W, K, kd..kw, sd..sw, pd..pw, OD, OH, OW,
act_f16).  No library call, no torch, no module state; tests/test_tuner.py replays every list on a CPU."""
from collections import namedtuple
from math import prod

# A launch code is what the tuner pins in gca_conv_geom.tune_<pass>_<field> and what a tune-cache entry lists, in this order.
# All zeros (the default) = the library's own heuristic; CODES[which](*entry) reads a cache entry, a short one leaves the rest zero.
ConvCode = namedtuple('ConvCode', 'bm splits tail math box', defaults=(0,) * 5)      # forward (pass 0) and dgrad (1)
WgradCode = namedtuple('WgradCode', 'tile splits math', defaults=(0,) * 3)           # weight gradient (2)
CODES = (ConvCode, ConvCode, WgradCode)
PASSES = ('fwd', 'dgrad', 'wgrad')

# Flags of ConvCode.bm (the low bits are the tile rows, 32..160)
TUNE_VEC = 1024      # 256-column float4 variant of the gather kernels
TUNE_HALO = 2048     # LDS-halo kernel (conv3d_halo.hip), box in ConvCode.box
TUNE_STEM = 4096     # stem kernel (conv3d_stem.hip), forward only
TUNE_PW = 8192       # pointwise fp16 GEMM kernel (conv3d_pw.hip)

# WgradCode.tile 1..10: (rows, columns) of the gather kernel's tile; 11..14 are the streaming kernels (ConvPlan.WGRAD_KERNELS)
WGRAD_SHAPES = {1: (64, 64), 2: (64, 128), 3: (128, 64), 4: (128, 128), 5: (96, 128), 6: (160, 128), 7: (128, 96),
                8: (128, 160), 9: (64, 192), 10: (192, 64)}


def _gemm(which, g):
    """(M, Ntot) of the implicit GEMM of forward / dgrad: output rows (channels) and columns (positions)."""
    return (g.K, g.N * g.OD * g.OH * g.OW) if which == 0 else (g.C, g.N * g.D * g.H * g.W)


def gather_shapes(which, g):
    """(tile code, split) pairs of the gather kernels: tile code = rows (32..160) | TUNE_VEC for the 256-column float4 variant."""
    M, Ntot = _gemm(which, g)
    nk = -(-((g.C if which == 0 else g.K) * (g.kd * g.kh * g.kw)) // 16)      # 16-deep steps of the reduction
    pointwise = g.kh == 1 and g.kw == 1 and g.sh == 1 and g.sw == 1 and g.ph == 0 and g.pw == 0
    cands = []
    for vec in ((0, TUNE_VEC) if pointwise else (0,)):
        bn = 256 if vec else 128
        for bm in (32, 64, 96, 128, 160):
            padded = -(-M // bm) * bm
            if padded > 1.35 * max(M, 32) and bm > 32:       # skip tile heights that mostly multiply zeros
                continue
            tiles = -(-M // bm) * -(-Ntot // bn)
            for s in (1, 2, 3, 4, 6, 8, 12, 16):
                if s > 1 and (tiles >= 1024 or nk // s < 4 or s * M * Ntot * 4 > (96 << 20)):
                    continue
                cands.append((bm | vec, s))
    return cands


HaloBox = namedtuple('HaloBox', 'bm box')       # tile code | TUNE_HALO, box code d | h << 8 | w << 16


def halo_boxes(which, g):
    """LDS-halo kernel candidates: the few boxes with the least padding of the output grid x halo size, each with the tile
    heights that pad M least.  Unit-stride dgrad and forward only."""
    if which == 0:
        q, m, C = (g.OD, g.OH, g.OW), (g.sd, g.sh, g.sw), g.C
    else:
        if (g.sd, g.sh, g.sw) != (1, 1, 1):
            return []
        q, m, C = (g.D, g.H, g.W), (1, 1, 1), g.K
    k = (g.kd, g.kh, g.kw)
    if C < 16 or (g.kd * g.kh * g.kw) > 64:
        return []
    M = _gemm(which, g)[0]
    out = []
    for bn, nbox in ((128, 3), (256, 2)):
        boxes = []
        d = 1
        while d <= bn:
            h = 1
            while d * h <= bn:
                w = bn // (d * h)
                b = (d, h, w)
                if all(b[i] <= 2 * q[i] for i in range(3)):
                    P = prod((b[i] - 1) * m[i] + k[i] for i in range(3))             # halo positions staged per box
                    if P <= 384:
                        cover = prod(-(-q[i] // b[i]) * b[i] / q[i] for i in range(3))    # padding of the grid by whole boxes
                        cost = cover * (1.0 + 0.08 * P / bn) * (1.0 if w >= 8 else (1.1 if w >= 4 else 1.3))
                        boxes.append((cost, b))
                h *= 2
            d *= 2
        boxes.sort()
        tmax = 5 if bn == 128 else 3
        pads = sorted((-(-M // (32 * t)) * 32 * t, -t) for t in range(1, tmax + 1))
        rows = [32 * -t for _, t in pads[:2]]
        for cost, b in boxes[:nbox]:
            if cost > 2.0:
                continue
            for bm in rows:
                out.append(HaloBox(bm | TUNE_HALO, b[0] | (b[1] << 8) | (b[2] << 16)))
    return out


def wgrad_shapes(g):
    """(tile, split) pairs.  Shapes whose padding multiplies mostly zeros are skipped; the kernel refuses shapes it was not
    built for (the tuner then just skips them)."""
    M, Nred, kt = g.K, g.C * (g.kd * g.kh * g.kw), -(-(g.N * g.OD * g.OH * g.OW) // 32)
    cands = []
    least = min(-(-M // bm) * bm * -(-Nred // bn) * bn for bm, bn in WGRAD_SHAPES.values())
    for idx, (bm, bn) in WGRAD_SHAPES.items():
        padded = -(-M // bm) * bm * -(-Nred // bn) * bn
        if padded > 1.25 * least:
            continue
        tiles = -(-M // bm) * -(-Nred // bn)
        base = max(1, min(kt // 4, 1024 // max(1, tiles)))
        for f in (0.5, 1, 2):
            sp = max(1, min(kt, 1024, int(base * f)))
            if sp * M * Nred * 4 > (256 << 20):
                continue
            cands.append((idx, sp))
    # the streaming temporal kernel (conv3d_wgrad_ts.hip: tile 11 = 32, 12 = 64 output channels per wave); its split
    # is over (clip, 16-position chunk) units.  The library refuses it where it does not apply (fp32-MFMA mode, ...).
    hw = g.H * g.W
    if (g.kh, g.kw, g.sd, g.sh, g.sw, g.ph, g.pw) == (1, 1, 1, 1, 1, 0, 0) and g.kd in (3, 7) and hw % 16 == 0 and not g.act_f16:
        units = g.N * (hw // 16)
        for idx, tm in ((11, 1), (12, 2)):
            tiles = -(-M // (32 * tm)) * -(-g.C // 32)
            for nb in (256, 512, 1024):
                cands.append((idx, max(1, min(units // 4, -(-nb // tiles)))))
    # the streaming (1,3,3) kernel (tile 13): units = (clip, plane, 16-column chunk); one wave per SIMD, so the block
    # count that fills the chip once (256) and its multiples are the candidates worth timing
    if ((g.kd, g.kh, g.kw, g.sd, g.sh, g.sw, g.pd, g.ph, g.pw) == (1, 3, 3, 1, 1, 1, 0, 1, 1) and (g.W % 4 == 0 or g.W <= 16) and g.H >= 2
            and not g.act_f16):
        units = g.N * g.D * -(-g.W // 16)
        tiles = -(-M // 32) * -(-g.C // 32)
        for nb in (256, 512, 768):
            cands.append((13, max(1, min(units // 4, nb // tiles))))
    # the stem kernel (conv3d_wgrad_stem.hip, tile 14): <= 4 input channels, stride 2 along H and W; its split is over
    # (clip, od) units, one workgroup per (split, group of tap planes)
    if g.C <= 4 and (g.sd, g.sh, g.sw) == (1, 2, 2) and g.K <= 128:
        units = g.N * g.OD
        groups = (-(-g.kd // 2) if g.K <= 64 else g.kd) if g.kd > 1 else 1
        for nb in (256, 512, 1024, 2048):
            sp = max(1, min(units * max(1, g.OH // 8), nb // groups, 1024))     # (the library chunks the output rows past N * OD units)
            if sp * M * Nred * 4 <= (256 << 20):
                cands.append((14, sp))
    return sorted(set(cands))


def candidates(which, g, math):
    """The complete launch codes the tuner measures first for pass `which` under arithmetic mode `math` (gca_get_conv_math),
    in measuring order: for each arithmetic pin, for each launch shape."""
    # The arithmetic mode is a floor on accuracy: a pass may run a MORE accurate kernel when that one is faster
    # (math code = 1 + arithmetic; f32 > bf16x6 > bf16x3).  0 = the mode itself.
    pins = (0,) if g.act_f16 else {0: (0,), 2: (0, 1), 1: (0, 3, 1)}[math]
    if which == 2:
        return [WgradCode(tile, sp, m) for m in pins for tile, sp in wgrad_shapes(g)]
    shapes = [(bm, sp, 0) for bm, sp in gather_shapes(which, g)] + [(h.bm, 1, h.box) for h in halo_boxes(which, g)]
    if which == 0 and g.C <= 4 and g.sw == 2 and g.kw <= 8:
        shapes.append((TUNE_STEM | 64, 1, 0))                 # stem kernel (conv3d_stem.hip), box by its own heuristic
    if g.act_f16 and (g.kd * g.kh * g.kw) == 1:
        shapes.append((TUNE_PW | 128, 1, 0))                  # pointwise fp16 GEMM kernel (conv3d_pw.hip)
    return [ConvCode(bm, sp, 0, m, box) for m in pins for bm, sp, box in shapes]


def two_phase(which, g, base):
    """Two-phase launches on a fast single-launch code `base`: tall tiles for the full waves of workgroups, short tiles for
    the remainder (how many workgroups run at once is not known here, so a few guesses are measured).  Built for fp32
    storage, forward and unit-stride dgrad, un-split gather tiles taller than 32 rows only."""
    if which == 2 or g.act_f16 or (which == 1 and (g.sd, g.sh, g.sw) != (1, 1, 1)):
        return []
    if base.splits != 1 or base.bm >= TUNE_VEC or base.bm <= 32:
        return []
    M, Ntot = _gemm(which, g)
    tilesM, tilesN = -(-M // base.bm), -(-Ntot // 128)
    out, seen = [], set()
    for slots in (512, 768, 1024, 1280):
        main_cols = (tilesM * tilesN // slots) * slots // tilesM
        if main_cols <= 0 or main_cols >= tilesN or main_cols in seen:
            continue
        seen.add(main_cols)
        out += [base._replace(tail=(tail_rows // 32) | (main_cols << 8), box=0) for tail_rows in (32, 64) if tail_rows < base.bm]
    return out
