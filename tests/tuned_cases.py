"""One test case per (arithmetic prefix, geometry) of profiles/tune_cache.json, for tests/test_tuned_cases.py (CPU: every
case launches what its cache entries launch) and tests/test_gpu_tuned.py (GPU: what that launch computes).  Host arithmetic
and host-only library queries; nothing here touches a device or launches a kernel.

A case carries the up-to-three launch codes the cache holds for its geometry (forward, dgrad, wgrad).  If its forward pass
has at most MAC_BUDGET multiply-adds and x, w and y have at most ELEM_BUDGET elements each, it runs AS CACHED: at the
geometry of the key, its codes adopted from the cache by the tuner.  Otherwise it runs SHRUNKEN: C, K, kernel, stride,
padding, storage type and "x is a channel slice of a wider batch" are the key's, and (N, D, H, W) are the extents with the
fewest multiply-adds (ties: smallest N, D, H, W) for which `violations` is empty, i.e. the library resolves the pinned codes
to the same kernel, the same tile, the same configuration word, the same splits, box and tail rows as at full size, and

  * forward and dgrad run at least two full column tiles and a ragged one (pointwise fp16 kernel: per clip, with
    D*H*W % 8 == 0; the stem kernel tiles by boxes it picks from the grid and only wants its 8192 outputs); an LDS-halo
    pass keeps, on every axis that had more than one box, at least two boxes with a ragged last one (a box extent of 1
    cannot be ragged), and an axis that fit one box still does;
  * a two-phase code keeps its short-tile rows and splits the column tiles at tilesN // 2;
  * the reduction is the same: same classes, same taps per class (gather-table rows, packed elements), same float4 paths
    (W keeps its residue mod 4 where the configuration word reports one, and for the streaming (1,3,3) weight gradient);
  * the weight gradient resolves to the split count it resolves to at full size, or to the cached count itself (the
    library evens a split out over its units: 21 cached splits of 128 units run as 19 splits of 7 units).  Where no
    geometry inside the two budgets does (`wgrad_clamped`), it takes the most positions the budgets allow, still split at
    least two ways where the code asks for two or more, the last split ragged if it was ragged at full size.

The search (`build`) prefers, in this order: boxes ragged on every axis over ragged on at least one (`relaxed_boxes`: some
streaming weight gradients want H * W % 16 == 0 where the boxes want an odd H); a geometry inside the two budgets over the
cheapest one outside them (deep layers on tiny grids need more clips than the budget buys to fill three column tiles); the
full split count of the weight gradient over a clamped one.  Its window is N <= 8 clips (all of them on grids below 4096
positions), D <= 16 and H, W <= 128.  An entry for which nothing smaller keeps these invariants would run at its own size
(`forced_full`); tests/test_tuned_cases.py asserts that there is none, and lists the cases with relaxed boxes.
"""
import collections
import functools
import importlib

import numpy as np
import torch

from test_tuner import committed_cache, parse_key

MAC_BUDGET = 1 << 30            # multiply-adds of the forward pass
ELEM_BUDGET = 4 << 20           # elements of x, of w and of y
CPU = torch.device('cpu')
MODE_NAMES = {'': 'f32', 'b': 'bf16x3', 'c': 'bf16x6', 'h': 'fp16'}

Entry = collections.namedtuple('Entry', 'id prefix mode f16 geom codes')
# geom: the 16 ints of the key; codes: ((pass, the cache entry), ...)
Run = collections.namedtuple('Run', 'entry geom codes shrunken forced_full wgrad_clamped relaxed_boxes')
# geom: the 16 ints the case runs at (x_batch_stride re-derived); codes: {pass: tune.ConvCode / tune.WgradCode} to pin


def _pkg():
    return importlib.import_module('video-graph-ssl_amd')


def case_id(prefix, geom):
    N, C, D, H, W, K, kd, kh, kw, sd, sh, sw, pd, ph, pw, xbs = geom
    return '%s-n%d-c%d-%dx%dx%d-k%d-%d%d%d-s%d%d%d-p%d%d%d%s' % (prefix, N, C, D, H, W, K, kd, kh, kw, sd, sh, sw, pd, ph, pw,
                                                                  '-view' if xbs else '')


@functools.lru_cache(maxsize=None)
def entries():
    """Every (prefix, geometry) of the committed cache with the codes of its passes, sorted by geometry then prefix (so that
    cases sharing a reference run next to each other)."""
    by = collections.OrderedDict()
    for key, entry in committed_cache():
        prefix = key.split(':')[0]
        _, f16, which, geom = parse_key(key)
        by.setdefault((tuple(geom), prefix), {})[which] = tuple(entry)
    out = []
    for (geom, prefix), codes in sorted(by.items()):
        mode = prefix.lstrip('v0123456789')
        out.append(Entry(case_id(prefix, geom), prefix, MODE_NAMES[mode], mode == 'h', geom, tuple(sorted(codes.items()))))
    assert len({e.id for e in out}) == len(out)
    return tuple(out)


def out_dims(geom):
    return tuple((n + 2 * p - k) // s + 1 for n, p, k, s in zip(geom[2:5], geom[12:15], geom[6:9], geom[9:12]))


def macs(geom):
    N, C, K = geom[0], geom[1], geom[5]
    return N * K * int(np.prod(out_dims(geom))) * C * geom[6] * geom[7] * geom[8]


def elems(geom):
    N, C, D, H, W, K = geom[:6]
    return max(N * C * D * H * W, K * C * geom[6] * geom[7] * geom[8], N * K * int(np.prod(out_dims(geom))))


def runs_as_cached(geom):
    return macs(geom) <= MAC_BUDGET and elems(geom) <= ELEM_BUDGET


# ----------------------------------------------------------------------------- what a plan launches
def set_mode(entry):
    """Set the library's arithmetic mode for `entry` (fp16 storage multiplies under the bf16x6 setting); -> the previous one."""
    H = _pkg()._hip
    prev = H.lib.gca_get_conv_math()
    assert H.lib.gca_set_conv_math({'f32': 0, 'bf16x3': 1, 'bf16x6': 2, 'fp16': 2}[entry.mode]) == 0
    return prev


def make_plan(geom, f16, device, codes=None):
    """A fresh ConvPlan of `geom` (not the cached one of ops.conv_plan), tuner off, `codes` pinned."""
    ops = _pkg().engine.ops
    N, C, D, H, W, K, kd, kh, kw, sd, sh, sw, pd, ph, pw, xbs = geom
    plan = ops.ConvPlan(N, C, D, H, W, K, (kd, kh, kw), (sd, sh, sw), (pd, ph, pw), device, xbs, act_f16=f16)
    plan.tuned = [True] * 3
    for which, code in sorted((codes or {}).items()):
        plan.set_code(which, code)
    return plan


def codes_of(entry):
    tune = _pkg().engine.tune
    return {which: tune.CODES[which](*c) for which, c in entry.codes}


def first_class_positions(geom, which):
    """Columns of the implicit GEMM of the class gca_conv_kernel_cfg reports: every output position (forward), the input
    positions of stride residue 0 (dgrad)."""
    if which == 0:
        return geom[0] * int(np.prod(out_dims(geom)))
    return geom[0] * int(np.prod([-(-n // s) for n, s in zip(geom[2:5], geom[9:12])]))


def grid_of(geom, which):
    """The position grid a halo box tiles: the output grid (forward), the input grid (unit-stride dgrad)."""
    return out_dims(geom) if which == 0 else tuple(geom[2:5])


def box_of(code):
    return (code.box & 255, code.box >> 8 & 255, code.box >> 16 & 255)


def tail_in_force(plan, geom, which, code):
    """(short-tile rows, main column tiles) of the two-phase launch the library runs for `code` on `plan`, or (0, 0): the
    admission rule of cfg_for in csrc/conv3d.hip (single class, gather kernel, fp32 storage, 128 columns, no split)."""
    cfg = plan.cfg(which)
    tb, mc = (code.tail & 255) * 32, code.tail >> 8
    tiles = -(-first_class_positions(geom, which) // 128)
    ok = (code.tail > 0 and plan.kernel(which) == 'gather' and not plan.g.act_f16 and cfg[3] & 255 == 1 and cfg[2] == 1 and
          cfg[1] == 128 and 32 <= tb < cfg[0] and 0 < mc < tiles)
    return (tb, mc) if ok else (0, 0)


def wgrad_units(geom, tile):
    """(units the weight gradient's split runs over, the most splits the library grants), or None where the unit count is the
    stem kernel's own (tile 14: output rows in chunks)."""
    N, C, D, H, W = geom[:5]
    if tile in (11, 12):
        u = N * (H * W // 16)
        return u, max(1, u // 4)
    if tile == 13:
        u = N * D * -(-W // 16)
        return u, max(1, u // 4)
    if tile == 14:                      # (clip, od) units, the output rows in chunks of >= 8: an upper bound
        od, oh, _ = out_dims(geom)
        u = N * od * max(1, oh // 8)
        return u, u
    u = -(-N * int(np.prod(out_dims(geom))) // 32)
    return u, u


def wgrad_last_split_ragged(geom, tile, splits):
    u = wgrad_units(geom, tile)
    if tile == 14 or splits < 1:
        return None
    return u[0] % -(-u[0] // splits) != 0


def describe(plan, geom, codes):
    """Everything `violations` compares, per pass."""
    H = _pkg()._hip
    out = {}
    for which, code in codes.items():
        d = dict(kernel=plan.kernel(which), cfg=plan.cfg(which))
        if which < 2:
            d['rows'] = H.lib.gca_conv_table_rows(plan.gp, which)
            d['pack'] = plan.pack_elems[which]
            d['layout'] = plan.pack_layout(which)
            d['tail'] = tail_in_force(plan, geom, which, code)
        out[which] = d
    return out


def violations(full_geom, full, geom, small, codes, small_codes, wgrad_exact=True, ragged_boxes=True):
    """Why the launch `small` (describe() of the shrunken plan) is not the launch `full` (of the key's geometry): a list of
    strings, empty when it is."""
    bad = []
    for which, code in codes.items():
        f, s = full[which], small[which]
        name = ('fwd', 'dgrad', 'wgrad')[which]
        if s['kernel'] != f['kernel']:
            bad.append('%s kernel %s != %s' % (name, s['kernel'], f['kernel']))
            continue
        if s['cfg'][:2] != f['cfg'][:2] or s['cfg'][3] != f['cfg'][3]:
            bad.append('%s cfg %r != %r' % (name, s['cfg'], f['cfg']))
        if which == 2:
            tile = f['cfg'][3] & 255
            if wgrad_exact:
                if s['cfg'][2] not in (f['cfg'][2], code.splits):          # the count the key's geometry resolves to, or the cached one
                    bad.append('wgrad splits %d != %d (cached: %d)' % (s['cfg'][2], f['cfg'][2], code.splits))
            else:
                if not (s['cfg'][2] < f['cfg'][2] and (s['cfg'][2] >= 2 or f['cfg'][2] < 2)):
                    bad.append('wgrad splits %d not a clamp of %d' % (s['cfg'][2], f['cfg'][2]))
                if wgrad_last_split_ragged(full_geom, tile, f['cfg'][2]) and not wgrad_last_split_ragged(geom, tile, s['cfg'][2]):
                    bad.append('wgrad last split no longer ragged')
            if tile == 13 and (geom[4] % 4 == 0) != (full_geom[4] % 4 == 0):
                bad.append('wgrad (1,3,3) streaming kernel: W %% 4 changed')
            if s['cfg'][3] >> 11 & 1 and tile <= 10 and geom[4] % 4 != full_geom[4] % 4:
                bad.append('wgrad float4 x path: W %% 4 changed')
            continue
        if s['cfg'][2] != f['cfg'][2]:
            bad.append('%s splits %d != %d' % (name, s['cfg'][2], f['cfg'][2]))
        if (s['rows'], s['pack'], s['layout']) != (f['rows'], f['pack'], f['layout']):
            bad.append('%s classes / taps / packed layout differ' % name)
        if f['cfg'][3] >> 10 & 1 and geom[4] % 4 != full_geom[4] % 4:
            bad.append('%s float4 path: W %% 4 changed' % name)
        if s['tail'][0] != f['tail'][0]:
            bad.append('%s tail rows %d != %d' % (name, s['tail'][0], f['tail'][0]))
        elif f['tail'][0]:
            tiles = -(-first_class_positions(geom, which) // 128)
            if s['tail'][1] != tiles // 2:
                bad.append('%s main_cols %d != %d' % (name, s['tail'][1], tiles // 2))
        kernel = f['kernel']
        if kernel == 'halo':
            if box_of(small_codes[which]) != box_of(code):
                bad.append('%s box differs' % name)
            could, ragged = 0, 0
            for b, q0, q in zip(box_of(code), grid_of(full_geom, which), grid_of(geom, which)):
                if q0 <= b:
                    if q > b:
                        bad.append('%s: an axis that fit one box no longer does' % name)
                elif q <= b or (ragged_boxes and b > 1 and q % b == 0):
                    bad.append('%s: an axis with several boxes lost its second or its ragged box' % name)
                elif b > 1:
                    could, ragged = could + 1, ragged + (q % b != 0)
            if could and not ragged:
                bad.append('%s: no axis ends in a ragged box' % name)
        elif kernel == 'pw':
            sp = geom[2] * geom[3] * geom[4]
            if sp % 8 or sp < 2 * 128 + 8 or sp % 128 == 0:
                bad.append('%s pointwise kernel: %d positions per clip' % (name, sp))
        elif kernel != 'stem':              # (the stem kernel tiles by boxes the library picks from the grid)
            bn, cols = f['cfg'][1], first_class_positions(geom, which)
            if cols < 2 * bn + 1 or cols % bn == 0:
                bad.append('%s: %d columns are not two full tiles of %d and a ragged one' % (name, cols, bn))
    return bad


# ----------------------------------------------------------------------------- the shrunken geometry
def _with_tail(code, geom, which):
    if getattr(code, 'tail', 0) == 0:
        return code
    tiles = -(-first_class_positions(geom, which) // 128)
    return code._replace(tail=(code.tail & 255) | (tiles // 2 << 8))


def _candidates(entry, full, codes):
    """Every (N, D, H, W) of the search window that passes the cheap necessary conditions, as arrays sorted by forward
    multiply-adds, then N, D, H, W: dict(ndhw [n, 4], mac, pos, inside [both budgets], splits [of the weight gradient, as the library
    resolves them], strict [LDS-halo boxes ragged on every axis])."""
    g = entry.geom
    N0, C, D0, H0, W0, K = g[:6]
    k, s, p = g[6:9], g[9:12], g[12:15]
    # (search window: whole clips are only worth trading for positions on small grids)
    nmax, dmax = (N0, D0) if D0 * H0 * W0 < 4096 else (min(N0, 8), min(D0, 16))
    n, d, h, w = np.meshgrid(np.arange(2, nmax + 1), np.arange(1, dmax + 1), np.arange(1, min(H0, 128) + 1),
                             np.arange(1, min(W0, 128) + 1), indexing='ij')
    n, d, h, w = (a.ravel().astype(np.int64) for a in (n, d, h, w))
    od, oh, ow = ((a + 2 * p[i] - k[i]) // s[i] + 1 for i, a in enumerate((d, h, w)))
    ok = (d + 2 * p[0] >= k[0]) & (h + 2 * p[1] >= k[1]) & (w + 2 * p[2] >= k[2])
    ok &= ~((n == N0) & (d == D0) & (h == H0) & (w == W0))
    strict = np.ones_like(ok)
    pos_f = n * od * oh * ow
    pos_d = n * (-(-d // s[0])) * (-(-h // s[1])) * (-(-w // s[2]))
    for which, pos, grid in ((0, pos_f, (od, oh, ow)), (1, pos_d, (d, h, w))):
        if which not in full:
            continue
        f = full[which]
        if f['kernel'] == 'halo':
            for b, q0, q in zip(box_of(codes[which]), grid_of(g, which), grid):
                ok &= (q <= b) if q0 <= b else (q > b)
                if q0 > b and b > 1:
                    strict &= q % b != 0
        elif f['kernel'] == 'pw':
            sp = d * h * w
            ok &= (sp % 8 == 0) & (sp >= 264) & (sp % 128 != 0)
        elif f['kernel'] == 'stem':         # (tiled by boxes the library picks from the grid; it wants >= 8192 outputs)
            ok &= pos >= 8192
        else:
            ok &= (pos >= 2 * f['cfg'][1] + 1) & (pos % f['cfg'][1] != 0)
        if f['cfg'][3] >> 10 & 1:
            ok &= w % 4 == W0 % 4
    splits = np.ones_like(n)                # the split count the library resolves the weight gradient's code to (its own rules)
    if 2 in full:
        tile, want = full[2]['cfg'][3] & 255, max(1, codes[2].splits)
        cdiv = lambda a, b: -(-a // np.maximum(b, 1))
        if tile == 13:
            ok &= (w % 4 == 0) == (W0 % 4 == 0)
            units = n * d * cdiv(w, 16)
            granted = np.maximum(1, np.minimum(want, units // 4))
        elif tile in (11, 12):
            ok &= (h * w) % 16 == 0
            units = n * (h * w // 16)
            granted = np.maximum(1, np.minimum(want, units // 4))
        elif tile == 14:                    # (clip, od) units, the output rows in chunks of >= 8 where those are too few
            base = n * od
            chunks = np.where(want > base, np.minimum(cdiv(want, base), np.maximum(1, oh // 8)), 1)
            units = base * cdiv(oh, cdiv(oh, chunks))
            granted = np.minimum(want, units)
        else:
            units = cdiv(pos_f, 32)
            granted = np.minimum(want, units)
        splits = cdiv(units, cdiv(units, granted))
    mac = pos_f * (K * C * k[0] * k[1] * k[2])
    el = np.maximum(n * C * d * h * w, n * K * od * oh * ow)
    inside = (mac <= MAC_BUDGET) & (el <= ELEM_BUDGET)
    idx = np.nonzero(ok)[0]
    idx = idx[np.lexsort((w[idx], h[idx], d[idx], n[idx], mac[idx]))]
    return dict(ndhw=np.stack((n[idx], d[idx], h[idx], w[idx]), 1), mac=mac[idx], pos=pos_f[idx], inside=inside[idx],
                splits=splits[idx], strict=strict[idx])


def _geom_at(entry, ndhw):
    N, D, H, W = (int(v) for v in ndhw)
    g = list(entry.geom)
    g[0], g[2], g[3], g[4] = N, D, H, W
    if g[15]:
        g[15] = 2 * g[1] * D * H * W                # still the second half of the channels of a batch twice as wide
    return tuple(g)


MAX_PROBES = 2000


@functools.lru_cache(maxsize=None)
def build(entry):
    """-> the Run of `entry`.  Sets and restores the library's arithmetic mode."""
    H = _pkg()._hip
    prev = set_mode(entry)
    try:
        codes = codes_of(entry)
        if runs_as_cached(entry.geom):
            return Run(entry, entry.geom, codes, False, False, False, False)
        full = describe(make_plan(entry.geom, entry.f16, CPU, codes), entry.geom, codes)
        c = _candidates(entry, full, codes)

        def probe(ndhw, wgrad_exact, ragged_boxes):
            geom = _geom_at(entry, ndhw)
            small_codes = {which: _with_tail(code, geom, which) for which, code in codes.items()}
            try:
                plan = make_plan(geom, entry.f16, CPU, small_codes)
            except ValueError:
                return None
            small = describe(plan, geom, small_codes)
            if violations(entry.geom, full, geom, small, codes, small_codes, wgrad_exact, ragged_boxes):
                return None
            return geom, small_codes

        enough = np.isin(c['splits'], (full[2]['cfg'][2], codes[2].splits)) if 2 in full else np.ones_like(c['inside'])
        for ragged in (True, False):            # boxes ragged on every axis; else (no such geometry) on at least one
            boxes = c['strict'] if ragged else ~c['strict']
            for inside in (True, False):        # inside the budgets; else (no such geometry) the cheapest outside them
                for exact in (True, False):     # the full-size split count of the weight gradient; else a clamped one
                    pool = np.nonzero(boxes & (c['inside'] == inside) & (enough | (not exact)))[0]
                    if inside and not exact:    # ... on the most positions the budgets allow
                        pool = pool[np.lexsort((c['mac'][pool], -c['pos'][pool]))]
                    for i in pool[:MAX_PROBES]:
                        hit = probe(c['ndhw'][i], exact, ragged)
                        if hit is not None:
                            return Run(entry, hit[0], hit[1], True, False, not exact, not ragged)
        return Run(entry, entry.geom, codes, False, True, False, False)
    finally:
        H.lib.gca_set_conv_math(prev)


def runs():
    return [build(e) for e in entries()]


# ----------------------------------------------------------------------------- operands and references
def _exact():
    import exact
    return exact


def conv_sums(x, w, s, p, dy, device=CPU):
    """fp64 y, per-channel sum y and sum y^2, dx and dw of a bias-free conv3d, as one matrix product per (kd, kh) tap plane on `device`
    (nothing of the kernels under test; on dyadic operands every sum is exact in fp64, so it equals ATen's bit for bit)."""
    F64 = torch.float64
    x, w, dy = x.to(device, F64), w.to(device, F64), dy.to(device, F64)
    N, C = x.shape[:2]
    K, (kd, kh, kw) = w.shape[0], w.shape[2:]
    OD, OH, OW = dy.shape[2:]
    P = OD * OH * OW
    xp = torch.nn.functional.pad(x, (p[2], p[2], p[1], p[1], p[0], p[0]))
    y = torch.zeros((N, K, P), dtype=F64, device=device)
    dxp, dw = torch.zeros_like(xp), torch.zeros_like(w)
    dyf = dy.reshape(N, K, P)
    dyk = dyf.permute(1, 0, 2).reshape(K, N * P)
    for a in range(kd):
        for b in range(kh):                 # one product per (a, b): the kw taps along W ride in the reduction
            da, hb = slice(a, a + (OD - 1) * s[0] + 1, s[0]), slice(b, b + (OH - 1) * s[1] + 1, s[1])
            xs = xp[:, :, da, hb, :].unfold(4, kw, s[2]).permute(0, 1, 5, 2, 3, 4).reshape(N, C * kw, P)
            wt = w[:, :, a, b, :].reshape(K, C * kw)
            y += torch.matmul(wt, xs)
            dw[:, :, a, b, :] = (dyk @ xs.permute(1, 0, 2).reshape(C * kw, N * P).t()).reshape(K, C, kw)
            g = torch.matmul(wt.t(), dyf).reshape(N, C, kw, OD, OH, OW)
            for c in range(kw):
                dxp[:, :, da, hb, c:c + (OW - 1) * s[2] + 1:s[2]] += g[:, :, c]
    D, H, W = x.shape[2:]
    dx = dxp[:, :, p[0]:p[0] + D, p[1]:p[1] + H, p[2]:p[2] + W].contiguous()
    y = y.reshape(N, K, OD, OH, OW)
    return dict(y=y, sy=y.sum((0, 2, 3, 4)), sq=(y * y).sum((0, 2, 3, 4)), dx=dx, dw=dw)


def conv_ref_abs(x, w, s, p, dy, device=CPU):
    """-> (reference, the same sums over absolute values: y, dx, dw per element; sy = sum |y|, sq = sum y^2 per channel)."""
    ref = conv_sums(x, w, s, p, dy, device)
    a = conv_sums(x.abs(), w.abs(), s, p, dy.abs(), device)
    a['sy'], a['sq'] = ref['y'].abs().sum((0, 2, 3, 4)), ref['sq']
    return ref, a


def shapes(geom):
    N, C, D, H, W, K = geom[:6]
    return (N, C, D, H, W), (K, C) + tuple(geom[6:9]), (N, K) + out_dims(geom)


def _seed(geom, salt):
    import zlib
    return zlib.crc32(repr((tuple(geom[:15]), salt)).encode())


def _moments(m):
    return m * (m + 1) / (2 * m + 1), m * (m + 1) / 3            # E|k|, E k^2 of k uniform on -m..m


def estimate_budgets(geom, name):
    """Expected shares of 2^24 (exact.exact_in_fp32) of the sums of a case on operand set `name`, from the moments of the
    grids: what picks the set.  The real shares are asserted by tests/test_tuned_cases.py."""
    (mx, _), (mw, _), (mdy, _) = _exact().SETS[name]
    (ax, qx), (aw, qw), (ady, _) = _moments(mx), _moments(mw), _moments(mdy)
    ct, taps = geom[1] * geom[6] * geom[7] * geom[8], geom[6] * geom[7] * geom[8]
    pos = geom[0] * int(np.prod(out_dims(geom)))
    return dict(y=1.5 * ct * ax * aw, dx=1.5 * geom[5] * taps * ady * aw, dw=2 * 1.5 * pos * ax * ady,
                sy=pos * (ct * qx * qw) ** 0.5, sq=pos * ct * qx * qw)


def pick_sets(run):
    """-> (the operand set of exact.SETS the case runs on, the set its forward statistics are asserted on).  fp32 storage: the
    widest of MID / NARROW whose sums, the per-channel sum of |y| included, are expected to stay exact in fp32 (deep or long
    reductions end on NARROW), for both.  fp16 storage: ROUND, or WIDE where ROUND's sums are not expected to reach values
    fp16 must round (|y| >= 64 on the 1/32 grid); where the per-channel sum of |y| over the case's positions leaves fp32's
    integer range on those, the statistics are asserted on a second forward, on MID / NARROW."""
    fits = lambda b, keys: max(b[k] for k in keys) < 0.6 * 2.0 ** 24
    narrow = next((n for n in ('MID', 'NARROW') if fits(estimate_budgets(run.geom, n), ('y', 'dx', 'dw', 'sy'))), 'NARROW')
    if not run.entry.f16:
        return narrow, narrow
    (mx, ux), (mw, uw), _ = _exact().SETS['ROUND']
    ct = run.geom[1] * run.geom[6] * run.geom[7] * run.geom[8]
    main = 'ROUND' if 3 * (ct * _moments(mx)[1] * _moments(mw)[1]) ** 0.5 * ux * uw >= 64 else 'WIDE'
    return main, (main if fits(estimate_budgets(run.geom, main), ('sy',)) else narrow)


def dyadic_operands(geom, name):
    """-> x, w, dy (fp64, CPU) on the grids of exact.SETS[name], and the three units."""
    ex = _exact()
    (kx, ux), (kw, uw), (kdy, udy) = ex.SETS[name]
    xs, ws, ys = shapes(geom)
    return (ex.grid(xs, kx, ux, _seed(geom, 1)), ex.grid(ws, kw, uw, _seed(geom, 2)), ex.grid(ys, kdy, udy, _seed(geom, 3))), (ux, uw, udy)


def float_operands(geom, f16):
    """randn x and dy, He-scaled randn weights (fp64, CPU); rounded to fp16 numbers for the fp16-storage path, whose products
    are then exact in fp32."""
    xs, ws, ys = shapes(geom)
    g = torch.Generator().manual_seed(_seed(geom, 4))
    x = torch.randn(xs, generator=g)
    w = torch.randn(ws, generator=g) * (2.0 / (ws[1] * ws[2] * ws[3] * ws[4])) ** 0.5
    dy = torch.randn(ys, generator=g)
    if f16:
        x, w, dy = x.half(), w.half(), dy.half()
    return x.double(), w.double(), dy.double()


def budgets(a, units):
    """Shares of 2^24 of the absolute sums `a` (conv_ref_abs) of dyadic operands with `units` = (ux, uw, udy)."""
    ex = _exact()
    ux, uw, udy = units
    return dict(y=ex.exact_in_fp32(a['y'], ux * uw), dx=ex.exact_in_fp32(a['dx'], udy * uw), dw=ex.exact_in_fp32(a['dw'], ux * udy),
                sy=ex.exact_in_fp32(a['sy'], ux * uw), sq=ex.exact_in_fp32(a['sq'], (ux * uw) ** 2))


@functools.lru_cache(maxsize=3)
def dyadic_case(geom, name, device=CPU):
    """-> dict(x, w, dy [CPU fp64], ref, abs [on `device`], units, budgets) of geometry `geom` on operand set `name`; shared by
    the arithmetic prefixes that run the geometry."""
    (x, w, dy), units = dyadic_operands(geom, name)
    ref, a = conv_ref_abs(x, w, geom[9:12], geom[12:15], dy, device)
    return dict(x=x, w=w, dy=dy, ref=ref, abs=a, units=units, budgets=budgets(a, units))


@functools.lru_cache(maxsize=3)
def float_case(geom, f16, device=CPU):
    x, w, dy = float_operands(geom, f16)
    ref, a = conv_ref_abs(x, w, geom[9:12], geom[12:15], dy, device)
    return dict(x=x, w=w, dy=dy, ref=ref, abs=a)
