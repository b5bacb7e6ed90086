"""Specification of the device-side contrastive augmentations (gca_clip_augment), in numpy.  Test infrastructure.

What it restates.  The reference's contrastive chain (build_video_contrast_transform_cv2, lib/data/transform/build.py:45-62):
VideoRandomResizedCrop -> VideoRandomApply(VideoRandomColorJitter, 0.8) -> VideoRandomGrayScale(0.2) ->
VideoRandomApply(VideoGaussianBlur, 0.5) -> VideoRandomHorizontalFlip -> VideoNormalize -> VideoToTensor
(consistency_transforms.py:81-145, 226-340).  Those classes call cv2 / albumentations, which are installed neither where
this suite runs nor where the kernels run: NOTHING here is checked against cv2, and no bit parity with cv2 is claimed.  This
file fixes the arithmetic instead, and the kernels are held to it bit for bit.  Three rules:

  1. every stage maps uint8 -> uint8, as the reference's chain does;
  2. every stage is integer / fixed-point arithmetic, or np.float32 with exactly one rounding per written operation;
  3. whatever needs exp, log, a floating division or double precision is computed by the HOST and shipped as data
     (``pack``): resize taps, the brightness and hue look-up tables, 1 - factor, the blur weights, the HSV division tables.

Where the published definitions of the third-party calls leave the internals open, this file decides; every such place is
marked DECIDED.

Layout of what the host ships for one (clip, view), shared by its T frames:

  record  int32[24]   0 y0  1 x0  2 ch  3 cw          crop box inside the (Hs, Ws) source frame
                      4 flip  5 gray  6 k             k in {0, 3, 5, 7}; 0 = no blur
                      7..10 perm                      the order of the four jitter ops: 0 brightness 1 contrast
                                                      2 saturation 3 hue
                      11 mask                         bit op set = the op is applied (0 = no jitter; an op with factor 1,
                                                      or hue 0, is the identity BY DEFINITION and has its bit clear)
                      12 f_c  13 1 - f_c  14 f_s  15 1 - f_s      contrast / saturation factors, float32 bit patterns
                      16..22 blur weights             k taps, fixed point, sum == 1 << BLUR_SHIFT; the rest 0
                      23 0
  taps    int16[H + W][4]   (i0, i1, c0, c1): source row (first H entries) / column (last W) indices in FRAME coordinates,
                            already clamped to the crop box, and their 11-bit weights, c0 + c1 == 1 << TAP_SHIFT
  luts    uint8[2][256]     brightness table, hue table (H in [0, 180) -> shifted H)
and once for all records: divtab int32[2][256], the saturation / hue division tables of the 8-bit RGB -> HSV conversion.
"""
import math

import numpy as np
import torch

from oracle import input as oinput

REC = 24
TAP_SHIFT = 11            # bilinear coefficients: 11 bits, as cv2's INTER_RESIZE_COEF_BITS
BLUR_SHIFT = 12           # DECIDED: blur weights in 12-bit fixed point
HSV_SHIFT = 12            # cv2's hsv_shift
OPS = ('brightness', 'contrast', 'saturation', 'hue')
F32 = np.float32


def _bits(x):
    return int(np.array(x, dtype=np.float32).view(np.int32))


def _f32_of(bits):
    return np.array(bits, dtype=np.int32).view(np.float32)[()]


# ------------------------------------------------------------------------------------------------ host-computed data
def resize_taps(origin, crop, out, frame):
    """(out, 4) int16 {i0, i1, c0, c1} for one axis: `crop` source samples starting at `origin` -> `out` samples, half-pixel
    centres (INTER_LINEAR's map: src = (dst + 0.5) * crop / out - 0.5), indices clamped to the crop box.
    DECIDED: the map is evaluated in float64 and the fraction rounded to 11 bits with rint (cv2 evaluates it in float)."""
    assert 0 <= origin and crop >= 1 and origin + crop <= frame
    d = np.arange(out, dtype=np.float64)
    f = (d + 0.5) * (float(crop) / float(out)) - 0.5
    s = np.floor(f)
    a = f - s
    a[s < 0] = 0.0
    s[s < 0] = 0
    a[s >= crop - 1] = 0.0
    s[s >= crop - 1] = crop - 1
    c1 = np.rint(a * (1 << TAP_SHIFT)).astype(np.int64)
    i0 = s.astype(np.int64)
    i1 = np.minimum(i0 + 1, crop - 1)
    return np.stack([origin + i0, origin + i1, (1 << TAP_SHIFT) - c1, c1], axis=1).astype(np.int16)


def brightness_lut(factor):
    """albumentations' uint8 branch of adjust_brightness_torchvision: clip(arange(256) * factor, 0, 255).astype(uint8)."""
    return np.clip(np.arange(256, dtype=np.float64) * float(factor), 0, 255).astype(np.uint8)


def hue_lut(factor):
    """albumentations' uint8 branch of adjust_hue_torchvision: mod(arange(256) + 180 * factor, 180).astype(uint8)."""
    return np.mod(np.arange(256, dtype=np.int16) + 180.0 * float(factor), 180).astype(np.uint8)


def blur_weights(k, sigma):
    """k Gaussian taps in BLUR_SHIFT fixed point.  DECIDED: exp(-x^2 / (2 sigma^2)) in float64, normalised, rounded half up;
    what the rounding leaves over goes to the centre tap, so the taps sum to 1 << BLUR_SHIFT exactly."""
    assert k in (3, 5, 7) and sigma > 0
    x = np.arange(k, dtype=np.float64) - (k - 1) / 2.0
    w = np.exp(-(x * x) / (2.0 * float(sigma) * float(sigma)))
    w /= w.sum()
    q = np.floor(w * (1 << BLUR_SHIFT) + 0.5).astype(np.int64)
    q[k // 2] += (1 << BLUR_SHIFT) - q.sum()
    assert q.min() >= 0 and q.sum() == 1 << BLUR_SHIFT
    return q.astype(np.int32)


def hsv_div_tables():
    """(2, 256) int32: sdiv[i] = round((255 << 12) / i), hdiv[i] = round((180 << 12) / (6 i)), entry 0 = 0 (cv2's
    sdiv_table / hdiv_table180)."""
    t = np.zeros((2, 256), dtype=np.int32)
    i = np.arange(1, 256, dtype=np.float64)
    t[0, 1:] = np.rint((255 << HSV_SHIFT) / i).astype(np.int32)
    t[1, 1:] = np.rint((180 << HSV_SHIFT) / (6.0 * i)).astype(np.int32)
    return t


def identity_params(y0, x0, H, W, flip=0):
    return dict(y0=y0, x0=x0, ch=H, cw=W, jitter=False, perm=(0, 1, 2, 3), brightness=1.0, contrast=1.0, saturation=1.0,
                hue=0.0, gray=False, k=0, sigma=0.0, flip=bool(flip))


def check_params(p, Hs, Ws, H, W):
    if p['ch'] < 1 or p['cw'] < 1 or p['y0'] < 0 or p['x0'] < 0 or p['y0'] + p['ch'] > Hs or p['x0'] + p['cw'] > Ws:
        raise ValueError('crop box outside the source frame')
    if p['k'] not in (0, 3, 5, 7):
        raise ValueError('blur size must be 0, 3, 5 or 7')
    if p['k'] // 2 >= min(H, W):
        raise ValueError('blur radius does not fit the output (reflect-101 needs radius < size)')
    if sorted(p['perm']) != [0, 1, 2, 3]:
        raise ValueError('perm is not a permutation of the four jitter ops')


def pack(params, Hs, Ws, H, W):
    """params: b lists of `views` dicts (see identity_params) -> (records (b, views, 24) int32, taps (b, views, H + W, 4)
    int16, luts (b, views, 2, 256) uint8)."""
    b, views = len(params), len(params[0])
    rec = np.zeros((b, views, REC), dtype=np.int32)
    taps = np.zeros((b, views, H + W, 4), dtype=np.int16)
    luts = np.zeros((b, views, 2, 256), dtype=np.uint8)
    for n in range(b):
        for v in range(views):
            p = params[n][v]
            check_params(p, Hs, Ws, H, W)
            r = rec[n, v]
            r[0:7] = (p['y0'], p['x0'], p['ch'], p['cw'], int(bool(p['flip'])), int(bool(p['gray'])), p['k'])
            r[7:11] = p['perm']
            fc, fs = F32(p['contrast']), F32(p['saturation'])
            mask = 0
            if p['jitter']:
                mask = ((p['brightness'] != 1.0) << 0 | (fc != F32(1)) << 1 | (fs != F32(1)) << 2 | (p['hue'] != 0.0) << 3)
            r[11] = mask
            r[12], r[13], r[14], r[15] = _bits(fc), _bits(F32(1) - fc), _bits(fs), _bits(F32(1) - fs)
            if p['k']:
                r[16:16 + p['k']] = blur_weights(p['k'], p['sigma'])
            taps[n, v, :H] = resize_taps(p['y0'], p['ch'], H, Hs)
            taps[n, v, H:] = resize_taps(p['x0'], p['cw'], W, Ws)
            luts[n, v, 0] = brightness_lut(p['brightness'] if p['jitter'] else 1.0)
            luts[n, v, 1] = hue_lut(p['hue'] if p['jitter'] else 0.0)
    return rec, taps, luts


# ------------------------------------------------------------------------------------------------ the stages (uint8 -> uint8)
def resize(img, ty, tx):
    """img (Hs, Ws, 3) uint8, ty (H, 4) / tx (W, 4) taps -> (H, W, 3) uint8.  Horizontal blend, vertical blend, ONE rounding
    shift.  DECIDED: cv2 rounds between its two passes (its intermediate is narrowed); here all 22 fraction bits are kept,
    2048 * 2048 * 255 + 2^21 < 2^31."""
    ty, tx = ty.astype(np.int64), tx.astype(np.int64)
    a = img.astype(np.int64)
    top, bot = a[ty[:, 0]], a[ty[:, 1]]                                   # (H, Ws, 3)
    c0, c1 = tx[None, :, 2, None], tx[None, :, 3, None]
    ht = c0 * top[:, tx[:, 0]] + c1 * top[:, tx[:, 1]]                   # (H, W, 3)
    hb = c0 * bot[:, tx[:, 0]] + c1 * bot[:, tx[:, 1]]
    v = ty[:, 2, None, None] * ht + ty[:, 3, None, None] * hb
    return ((v + (1 << (2 * TAP_SHIFT - 1))) >> (2 * TAP_SHIFT)).astype(np.uint8)


def gray_of(img):
    """cv2's 8-bit RGB2GRAY: (4899 R + 9617 G + 1868 B + 8192) >> 14 -> (H, W) int32."""
    a = img.astype(np.int32)
    return (4899 * a[..., 0] + 9617 * a[..., 1] + 1868 * a[..., 2] + 8192) >> 14


def to_gray(img):
    g = gray_of(img).astype(np.uint8)
    return np.stack([g, g, g], axis=-1)


def adjust_brightness(img, lut):
    return lut[img]


def adjust_contrast(img, f, omf):
    """lut = arange(256) * f + mean * (1 - f), clipped, truncated (albumentations' uint8 branch), mean = the frame's mean
    gray.  fp32, in this order: mean = f32(sum) * f32(1 / n); off = mean * (1 - f); y = f32(v) * f; z = y + off.
    DECIDED: the mean is the exact integer sum times the fp32 reciprocal of the pixel count (albumentations takes a float64
    mean); the general formula also serves f = 0 (albumentations special-cases it)."""
    g = gray_of(img)
    inv_n = F32(1) / F32(g.size)
    mean = F32(int(g.sum(dtype=np.int64))) * inv_n
    off = F32(mean * F32(omf))
    z = img.astype(F32) * F32(f) + off
    return np.minimum(np.maximum(z, F32(0)), F32(255)).astype(np.uint8)


def adjust_saturation(img, f, omf):
    """cv2.addWeighted(img, f, gray, 1 - f, 0) on uint8.  fp32: y = f32(v) * f; g = f32(gray) * (1 - f); z = y + g; round half
    to even, clamp.  DECIDED: that evaluation order and precision."""
    g = gray_of(img).astype(F32) * F32(omf)
    z = img.astype(F32) * F32(f) + g[..., None]
    return np.minimum(np.maximum(np.rint(z), F32(0)), F32(255)).astype(np.uint8)


def rgb_to_hsv(img, divtab):
    """cv2's 8-bit RGB2HSV with H in [0, 180): integer, with the two division tables."""
    a = img.astype(np.int32)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    s = (diff * divtab[0][v] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * divtab[1][diff] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT         # arithmetic shift: floor for negative h
    h = np.where(h < 0, h + 180, h)
    return h, s, v


def hsv_to_rgb(h, s, v):
    """DECIDED: an integer inverse (cv2 converts back through float): sector = h // 30, f = h % 30,
    p = v (255 - s) / 255, q = v (7650 - s f) / 7650, t = v (7650 - s (30 - f)) / 7650, each rounded to nearest by adding
    half the divisor before an integer division by a constant."""
    sec = h // 30
    f = h - 30 * sec
    p = (v * (255 - s) + 127) // 255
    q = (v * (7650 - s * f) + 3825) // 7650
    t = (v * (7650 - s * (30 - f)) + 3825) // 7650
    r = np.select([sec == 0, sec == 1, sec == 2, sec == 3, sec == 4], [v, q, p, p, t], v)
    g = np.select([sec == 0, sec == 1, sec == 2, sec == 3, sec == 4], [t, v, v, q, p], p)
    b = np.select([sec == 0, sec == 1, sec == 2, sec == 3, sec == 4], [p, p, t, v, v], q)
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


def adjust_hue(img, lut, divtab):
    h, s, v = rgb_to_hsv(img, divtab)
    return hsv_to_rgb(lut[h].astype(np.int32), s, v)


def gaussian_blur(img, w):
    """Separable, reflect-101 border, horizontal pass then vertical pass, each rounded once to uint8:
    (sum_i w_i p_i + half) >> BLUR_SHIFT.  DECIDED: the intermediate is uint8 (cv2 keeps 16 bits between its passes)."""
    k = len(w)
    r = k // 2
    w = w.astype(np.int64)
    half = 1 << (BLUR_SHIFT - 1)
    a = np.pad(img.astype(np.int64), ((0, 0), (r, r), (0, 0)), mode='reflect')
    a = (sum(w[i] * a[:, i:i + img.shape[1]] for i in range(k)) + half) >> BLUR_SHIFT
    a = np.pad(a, ((r, r), (0, 0), (0, 0)), mode='reflect')
    a = (sum(w[i] * a[i:i + img.shape[0]] for i in range(k)) + half) >> BLUR_SHIFT
    return a.astype(np.uint8)


def augment_frame(img, rec, taps, luts, divtab, H, W):
    """One (Hs, Ws, 3) uint8 frame -> (H, W, 3) uint8, everything up to and including the blur (the flip is an index map and
    lives with normalise / to-tensor in augment_batch)."""
    x = resize(img, taps[:H], taps[H:])
    for op in rec[7:11]:
        if not (rec[11] >> op) & 1:
            continue
        if op == 0:
            x = adjust_brightness(x, luts[0])
        elif op == 1:
            x = adjust_contrast(x, _f32_of(rec[12]), _f32_of(rec[13]))
        elif op == 2:
            x = adjust_saturation(x, _f32_of(rec[14]), _f32_of(rec[15]))
        else:
            x = adjust_hue(x, luts[1], divtab)
    if rec[5]:
        x = to_gray(x)
    if rec[6]:
        x = gaussian_blur(x, rec[16:16 + rec[6]])
    return x


def augment_batch(frames, packed, H, W, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """frames (b, views, T, Hs, Ws, 3) uint8, packed = pack(...) -> (b, 3 * views, T, H, W) float32 torch tensor: the frames
    through augment_frame, then flip / VideoNormalize / VideoToTensor / view concatenation exactly as oracle.input does them."""
    rec, taps, luts = packed
    divtab = hsv_div_tables()
    b, views, T = frames.shape[:3]
    aug = np.empty((b, views, T, H, W, 3), dtype=np.uint8)
    for n in range(b):
        for v in range(views):
            for t in range(T):
                aug[n, v, t] = augment_frame(frames[n, v, t], rec[n, v], taps[n, v], luts[n, v], divtab, H, W)
    flips = np.zeros((b, views, 3), dtype=np.int64)
    flips[..., 2] = rec[..., 4]
    return oinput.make_batch(aug, flips, H, W, mean, std)


# ------------------------------------------------------------------------------------------------ the sampler
def sample_params(Hs, Ws, rnd, nprnd, scale=(0.2, 1.0), ratio=(0.75, 1.3333333333333333), brightness=0.4, contrast=0.4,
                  saturation=0.4, hue=0.1, p_jitter=0.8, p_gray=0.2, p_blur=0.5, blur_limit=(3, 7), sigma_limit=(0.1, 2.0),
                  p_flip=0.5):
    """One (clip, view): the draws of the reference's chain, in its order, from `rnd` (a random.Random: the reference uses the
    `random` module) and `nprnd` (a np.random.RandomState: VideoGaussianBlur.get_params draws the size from np.random)."""
    # VideoRandomResizedCrop.get_params (:95-134)
    area = Hs * Ws
    for _attempt in range(10):
        target_area = rnd.uniform(*scale) * area
        log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
        aspect_ratio = math.exp(rnd.uniform(*log_ratio))
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= Ws and 0 < h <= Hs:
            i = rnd.randint(0, Hs - h)
            j = rnd.randint(0, Ws - w)
            break
    else:
        in_ratio = Ws / Hs
        if in_ratio < min(ratio):
            w = Ws
            h = int(round(w / min(ratio)))
        elif in_ratio > max(ratio):
            h = Hs
            w = int(round(h * max(ratio)))
        else:
            w, h = Ws, Hs
        i = (Hs - h) // 2
        j = (Ws - w) // 2
    h_start = i * 1.0 / (Hs - h + 1e-10)
    w_start = j * 1.0 / (Ws - w + 1e-10)
    y0, x0 = oinput.random_crop_coords(Hs, Ws, h, w, h_start, w_start)     # F.random_crop's origin (may land on i - 1)
    p = dict(y0=y0, x0=x0, ch=h, cw=w, jitter=False, perm=(0, 1, 2, 3), brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0,
             gray=False, k=0, sigma=0.0, flip=False)
    # VideoRandomApply(VideoRandomColorJitter, p) (:70-79, 316-330)
    if rnd.random() < p_jitter:
        p['jitter'] = True
        p['brightness'] = rnd.uniform(max(0, 1 - brightness), 1 + brightness)
        p['contrast'] = rnd.uniform(max(0, 1 - contrast), 1 + contrast)
        p['saturation'] = rnd.uniform(max(0, 1 - saturation), 1 + saturation)
        p['hue'] = rnd.uniform(-hue, hue)
        order = [0, 1, 2, 3]
        rnd.shuffle(order)
        p['perm'] = tuple(order)
    # VideoRandomGrayScale (:269-273)
    p['gray'] = rnd.random() < p_gray
    # VideoRandomApply(VideoGaussianBlur, p) (:251-256)
    if rnd.random() < p_blur:
        ksize = int(nprnd.randint(blur_limit[0], blur_limit[1] + 1))
        if ksize != 0 and ksize % 2 != 1:
            ksize = (ksize + 1) % (blur_limit[1] + 1)
        p['k'] = ksize
        p['sigma'] = rnd.uniform(*sigma_limit)
    # VideoRandomHorizontalFlip (:355-364)
    p['flip'] = rnd.random() < p_flip
    return p


def sample_batch(b, views, Hs, Ws, rnd, nprnd, **kw):
    return [[sample_params(Hs, Ws, rnd, nprnd, **kw) for _ in range(views)] for _ in range(b)]
