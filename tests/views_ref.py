"""Specification of the downstream (action-recognition) views kernel gca_clip_views, in numpy.  Test infrastructure.

What it restates.  The reference's host transforms for fine-tuning and for the video-level test:

  training  VideoMultiScaleCrop(BASE_SIZE, [1, .875, .75, .66]) -> VideoRandomHorizontalFlip -> VideoNormalize -> VideoToTensor
            (build_transform_cv2(is_train=True), lib/data/transform/build.py:27-35; consistency_transforms.py:351-468)
  testing   VideoResize(scale_size) -> VideoCenterCrop | VideoFullResSample (3 crops) | VideoOverSampleCrop (5 crops, 10 with
            flips) -> VideoNormalize -> VideoToTensor  (tools/test_ds.py:95-120; consistency_transforms.py:159-170, 341-349,
            470-551)

The rules are those of tests/augment_ref.py: integer / fixed-point arithmetic or np.float32 with one rounding per written
operation, and whatever needs a floating division is computed on the host and shipped as data.  The resize taps, the resize
itself and the normalise step are NOT restated here: they are augment_ref.resize_taps, augment_ref.resize and oracle.input.
As there, nothing is checked against cv2 (F.resize is cv2.resize), and no bit parity with cv2 is claimed.

What IS pinned to the reference (tests/golden/views.npz, written by tests/golden/make_golden_views.py from the reference's
own classes): the crop pairs, the fix-offset lists, the sampled (crop, offset) traces and flip decisions, and the origins,
truncation and output order of the 3-crop and the 5-crop layouts.  The flipped half of the 10-crop layout is restated from
the source (:491-506: per offset, the unflipped frames, then the flipped ones) and is NOT pinned: with flip=True the
reference calls albumentations' hflip, which is not installed.

Data model of one batch:

  frames   (n_src, F, Hs, Ws, 3) uint8   one decoded source per video; F = T for training, test_clips * T for testing
  taps     (n_tab, Lh + Lw, 4) int16     {i0, i1, c0, c1}: Lh row taps, then Lw column taps; indices in source-frame
                                         coordinates, c0 + c1 == 2048
  records  (n_views, 8) int32            {src, t0, tab, oy, ox, flip, 0, 0}
  out      (n_views, 3, T, H, W) fp32    pixel (y, x) of frame t samples frames[src, t0 + t] through the row tap
                                         taps[tab, oy + y] and the column tap taps[tab, Lh + ox + (W - 1 - x if flip else x)];
                                         two-pass blend with one rounding shift to uint8, then (float(px) - mean255_c) *
                                         inv_std255_c

Training: n_tab = n_src, Lh = H, Lw = W, oy = ox = 0, one view per clip, the taps map the clip's crop box onto the output.
Testing: n_tab = 1, (Lh, Lw) = scale_size, (oy, ox) the crop origin inside the resized frame -- a crop of a resized uint8 frame
is a window of its taps (test_views_ref.py checks exactly that sentence).
"""
import numpy as np
import torch

import augment_ref as ar
from oracle import input as oinput

REC = 8
SCALES = (1, .875, .75, .66)


def _pair(size):
    return (int(size), int(size)) if isinstance(size, (int, np.integer)) else (int(size[0]), int(size[1]))


# ------------------------------------------------------------------------------------------------ parameter generators
def multiscale_pairs(img_h, img_w, input_size, scales=SCALES, max_distort=1):
    """The (crop_w, crop_h) candidates of VideoMultiScaleCrop._sample_crop_size (:406-424), in its order.  input_size: an int
    or the two-entry list the class keeps.  NOTE which entry each axis is compared with: the reference snaps crop_h to
    input_size[1] and crop_w to input_size[0], yet resizes to input_size[0] rows by input_size[1] columns (:400).  Restated
    literally; every config uses square sizes, where it makes no difference."""
    input_size = _pair(input_size)
    base_size = min(img_w, img_h)
    crop_sizes = [int(base_size * x) for x in scales]
    crop_h = [input_size[1] if abs(x - input_size[1]) < 3 else x for x in crop_sizes]
    crop_w = [input_size[0] if abs(x - input_size[0]) < 3 else x for x in crop_sizes]
    pairs = []
    for i, h in enumerate(crop_h):
        for j, w in enumerate(crop_w):
            if abs(i - j) <= max_distort:
                pairs.append((w, h))
    return pairs


def fix_offsets(more_fix_crop, image_w, image_h, crop_w, crop_h):
    """VideoMultiScaleCrop.fill_fix_offset (:446-468): (w_offset, h_offset) FLOATS; their users truncate with int()."""
    w_step = (image_w - crop_w) / 4
    h_step = (image_h - crop_h) / 4
    ret = [(0, 0), (4 * w_step, 0), (0, 4 * h_step), (4 * w_step, 4 * h_step), (2 * w_step, 2 * h_step)]
    if more_fix_crop:
        ret += [(0, 2 * h_step), (4 * w_step, 2 * h_step), (2 * w_step, 4 * h_step), (2 * w_step, 0 * h_step),
                (1 * w_step, 1 * h_step), (3 * w_step, 1 * h_step), (1 * w_step, 3 * h_step), (3 * w_step, 3 * h_step)]
    return ret


def sample_train(Hs, Ws, input_size, nprnd, rnd, scales=SCALES, max_distort=1, fix_crop=True, more_fix_crop=True, p_flip=0.5):
    """One training clip: the draws of VideoMultiScaleCrop._sample_crop_size (:426-436) and VideoRandomHorizontalFlip
    (:355-356), in the reference's order: nprnd.randint(len(pairs)); nprnd.randint(len(offsets)) -- or, with fix_crop off, the
    two randint(0, img - crop) draws, width first --; rnd.random() < p for the flip.  nprnd: a np.random.RandomState (the
    reference draws from np.random), rnd: a random.Random (the reference's `random` module).
    -> dict(y0, x0, ch, cw, flip): the crop box inside the source frame and the flip."""
    pairs = multiscale_pairs(Hs, Ws, input_size, scales, max_distort)
    cw, ch = pairs[nprnd.randint(len(pairs))]
    if not fix_crop:
        w_offset = nprnd.randint(0, Ws - cw)
        h_offset = nprnd.randint(0, Hs - ch)
    else:
        offsets = fix_offsets(more_fix_crop, Ws, Hs, cw, ch)
        w_offset, h_offset = offsets[nprnd.randint(len(offsets))]
    flip = rnd.random() < p_flip
    return dict(y0=int(h_offset), x0=int(w_offset), ch=int(ch), cw=int(cw), flip=bool(flip))


def check_box(p, Hs, Ws):
    if p['ch'] < 1 or p['cw'] < 1 or p['y0'] < 0 or p['x0'] < 0 or p['y0'] + p['ch'] > Hs or p['x0'] + p['cw'] > Ws:
        raise ValueError('crop box outside the source frame')


def pack_train(params, Hs, Ws, H, W):
    """b dicts (sample_train) -> (records (b, 8) int32, taps (b, H + W, 4) int16): clip n is view n, reads source n from
    frame 0 through its own table, whose taps map the crop box onto the (H, W) output (F.resize(img, H, W), :400)."""
    b = len(params)
    rec = np.zeros((b, REC), dtype=np.int32)
    taps = np.zeros((b, H + W, 4), dtype=np.int16)
    for n, p in enumerate(params):
        check_box(p, Hs, Ws)
        rec[n, :6] = (n, 0, n, 0, 0, int(bool(p['flip'])))
        taps[n, :H] = ar.resize_taps(p['y0'], p['ch'], H, Hs)
        taps[n, H:] = ar.resize_taps(p['x0'], p['cw'], W, Ws)
    return rec, taps


def crop_origins(Hr, Wr, H, W, test_crops):
    """-> ([(oy, ox), ...] in the reference's order, (flips per origin)) inside an (Hr, Wr) frame, the cases of
    tools/test_ds.py:96-114."""
    if test_crops == 1:
        # VideoCenterCrop -> albumentations' center_crop.  DECIDED: origin ((Hr - H) // 2, (Wr - W) // 2), the published
        # get_center_crop_coords; albumentations is not installed to compare with
        return [((Hr - H) // 2, (Wr - W) // 2)], (0,)
    if test_crops == 3:
        # VideoFullResSample(flip=False), :528-534: integer steps
        w_step = (Wr - W) // 4
        h_step = (Hr - H) // 4
        offsets = [(0 * w_step, 2 * h_step), (4 * w_step, 2 * h_step), (2 * w_step, 2 * h_step)]
        return [(int(oh), int(ow)) for ow, oh in offsets], (0,)
    if test_crops in (5, 10):
        # VideoOverSampleCrop, :489-495: float steps, truncated by int() where the frame is sliced
        offsets = fix_offsets(False, Wr, Hr, W, H)
        return [(int(oh), int(ow)) for ow, oh in offsets], ((0,) if test_crops == 5 else (0, 1))
    raise ValueError('only 1, 3, 5 and 10 test crops are supported, got %r' % (test_crops,))


def test_layout(Hs, Ws, scale_size, crop_size, test_crops, test_clips, T):
    """The views of ONE video -> (records (views, 8) int32 with src = 0, taps (1, Hr + Wr, 4) int16).  scale_size: an int
    (VideoResize's square) or (Hr, Wr); crop_size: an int or (H, W).  View order: offset-major, then unflipped before flipped,
    then temporal clip -- the order in which :491-506 emits the frames of a test_clips * T frame list."""
    (Hr, Wr), (H, W) = _pair(scale_size), _pair(crop_size)
    origins, flips = crop_origins(Hr, Wr, H, W, test_crops)
    if H < 1 or W < 1 or H > Hr or W > Wr or test_clips < 1 or T < 1:
        raise ValueError('crop %r does not fit the resized frame %r' % ((H, W), (Hr, Wr)))
    taps = np.concatenate([ar.resize_taps(0, Hs, Hr, Hs), ar.resize_taps(0, Ws, Wr, Ws)])[None]
    rec = [(0, clip * T, 0, oy, ox, flip, 0, 0) for (oy, ox) in origins for flip in flips for clip in range(test_clips)]
    return np.array(rec, dtype=np.int32), taps


test_layout.__test__ = False          # (an importer's pytest must not collect it)


def tile_videos(rec, n_src):
    """The records of one video (src = 0) -> those of n_src videos, video-major: (n_src * views, 8)."""
    out = np.tile(rec, (n_src, 1))
    out[:, 0] = np.repeat(np.arange(n_src, dtype=np.int32), len(rec))
    return out


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic
def clip_views(frames, records, taps, Lh, Lw, T, H, W, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """-> (n_views, 3, T, H, W) float32 torch tensor, by the data model of the module docstring."""
    n_src, F, Hs, Ws = frames.shape[:4]
    assert frames.dtype == np.uint8 and taps.shape[1:] == (Lh + Lw, 4) and records.shape[1:] == (REC,)
    out = []
    for src, t0, tab, oy, ox, flip in records[:, :6]:
        assert 0 <= src < n_src and 0 <= tab < len(taps) and 0 <= t0 and t0 + T <= F and flip in (0, 1)
        assert 0 <= oy and oy + H <= Lh and 0 <= ox and ox + W <= Lw
        ty = taps[tab, oy:oy + H]
        tx = taps[tab, Lh + ox:Lh + ox + W]
        assert ty[:, :2].min() >= 0 and ty[:, :2].max() < Hs and tx[:, :2].min() >= 0 and tx[:, :2].max() < Ws
        if flip:
            tx = tx[::-1]                                          # column x looks up tap W - 1 - x
        out.append(oinput.video_to_tensor([oinput.video_normalize(ar.resize(frames[src, t0 + t], ty, tx), mean, std)
                                           for t in range(T)]))
    return torch.stack(out) if out else torch.zeros((0, 3, T, H, W))
