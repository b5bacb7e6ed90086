"""Device-side input stage: uint8 frames in, normalised (b, 6, T, H, W) clips out, H2D overlapped with the step.

The reference decodes and augments on the host and copies the finished fp32 batch to the GPU inside the iteration
(tools/train_video_contrast_dis.py:402, 154 MB per 32-clip batch).  At ~21 ms per iteration that copy is worth 15 % of a
step.  Here the host keeps what only it can do (JPEG decode, resize, colour jitter, blur: cv2 / albumentations work,
lib/data/transform/build.py:45-62) and hands over uint8 frames + one (crop origin, flip) record per clip view; the rest --
crop, horizontal flip, VideoNormalize, VideoToTensor, the concatenation of the two views
(lib/data/datasets/video_contrast_dataset.py:196-203) -- is ONE kernel pass (gca_clip_prepare) writing straight into the
trainer's static input buffer.

Pipelining: two pinned host buffers and two device buffers; ``stage()`` copies batch t+1 on a copy stream while the
captured step of batch t runs; ``prepare()`` makes the compute stream wait for that copy (an event, no host sync) and
launches the kernel.  A slot is reused only after the kernel that read it has been issued and its event has passed.

Second, opt-in mode (``DeviceInputStage(..., augment=True)``, ``clip_augment``): the host stops after DECODE and hands over the
source frames (e.g. 128 x 171) + one sampled parameter record per (clip, view); the whole contrastive chain of
build_video_contrast_transform_cv2 (random resized crop, colour jitter, grayscale, Gaussian blur, flip, normalise) runs in
gca_clip_augment.  The host still computes everything that needs exp / log / a floating division (``pack_augment``: resize
taps, look-up tables, blur weights) -- a few KB per clip.  The arithmetic is the one tests/augment_ref.py writes down; cv2 and
albumentations are not available to compare with, so parity with cv2's own rounding is unverified.
"""
import math

import numpy as np
import torch

from . import ops
from .. import _hip as H


def normalize_constants(mean, std, max_pixel_value=255.0):
    """(mean*255, 1/(std*255)) in fp32, rounded where VideoNormalize.normalize rounds (consistency_transforms.py:54-60)."""
    m = np.array(mean, dtype=np.float32)
    m *= max_pixel_value
    s = np.array(std, dtype=np.float32)
    s *= max_pixel_value
    return m, np.reciprocal(s, dtype=np.float32)


def crop_coords(height, width, crop_height, crop_width, h_start, w_start):
    """albumentations' get_random_crop_coords, as F.random_crop(img, h, w, h_start, w_start) uses it (VideoRandomCrop,
    the crop step of VideoRandomResizedCrop): fractions in [0, 1) -> integer origin."""
    return int((height - crop_height) * h_start), int((width - crop_width) * w_start)


def clip_prepare(frames, params, mean255, inv_std255, H_out, W_out, out=None, out_dtype=torch.float32):
    """frames (b, views, T, Hs, Ws, 3) uint8 device tensor, params (b, views, 4) int32 device tensor {h0, w0, flip, 0}
    -> (b, 3*views, T, H_out, W_out) fp32 | fp16.  `out`: optional preallocated result (the trainer's static batch)."""
    if frames.dtype is not torch.uint8 or frames.dim() != 6 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise ValueError('frames must be a contiguous (b, views, T, Hs, Ws, 3) uint8 tensor')
    if not frames.is_cuda:
        raise RuntimeError('clip_prepare needs the frames on the GPU (there is no CPU fallback)')
    b, views, T, Hs, Ws, _ = frames.shape
    if params.dtype is not torch.int32 or tuple(params.shape) != (b, views, 4) or not params.is_contiguous():
        raise ValueError('params must be a contiguous (b, views, 4) int32 tensor')
    if out is None:
        out = torch.empty((b, 3 * views, T, H_out, W_out), dtype=out_dtype, device=frames.device)
    elif tuple(out.shape) != (b, 3 * views, T, H_out, W_out) or not out.is_contiguous() or out.dtype not in (torch.float32, torch.float16):
        raise ValueError('out must be a contiguous (b, 3*views, T, H, W) fp32 / fp16 tensor')
    m = np.ascontiguousarray(mean255, dtype=np.float32)
    d = np.ascontiguousarray(inv_std255, dtype=np.float32)
    H.call('gca_clip_prepare', frames.data_ptr(), b, views, T, Hs, Ws, params.data_ptr(), m.ctypes.data, d.ctypes.data,
           H_out, W_out, out.data_ptr(), int(out.dtype is torch.float16), ops.stream())
    return out


# ---------------------------------------------------------------------------------------------- augment mode: host side
AUG_REC = 24                      # int32 words per (clip, view) record of gca_clip_augment (include/gca_hip.h)
AUG_TAP_SHIFT, AUG_BLUR_SHIFT, AUG_HSV_SHIFT = 11, 12, 12


def augment_identity(y0, x0, H, W, flip=False):
    """The parameters under which gca_clip_augment computes what gca_clip_prepare does: an H x W crop at (y0, x0), a flip."""
    return dict(y0=y0, x0=x0, ch=H, cw=W, jitter=False, perm=(0, 1, 2, 3), brightness=1.0, contrast=1.0, saturation=1.0,
                hue=0.0, gray=False, k=0, sigma=0.0, flip=bool(flip))


def sample_augment(Hs, Ws, rnd, nprnd, scale=(0.2, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), brightness=0.4, contrast=0.4,
                   saturation=0.4, hue=0.1, p_jitter=0.8, p_gray=0.2, p_blur=0.5, blur_limit=(3, 7), sigma_limit=(0.1, 2.0),
                   p_flip=0.5):
    """Parameters of one (clip, view), drawn as the reference's chain draws them and in its order (defaults:
    build_video_contrast_transform_cv2): VideoRandomResizedCrop.get_params (ten attempts, then the central crop),
    VideoRandomApply + VideoRandomColorJitter.get_params (four factors, then random.shuffle of the four ops),
    VideoRandomGrayScale, VideoRandomApply + VideoGaussianBlur.get_params (size from np.random, even sizes moved up, sigma),
    VideoRandomHorizontalFlip.  rnd: a random.Random (or the random module); nprnd: a np.random.RandomState (or np.random)."""
    area = Hs * Ws
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for _ in range(10):
        target = rnd.uniform(*scale) * area
        aspect = math.exp(rnd.uniform(*log_ratio))
        cw = int(round(math.sqrt(target * aspect)))
        ch = int(round(math.sqrt(target / aspect)))
        if 0 < cw <= Ws and 0 < ch <= Hs:
            i, j = rnd.randint(0, Hs - ch), rnd.randint(0, Ws - cw)
            break
    else:
        in_ratio = Ws / Hs
        if in_ratio < min(ratio):
            cw = Ws
            ch = int(round(cw / min(ratio)))
        elif in_ratio > max(ratio):
            ch = Hs
            cw = int(round(ch * max(ratio)))
        else:
            cw, ch = Ws, Hs
        i, j = (Hs - ch) // 2, (Ws - cw) // 2
    # the reference turns (i, j) into fractions and F.random_crop turns them back: that round trip can land on i - 1
    y0, x0 = crop_coords(Hs, Ws, ch, cw, i * 1.0 / (Hs - ch + 1e-10), j * 1.0 / (Ws - cw + 1e-10))
    p = augment_identity(y0, x0, ch, cw)
    if rnd.random() < p_jitter:
        p['jitter'] = True
        p['brightness'] = rnd.uniform(max(0, 1 - brightness), 1 + brightness)
        p['contrast'] = rnd.uniform(max(0, 1 - contrast), 1 + contrast)
        p['saturation'] = rnd.uniform(max(0, 1 - saturation), 1 + saturation)
        p['hue'] = rnd.uniform(-hue, hue)
        order = [0, 1, 2, 3]
        rnd.shuffle(order)
        p['perm'] = tuple(order)
    p['gray'] = rnd.random() < p_gray
    if rnd.random() < p_blur:
        k = int(nprnd.randint(blur_limit[0], blur_limit[1] + 1))
        if k != 0 and k % 2 != 1:
            k = (k + 1) % (blur_limit[1] + 1)
        p['k'], p['sigma'] = k, rnd.uniform(*sigma_limit)
    p['flip'] = rnd.random() < p_flip
    return p


def hsv_div_tables():
    """(2, 256) int32: round((255 << 12) / i) and round((180 << 12) / (6 i)), entry 0 = 0 -- the division tables of the
    8-bit RGB -> HSV conversion (H in [0, 180))."""
    t = np.zeros((2, 256), dtype=np.int32)
    i = np.arange(1, 256, dtype=np.float64)
    t[0, 1:] = np.rint((255 << AUG_HSV_SHIFT) / i).astype(np.int32)
    t[1, 1:] = np.rint((180 << AUG_HSV_SHIFT) / (6.0 * i)).astype(np.int32)
    return t


def _resize_taps(origin, crop, out):
    """(out, 4) int16 {i0, i1, c0, c1}: half-pixel-centre bilinear taps of one axis, indices in frame coordinates and clamped
    to the crop box, 11-bit weights."""
    f = (np.arange(out, dtype=np.float64) + 0.5) * (float(crop) / float(out)) - 0.5
    s = np.floor(f)
    a = f - s
    lo, hi = s < 0, s >= crop - 1
    a[lo | hi] = 0.0
    s[lo] = 0
    s[hi] = crop - 1
    i0 = s.astype(np.int64)
    c1 = np.rint(a * (1 << AUG_TAP_SHIFT)).astype(np.int64)
    return np.stack([origin + i0, origin + np.minimum(i0 + 1, crop - 1), (1 << AUG_TAP_SHIFT) - c1, c1], axis=1).astype(np.int16)


def _blur_weights(k, sigma):
    """k Gaussian taps in 12-bit fixed point; the rounding remainder goes to the centre tap (sum == 4096 exactly)."""
    x = np.arange(k, dtype=np.float64) - (k - 1) / 2.0
    w = np.exp(-(x * x) / (2.0 * float(sigma) * float(sigma)))
    w /= w.sum()
    q = np.floor(w * (1 << AUG_BLUR_SHIFT) + 0.5).astype(np.int64)
    q[k // 2] += (1 << AUG_BLUR_SHIFT) - q.sum()
    return q.astype(np.int32)


def _f32_bits(x):
    return int(np.array(x, dtype=np.float32).view(np.int32))


def check_augment_records(rec, Hs, Ws, H, W):
    """ValueError for records gca_clip_augment would refuse (the entry checks the same words and returns GCA_EINVAL)."""
    r = np.asarray(rec).reshape(-1, AUG_REC).astype(np.int64)
    if ((r[:, 0] < 0) | (r[:, 1] < 0) | (r[:, 2] < 1) | (r[:, 3] < 1) | (r[:, 0] + r[:, 2] > Hs) | (r[:, 1] + r[:, 3] > Ws)).any():
        raise ValueError('crop box outside the source frame')
    if not np.isin(r[:, 6], (0, 3, 5, 7)).all():
        raise ValueError('blur size must be 0, 3, 5 or 7')
    if (r[:, 6] // 2 >= min(H, W)).any():
        raise ValueError('blur radius does not fit the output (reflect-101 needs radius < size)')
    if not (np.sort(r[:, 7:11], axis=1) == np.arange(4)).all():
        raise ValueError('perm is not a permutation of the four jitter ops')
    if ((r[:, 4:6] & ~1) != 0).any() or ((r[:, 11] & ~15) != 0).any():
        raise ValueError('flip / gray must be 0 or 1 and mask a 4-bit set')
    w = r[:, 16:23]
    if (w < 0).any() or ((r[:, 6] > 0) & (w.sum(axis=1) != 1 << AUG_BLUR_SHIFT)).any() or \
            (w * (np.arange(7) >= r[:, 6:7])).any():
        raise ValueError('blur weights must be >= 0, sum to 4096 and be 0 past the k-th')


def pack_augment(params, Hs, Ws, H, W, out=None):
    """params: b lists of `views` dicts (sample_augment / augment_identity) -> (records (b, views, 24) int32, taps
    (b, views, H + W, 4) int16, luts (b, views, 2, 256) uint8), the layout of include/gca_hip.h.  out: such a triple to fill
    in place (the pinned buffers of DeviceInputStage.acquire())."""
    b, views = len(params), len(params[0])
    if out is None:
        out = (np.zeros((b, views, AUG_REC), np.int32), np.zeros((b, views, H + W, 4), np.int16), np.zeros((b, views, 2, 256), np.uint8))
    rec, taps, luts = out
    if rec.shape != (b, views, AUG_REC) or taps.shape != (b, views, H + W, 4) or luts.shape != (b, views, 2, 256):
        raise ValueError('out does not have the table shapes of a (%d, %d) batch' % (b, views))
    one = np.float32(1)
    ramp = np.arange(256, dtype=np.float64)
    for n in range(b):
        for v in range(views):
            p = params[n][v]
            r = rec[n, v]
            r[:] = 0
            r[0:7] = (p['y0'], p['x0'], p['ch'], p['cw'], int(bool(p['flip'])), int(bool(p['gray'])), p['k'])
            if sorted(p['perm']) != [0, 1, 2, 3]:
                raise ValueError('perm is not a permutation of the four jitter ops')
            r[7:11] = p['perm']
            fb, fh = (float(p['brightness']), float(p['hue'])) if p['jitter'] else (1.0, 0.0)
            fc, fs = np.float32(p['contrast']), np.float32(p['saturation'])
            if p['jitter']:           # factor 1 / hue 0: the identity by definition, the op is left out
                r[11] = int(fb != 1.0) | int(fc != one) << 1 | int(fs != one) << 2 | int(fh != 0.0) << 3
            r[12:16] = (_f32_bits(fc), _f32_bits(one - fc), _f32_bits(fs), _f32_bits(one - fs))
            if p['k'] in (3, 5, 7):
                if not p['sigma'] > 0:
                    raise ValueError('blur needs sigma > 0')
                r[16:16 + p['k']] = _blur_weights(p['k'], p['sigma'])
            check_augment_records(r, Hs, Ws, H, W)
            taps[n, v, :H] = _resize_taps(p['y0'], p['ch'], H)
            taps[n, v, H:] = _resize_taps(p['x0'], p['cw'], W)
            luts[n, v, 0] = np.clip(ramp * fb, 0, 255).astype(np.uint8)
            luts[n, v, 1] = np.mod(np.arange(256, dtype=np.int16) + 180.0 * fh, 180).astype(np.uint8)
    return rec, taps, luts


def clip_augment(frames, tables, mean255, inv_std255, H_out, W_out, out=None, out_dtype=torch.float32, dev_tables=None,
                 divtab=None, ws=None):
    """frames (b, views, T, Hs, Ws, 3) uint8 device tensor, tables = pack_augment(...) (host arrays) ->
    (b, 3*views, T, H_out, W_out) fp32 | fp16 through gca_clip_augment.  dev_tables: the same three arrays already on the
    device (the stage copies them on its copy stream; only the records are then needed on the host); otherwise they are
    uploaded here.  divtab / ws: optional preallocated device division tables / workspace."""
    if frames.dtype is not torch.uint8 or frames.dim() != 6 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise ValueError('frames must be a contiguous (b, views, T, Hs, Ws, 3) uint8 tensor')
    if not frames.is_cuda:
        raise RuntimeError('clip_augment needs the frames on the GPU (there is no CPU fallback)')
    b, views, T, Hs, Ws, _ = frames.shape
    rec, taps, luts = tables
    rec = np.ascontiguousarray(rec, dtype=np.int32)
    shapes = ((b, views, AUG_REC), (b, views, H_out + W_out, 4), (b, views, 2, 256))
    if rec.shape != shapes[0] or tuple(tuple(t.shape) for t in (dev_tables or (rec, taps, luts))) != shapes:
        raise ValueError('tables must be (b, views, 24) int32, (b, views, H + W, 4) int16 and (b, views, 2, 256) uint8')
    check_augment_records(rec, Hs, Ws, H_out, W_out)
    dev = frames.device
    if dev_tables is None:
        dev_tables = (torch.from_numpy(rec).to(dev), torch.from_numpy(np.ascontiguousarray(taps, dtype=np.int16)).to(dev),
                      torch.from_numpy(np.ascontiguousarray(luts, dtype=np.uint8)).to(dev))
    drec, dtaps, dluts = dev_tables
    if divtab is None:
        divtab = torch.from_numpy(hsv_div_tables()).to(dev)
    need = int(H.lib.gca_clip_augment_ws_bytes(b, views, T))
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    elif ws.numel() * ws.element_size() < need:
        raise ValueError('workspace smaller than gca_clip_augment_ws_bytes')
    if out is None:
        out = torch.empty((b, 3 * views, T, H_out, W_out), dtype=out_dtype, device=dev)
    elif tuple(out.shape) != (b, 3 * views, T, H_out, W_out) or not out.is_contiguous() or out.dtype not in (torch.float32, torch.float16):
        raise ValueError('out must be a contiguous (b, 3*views, T, H, W) fp32 / fp16 tensor')
    m = np.ascontiguousarray(mean255, dtype=np.float32)
    d = np.ascontiguousarray(inv_std255, dtype=np.float32)
    H.call('gca_clip_augment', frames.data_ptr(), b, views, T, Hs, Ws, rec.ctypes.data, drec.data_ptr(), dtaps.data_ptr(),
           dluts.data_ptr(), divtab.data_ptr(), m.ctypes.data, d.ctypes.data, H_out, W_out, out.data_ptr(),
           int(out.dtype is torch.float16), ws.data_ptr(), ops.stream())
    return out


class StagedBatch(object):
    """One batch on its way to the GPU: device uint8 frames + params and the event that marks the end of its copy."""
    __slots__ = ('frames', 'params', 'ready', 'slot', 'stage', 'records')

    def __init__(self, stage, slot, frames, params, ready, records=None):
        self.stage, self.slot, self.frames, self.params, self.ready = stage, slot, frames, params, ready
        self.records = records          # augment mode: host copy of the records (params = the device tables)


class DeviceInputStage(object):
    def __init__(self, batch, frames, src_size, out_size, device, views=2, mean=(0.485, 0.456, 0.406),
                 std=(0.229, 0.224, 0.225), slots=2, augment=False):
        """augment=False (default): frames arrive augmented, params are (b, views, 4) {h0, w0, flip, 0} (gca_clip_prepare).
        augment=True: frames are decoded source frames of src_size, params are b lists of `views` dicts of sample_augment
        (gca_clip_augment does the contrastive chain; the output may be larger than a crop box)."""
        self.b, self.views, self.T = int(batch), int(views), int(frames)
        self.Hs, self.Ws = (src_size, src_size) if isinstance(src_size, int) else tuple(src_size)
        self.H, self.W = (out_size, out_size) if isinstance(out_size, int) else tuple(out_size)
        self.augment = bool(augment)
        if not self.augment and (self.H > self.Hs or self.W > self.Ws):
            raise ValueError('crop %r larger than the source frames %r' % ((self.H, self.W), (self.Hs, self.Ws)))
        self.device = torch.device(device)
        self.mean255, self.inv_std255 = normalize_constants(mean, std)
        shape = (self.b, self.views, self.T, self.Hs, self.Ws, 3)
        self._host = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self._dev = [torch.empty(shape, dtype=torch.uint8, device=self.device) for _ in range(slots)]
        if self.augment:
            # records | taps | luts of a slot live in ONE pinned buffer and ONE device buffer: one small H2D copy per batch
            nv = self.b * self.views
            sizes = (nv * AUG_REC * 4, nv * (self.H + self.W) * 8, nv * 512)
            self._hostp = [torch.empty(sum(sizes), dtype=torch.uint8).pin_memory() for _ in range(slots)]
            self._devp = [torch.empty(sum(sizes), dtype=torch.uint8, device=self.device) for _ in range(slots)]
            self._table_sizes = sizes
            self._divtab = torch.from_numpy(hsv_div_tables()).to(self.device)
            self._ws = torch.empty(int(H.lib.gca_clip_augment_ws_bytes(self.b, self.views, self.T)), dtype=torch.uint8,
                                   device=self.device)
        else:
            self._hostp = [torch.empty((self.b, self.views, 4), dtype=torch.int32).pin_memory() for _ in range(slots)]
            self._devp = [torch.empty((self.b, self.views, 4), dtype=torch.int32, device=self.device) for _ in range(slots)]
        self._consumed = [None] * slots          # event recorded on the compute stream after the slot's kernel was issued
        self._copied = [None] * slots            # event of the slot's last H2D copy (its pinned buffer is free after it)
        self._next = 0
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.frame_bytes = int(np.prod(shape))

    def _tables(self, blob):
        """(records, taps, luts) views of one slot's table buffer (host or device)."""
        a, t, _ = self._table_sizes
        return (blob[:a].view(torch.int32).view(self.b, self.views, AUG_REC),
                blob[a:a + t].view(torch.int16).view(self.b, self.views, self.H + self.W, 4),
                blob[a + t:].view(self.b, self.views, 2, 256))

    def out_shape(self):
        return (self.b, 3 * self.views, self.T, self.H, self.W)

    def acquire(self):
        """-> (frames, params): the pinned host buffers of the next slot -- (b, views, T, Hs, Ws, 3) uint8 and (b, views, 4)
        int32 {h0, w0, flip, 0} -- for the loader to fill IN PLACE (decoded frames land in pinned memory once; no second host
        copy).  Blocks only if the slot's previous H2D copy is still in flight.  Follow with submit().
        augment mode: params is the (records, taps, luts) triple of numpy views that pack_augment(..., out=params) fills."""
        s = self._next
        if self._copied[s] is not None:
            self._copied[s].synchronize()            # the pinned buffers of this slot are about to be overwritten by the host
        if self.augment:
            return self._host[s], tuple(t.numpy() for t in self._tables(self._hostp[s]))
        return self._host[s], self._hostp[s]

    def submit(self, check=True):
        """Start the asynchronous H2D copy of the slot handed out by the last acquire(); returns a StagedBatch."""
        s = self._next
        self._next = (s + 1) % len(self._host)
        records = None
        if self.augment:
            records = self._tables(self._hostp[s])[0].numpy().copy()     # what the entry validates at prepare() time
            if check:
                check_augment_records(records, self.Hs, self.Ws, self.H, self.W)
        elif check:
            p = self._hostp[s]
            if (int(p[..., 0].min()) < 0 or int(p[..., 1].min()) < 0 or int(p[..., 0].max()) > self.Hs - self.H
                    or int(p[..., 1].max()) > self.Ws - self.W):
                raise ValueError('crop window outside the source frame')
        with torch.cuda.stream(self.copy_stream):
            if self._consumed[s] is not None:
                self.copy_stream.wait_event(self._consumed[s])    # the kernel that read this device slot has been issued and passed
            self._dev[s].copy_(self._host[s], non_blocking=True)
            self._devp[s].copy_(self._hostp[s], non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(self.copy_stream)
        self._copied[s] = ready
        return StagedBatch(self, s, self._dev[s], self._devp[s], ready, records)

    def stage(self, frames, params):
        """Convenience for callers that hold the batch elsewhere: frames (b, views, T, Hs, Ws, 3) uint8 host tensor / ndarray,
        params (b, views, >=3) integers {h0, w0, flip}.  = acquire() + one host copy into the pinned slot + submit().
        augment mode: params = b lists of `views` dicts (sample_augment)."""
        f = torch.as_tensor(frames)
        if tuple(f.shape) != tuple(self._host[0].shape) or f.dtype is not torch.uint8:
            raise ValueError('frames must be uint8 of shape %r, got %s %r' % (tuple(self._host[0].shape), f.dtype, tuple(f.shape)))
        if self.augment:
            if len(params) != self.b or any(len(q) != self.views for q in params):
                raise ValueError('params must be b lists of `views` parameter dicts')
            # (packed before the slot is acquired: a refused record leaves the slot untouched)
            tables = pack_augment(params, self.Hs, self.Ws, self.H, self.W)
            hf, ht = self.acquire()
            hf.copy_(f)
            for dst, src in zip(ht, tables):
                dst[...] = src
            return self.submit(check=False)
        p = torch.as_tensor(np.asarray(params))
        if p.dim() != 3 or tuple(p.shape[:2]) != (self.b, self.views) or p.shape[2] < 3:
            raise ValueError('params must be (b, views, >=3): h0, w0, flip')
        hf, hp = self.acquire()
        hf.copy_(f)
        hp.zero_()
        hp[..., :3].copy_(p[..., :3].to(torch.int32))
        return self.submit()

    def prepare(self, staged, out):
        """Compute stream: wait for the copy, then crop + flip + normalise + layout change into `out`."""
        if staged.stage is not self:
            raise ValueError('batch was staged by another DeviceInputStage')
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(staged.ready)
        if self.augment:
            clip_augment(staged.frames, (staged.records, None, None), self.mean255, self.inv_std255, self.H, self.W, out=out,
                         dev_tables=self._tables(staged.params), divtab=self._divtab, ws=self._ws)
        else:
            clip_prepare(staged.frames, staged.params, self.mean255, self.inv_std255, self.H, self.W, out=out)
        done = torch.cuda.Event()
        done.record(cur)
        self._consumed[staged.slot] = done
        return out


# ---------------------------------------------------------------------------------------------- downstream views: host side
# Action recognition feeds on other transforms than pre-training (lib/data/transform/build.py:27-35, tools/test_ds.py:95-120):
# a multi-scale crop resized to the input size for training, and 1 / 3 / 5 / 10 crops of a resized frame times test_clips
# temporal clips for testing.  Every view of a video is a window of ONE resized copy of its frames, and a crop of a resized
# uint8 frame is a window of the resize's tap table -- so the host ships the decoded source once and gca_clip_views cuts all
# views out of it.  tests/views_ref.py is the specification; the functions below are held equal to it.
VIEW_REC = 8                      # int32 words per view record of gca_clip_views: src, t0, tab, oy, ox, flip, 0, 0
MULTISCALE_SCALES = (1, .875, .75, .66)


def _hw(size):
    return (int(size), int(size)) if isinstance(size, (int, np.integer)) else (int(size[0]), int(size[1]))


def _fix_offsets(more_fix_crop, image_w, image_h, crop_w, crop_h):
    """VideoMultiScaleCrop.fill_fix_offset (consistency_transforms.py:446-468): (w, h) offsets as FLOATS, truncated by their
    users."""
    ws, hs = (image_w - crop_w) / 4, (image_h - crop_h) / 4
    ret = [(0, 0), (4 * ws, 0), (0, 4 * hs), (4 * ws, 4 * hs), (2 * ws, 2 * hs)]
    if more_fix_crop:
        ret += [(0, 2 * hs), (4 * ws, 2 * hs), (2 * ws, 4 * hs), (2 * ws, 0 * hs), (1 * ws, 1 * hs), (3 * ws, 1 * hs),
                (1 * ws, 3 * hs), (3 * ws, 3 * hs)]
    return ret


def sample_multiscale_crop(Hs, Ws, input_size, nprnd, rnd, scales=MULTISCALE_SCALES, max_distort=1, fix_crop=True,
                           more_fix_crop=True, p_flip=0.5):
    """Parameters of one training clip, drawn as VideoMultiScaleCrop._sample_crop_size + VideoRandomHorizontalFlip draw them
    and in their order (consistency_transforms.py:405-436, 355-356): the crop pair, the fixed offset (or, fix_crop off, the two
    randint(0, img - crop) draws), the flip.  nprnd: a np.random.RandomState (or np.random); rnd: a random.Random (or the
    random module).  -> dict(y0, x0, ch, cw, flip).  The reference compares crop_h with input_size[1] and crop_w with
    input_size[0] although it resizes to input_size[0] rows: kept as it is (every config is square)."""
    size = _hw(input_size)
    base = min(Ws, Hs)
    sizes = [int(base * x) for x in scales]
    crop_h = [size[1] if abs(x - size[1]) < 3 else x for x in sizes]
    crop_w = [size[0] if abs(x - size[0]) < 3 else x for x in sizes]
    pairs = [(w, h) for i, h in enumerate(crop_h) for j, w in enumerate(crop_w) if abs(i - j) <= max_distort]
    cw, ch = pairs[nprnd.randint(len(pairs))]
    if fix_crop:
        offsets = _fix_offsets(more_fix_crop, Ws, Hs, cw, ch)
        x0, y0 = offsets[nprnd.randint(len(offsets))]
    else:
        x0 = nprnd.randint(0, Ws - cw)
        y0 = nprnd.randint(0, Hs - ch)
    return dict(y0=int(y0), x0=int(x0), ch=int(ch), cw=int(cw), flip=bool(rnd.random() < p_flip))


def test_view_layout(Hs, Ws, scale_size, crop_size, test_crops, test_clips, T):
    """The views of ONE test video (tools/test_ds.py:95-114) -> (records (views, 8) int32 with src = 0, taps (1, Hr + Wr, 4)
    int16): VideoResize(scale_size) as one tap table over the whole source frame, and one record per (crop origin, flip,
    temporal clip), in that nesting (the order in which consistency_transforms.py:491-506 emits them).
    test_crops 1: the central crop; 3: VideoFullResSample's left / right / centre at integer steps (:528-534); 5:
    VideoOverSampleCrop's corners and centre at float steps truncated by int() (:489-495); 10: the same, each also flipped."""
    (Hr, Wr), (H, W) = _hw(scale_size), _hw(crop_size)
    if test_crops == 1:
        origins, flips = [((Hr - H) // 2, (Wr - W) // 2)], (0,)
    elif test_crops == 3:
        ws, hs = (Wr - W) // 4, (Hr - H) // 4
        origins, flips = [(2 * hs, 0), (2 * hs, 4 * ws), (2 * hs, 2 * ws)], (0,)
    elif test_crops in (5, 10):
        origins = [(int(oh), int(ow)) for ow, oh in _fix_offsets(False, Wr, Hr, W, H)]
        flips = (0,) if test_crops == 5 else (0, 1)
    else:
        raise ValueError('only 1, 3, 5 and 10 test crops are supported, got %r' % (test_crops,))
    if H < 1 or W < 1 or H > Hr or W > Wr or test_clips < 1 or T < 1:
        raise ValueError('crop %r does not fit the resized frame %r' % ((H, W), (Hr, Wr)))
    taps = np.concatenate([_resize_taps(0, Hs, Hr), _resize_taps(0, Ws, Wr)])[None]
    rec = [(0, clip * T, 0, oy, ox, flip, 0, 0) for oy, ox in origins for flip in flips for clip in range(test_clips)]
    return np.array(rec, dtype=np.int32), taps


test_view_layout.__test__ = False          # (a name for the reference's test mode, not a test)


def check_views(records, taps, Lh, n_src, F, Hs, Ws, T, H_out, W_out):
    """ValueError for tables gca_clip_views would refuse (the entry checks the same record words and returns GCA_EINVAL) and
    for tap indices outside the frame, which only the host checks (the kernel clamps them)."""
    H, W = H_out, W_out
    r, t = np.asarray(records), np.asarray(taps)
    if r.ndim != 2 or r.shape[1] != VIEW_REC or t.ndim != 3 or t.shape[2] != 4 or t.shape[0] < 1:
        raise ValueError('tables must be (n_views, 8) records and (n_tab, Lh + Lw, 4) taps')
    if min(n_src, F, Hs, Ws, T, H, W) < 1 or max(Hs, Ws) > 32767:
        raise ValueError('sizes must be >= 1 and source frames at most 32767 x 32767')
    r = r.astype(np.int64)
    n_tab, Lw = t.shape[0], t.shape[1] - Lh
    if Lh < H or Lw < W:
        raise ValueError('tap table (%d rows, %d columns) smaller than the output %r' % (Lh, Lw, (H, W)))
    if ((r[:, 0] < 0) | (r[:, 0] >= n_src)).any() or ((r[:, 2] < 0) | (r[:, 2] >= n_tab)).any():
        raise ValueError('record names a source outside [0, %d) or a table outside [0, %d)' % (n_src, n_tab))
    if ((r[:, 1] < 0) | (r[:, 1] + T > F)).any():
        raise ValueError('temporal clip outside the source: t0 + T > F = %d' % F)
    if ((r[:, 3] < 0) | (r[:, 3] + H > Lh) | (r[:, 4] < 0) | (r[:, 4] + W > Lw)).any():
        raise ValueError('window outside the tap table')
    if ((r[:, 5] & ~1) != 0).any():
        raise ValueError('flip must be 0 or 1')
    rows, cols = t[:, :Lh, :2], t[:, Lh:, :2]
    if rows.min() < 0 or rows.max() >= Hs or cols.min() < 0 or cols.max() >= Ws:
        raise ValueError('tap index outside the source frame')


def pack_views(views, n_src, F, Hs, Ws, T, H, W, out=None):
    """The tables of one batch for clip_views / gca_clip_views -> (records (n_views, 8) int32, taps (n_tab, Lh + Lw, 4) int16,
    Lh), checked.  `views` is one of
      * a list of n_src dicts of sample_multiscale_crop (training): clip n is view n, reads source n through its own table,
        whose taps map the crop box onto the (H, W) output; Lh = H;
      * a dict(scale_size=, test_crops=, test_clips=) (testing): test_view_layout's records repeated for each of the n_src
        videos, video-major, and its single table; Lh = the resized height; crop size = (H, W);
      * (records, taps, Lh): tables made elsewhere, only checked.
    ValueError for a crop box or a tap outside the frame, a window outside the table, t0 + T > F, an unsupported test_crops.
    out: a (records, taps) pair of arrays to fill in place (the pinned buffers of ActionInputStage.acquire())."""
    if isinstance(views, dict):
        rec1, taps = test_view_layout(Hs, Ws, views['scale_size'], (H, W), views['test_crops'], views.get('test_clips', 1), T)
        rec = np.tile(rec1, (n_src, 1))
        rec[:, 0] = np.repeat(np.arange(n_src, dtype=np.int32), len(rec1))
        Lh = _hw(views['scale_size'])[0]
    elif isinstance(views, (tuple, list)) and len(views) == 3 and isinstance(views[0], np.ndarray):
        rec, taps, Lh = np.ascontiguousarray(views[0], dtype=np.int32), np.ascontiguousarray(views[1], dtype=np.int16), int(views[2])
    else:
        if len(views) != n_src:
            raise ValueError('one parameter dict per clip expected (got %d for %d clips)' % (len(views), n_src))
        rec = np.zeros((n_src, VIEW_REC), dtype=np.int32)
        taps = np.zeros((n_src, H + W, 4), dtype=np.int16)
        for n, p in enumerate(views):
            if p['ch'] < 1 or p['cw'] < 1 or p['y0'] < 0 or p['x0'] < 0 or p['y0'] + p['ch'] > Hs or p['x0'] + p['cw'] > Ws:
                raise ValueError('crop box outside the source frame')
            rec[n, :6] = (n, 0, n, 0, 0, int(bool(p['flip'])))
            taps[n, :H] = _resize_taps(p['y0'], p['ch'], H)
            taps[n, H:] = _resize_taps(p['x0'], p['cw'], W)
        Lh = H
    check_views(rec, taps, Lh, n_src, F, Hs, Ws, T, H, W)
    if out is not None:
        if out[0].shape != rec.shape or out[1].shape != taps.shape:
            raise ValueError('out does not have the table shapes of this batch')
        out[0][...] = rec
        out[1][...] = taps
        rec, taps = out
    return rec, taps, Lh


def clip_views(frames, tables, mean255, inv_std255, T, H_out, W_out, out=None, dev_tables=None):
    """frames (n_src, F, Hs, Ws, 3) uint8 device tensor, tables = pack_views(...) = (records, taps, Lh) host arrays ->
    (n_views, 3, T, H_out, W_out) fp32 through gca_clip_views.  dev_tables: (records, taps) already on the device (the stage
    copies or keeps them there); the host taps may then be None, having been checked when they were packed.  Otherwise the
    tables are checked here -- every record word the entry checks, and that every tap index lies inside the frame -- and
    uploaded."""
    if frames.dtype is not torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise ValueError('frames must be a contiguous (n_src, F, Hs, Ws, 3) uint8 tensor')
    if not frames.is_cuda:
        raise RuntimeError('clip_views needs the frames on the GPU (there is no CPU fallback)')
    n_src, F, Hs, Ws, _ = frames.shape
    rec, taps, Lh = tables
    rec = np.ascontiguousarray(rec, dtype=np.int32)
    if rec.ndim != 2 or rec.shape[1] != VIEW_REC:
        raise ValueError('records must be (n_views, 8) int32')
    dev = frames.device
    if dev_tables is None:
        taps = np.ascontiguousarray(taps, dtype=np.int16)
        check_views(rec, taps, Lh, n_src, F, Hs, Ws, T, H_out, W_out)
        dev_tables = (torch.from_numpy(rec).to(dev), torch.from_numpy(taps).to(dev))
    drec, dtaps = dev_tables
    if (drec.dtype is not torch.int32 or tuple(drec.shape) != rec.shape or dtaps.dtype is not torch.int16 or dtaps.dim() != 3
            or dtaps.shape[2] != 4 or dtaps.shape[1] <= Lh or not drec.is_cuda or not dtaps.is_cuda
            or not drec.is_contiguous() or not dtaps.is_contiguous()):
        raise ValueError('device tables must be (n_views, 8) int32 records and (n_tab, Lh + Lw, 4) int16 taps on the GPU')
    n_views, n_tab, Lw = rec.shape[0], dtaps.shape[0], dtaps.shape[1] - Lh
    if out is None:
        out = torch.empty((n_views, 3, T, H_out, W_out), dtype=torch.float32, device=dev)
    elif (tuple(out.shape) != (n_views, 3, T, H_out, W_out) or not out.is_contiguous() or out.dtype is not torch.float32
          or out.device != dev):
        raise ValueError('out must be a contiguous (n_views, 3, T, H, W) fp32 tensor on the frames\' device')
    m = np.ascontiguousarray(mean255, dtype=np.float32)
    d = np.ascontiguousarray(inv_std255, dtype=np.float32)
    H.call('gca_clip_views', frames.data_ptr(), n_src, F, Hs, Ws, rec.ctypes.data, drec.data_ptr(), n_views, dtaps.data_ptr(),
           n_tab, Lh, Lw, m.ctypes.data, d.ctypes.data, T, H_out, W_out, out.data_ptr(), ops.stream())
    return out


class ActionInputStage(object):
    """DeviceInputStage's pipeline for action recognition: decoded uint8 source frames in, (batch * views, 3, T, H, W) fp32
    clips out through gca_clip_views; two pinned host buffers and two device buffers, the H2D copy on a copy stream, prepare()
    on the compute stream behind an event.

    mode='train': frames (batch, T, Hs, Ws, 3), one dict of sample_multiscale_crop per clip; the (records, taps) of a batch
    travel with it in one small copy.  views = 1.
    mode='test': frames (batch, test_clips * T, Hs, Ws, 3); the tap table of VideoResize(scale_size) and the records of the
    test_crops x test_clips views of every video are built ONCE here and stay on the device: a batch ships frames only.
    views = crops x test_clips (x 2 flips at test_crops = 10), video-major in the output.

    Unlike DeviceInputStage, a slot whose batch has not been through prepare() is never handed out again: staging more
    batches ahead than there are slots raises RuntimeError instead of overwriting a batch that is still waiting."""

    def __init__(self, batch, frames_per_video, src_size, out_size, device, mode='train', scale_size=None, test_crops=1,
                 test_clips=1, T=None, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), slots=2):
        if mode not in ('train', 'test'):
            raise ValueError('mode must be \'train\' or \'test\'')
        self.mode, self.b, self.F = mode, int(batch), int(frames_per_video)
        self.Hs, self.Ws = _hw(src_size)
        self.H, self.W = _hw(out_size)
        self.device = torch.device(device)
        self.mean255, self.inv_std255 = normalize_constants(mean, std)
        if mode == 'train':
            self.T = self.F if T is None else int(T)
            if self.T != self.F:
                raise ValueError('training clips are the whole source: frames_per_video must equal T')
            self.views, self.Lh, self.n_tab = 1, self.H, self.b
            self._table_sizes = (self.b * VIEW_REC * 4, self.b * (self.H + self.W) * 8)
            self._hostp = [torch.empty(sum(self._table_sizes), dtype=torch.uint8).pin_memory() for _ in range(slots)]
            self._devp = [torch.empty(sum(self._table_sizes), dtype=torch.uint8, device=self.device) for _ in range(slots)]
        else:
            if scale_size is None:
                raise ValueError('test mode needs scale_size (VideoResize)')
            self.T = self.F // int(test_clips) if T is None else int(T)
            if self.T < 1 or self.T * int(test_clips) != self.F:
                raise ValueError('frames_per_video must be test_clips * T')
            spec = dict(scale_size=scale_size, test_crops=test_crops, test_clips=test_clips)
            rec, taps, self.Lh = pack_views(spec, self.b, self.F, self.Hs, self.Ws, self.T, self.H, self.W)
            self.views, self.n_tab = rec.shape[0] // self.b, 1
            self._records = rec
            self._dev_tables = (torch.from_numpy(rec).to(self.device), torch.from_numpy(taps).to(self.device))
        shape = (self.b, self.F, self.Hs, self.Ws, 3)
        self._host = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self._dev = [torch.empty(shape, dtype=torch.uint8, device=self.device) for _ in range(slots)]
        self._consumed = [None] * slots          # event recorded on the compute stream after the slot's kernel was issued
        self._copied = [None] * slots            # event of the slot's last H2D copy (its pinned buffer is free after it)
        self._pending = [False] * slots          # staged, not yet through prepare(): the slot must not be staged into
        self._next = 0
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.frame_bytes = int(np.prod(shape))

    def _tables(self, blob):
        """(records, taps) views of one slot's table buffer (host or device); training mode."""
        a = self._table_sizes[0]
        return (blob[:a].view(torch.int32).view(self.b, VIEW_REC), blob[a:].view(torch.int16).view(self.b, self.H + self.W, 4))

    def out_shape(self):
        return (self.b * self.views, 3, self.T, self.H, self.W)

    def acquire(self):
        """-> (frames, tables): the pinned host buffers of the next slot for the loader to fill IN PLACE -- frames
        (batch, F, Hs, Ws, 3) uint8 and, in training mode, the (records, taps) numpy views that
        pack_views(params, ..., out=tables) fills (None in test mode).  RuntimeError if the slot still holds a batch that has
        not been through prepare().  Blocks only if the slot's previous H2D copy is still in flight.  Follow with submit()."""
        s = self._next
        if self._pending[s]:
            raise RuntimeError('all %d slots hold batches that have not been through prepare(): staging another one would '
                               'overwrite a batch that is still waiting' % len(self._host))
        if self._copied[s] is not None:
            self._copied[s].synchronize()            # the pinned buffers of this slot are about to be overwritten by the host
        if self.mode == 'train':
            return self._host[s], tuple(t.numpy() for t in self._tables(self._hostp[s]))
        return self._host[s], None

    def submit(self, check=True):
        """Start the asynchronous H2D copy of the slot handed out by the last acquire(); returns a StagedBatch."""
        s = self._next
        if self._pending[s]:
            raise RuntimeError('slot %d holds a batch that has not been through prepare()' % s)
        if self.mode == 'train':
            hrec, htaps = (t.numpy() for t in self._tables(self._hostp[s]))
            records = hrec.copy()                    # what the entry validates at prepare() time
            if check:
                check_views(records, htaps, self.Lh, self.b, self.F, self.Hs, self.Ws, self.T, self.H, self.W)
        else:
            records = self._records
        self._next = (s + 1) % len(self._host)
        with torch.cuda.stream(self.copy_stream):
            if self._consumed[s] is not None:
                self.copy_stream.wait_event(self._consumed[s])    # the kernel that read this device slot has been issued and passed
            self._dev[s].copy_(self._host[s], non_blocking=True)
            if self.mode == 'train':
                self._devp[s].copy_(self._hostp[s], non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(self.copy_stream)
        self._copied[s] = ready
        self._pending[s] = True
        tables = self._tables(self._devp[s]) if self.mode == 'train' else self._dev_tables
        return StagedBatch(self, s, self._dev[s], tables, ready, records)

    def stage(self, frames, params=None):
        """Convenience for callers that hold the batch elsewhere: frames (batch, F, Hs, Ws, 3) uint8 host tensor / ndarray and,
        in training mode, one dict of sample_multiscale_crop per clip.  = acquire() + one host copy + submit()."""
        f = torch.as_tensor(frames)
        if tuple(f.shape) != tuple(self._host[0].shape) or f.dtype is not torch.uint8:
            raise ValueError('frames must be uint8 of shape %r, got %s %r' % (tuple(self._host[0].shape), f.dtype, tuple(f.shape)))
        if self.mode == 'train':
            if params is None:
                raise ValueError('training mode needs one parameter dict per clip')
            # (packed before the slot is acquired: a refused record leaves the slot untouched)
            rec, taps, _ = pack_views(params, self.b, self.F, self.Hs, self.Ws, self.T, self.H, self.W)
            hf, (hrec, htaps) = self.acquire()
            hrec[...] = rec
            htaps[...] = taps
        else:
            if params is not None:
                raise ValueError('test mode takes frames only: the views are fixed at construction')
            hf, _ = self.acquire()
        hf.copy_(f)
        return self.submit(check=False)

    def prepare(self, staged, out):
        """Compute stream: wait for the copy, then all views of the batch into `out` (out_shape(), fp32)."""
        if staged.stage is not self:
            raise ValueError('batch was staged by another input stage')
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(staged.ready)
        clip_views(staged.frames, (staged.records, None, self.Lh), self.mean255, self.inv_std255, self.T, self.H, self.W, out=out,
                   dev_tables=staged.params)
        done = torch.cuda.Event()
        done.record(cur)
        self._consumed[staged.slot] = done
        self._pending[staged.slot] = False
        return out
