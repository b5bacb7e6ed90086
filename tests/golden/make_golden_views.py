#!/usr/bin/env python3
"""Generate tests/golden/views.npz by RUNNING THE REFERENCE's own multi-scale-crop and test-crop classes.

Run only where the reference lies; GCA_REFERENCE names its root, as for make_golden.py:

    GCA_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_views.py

Nothing of the reference is copied: lib/data/transform/consistency_transforms.py is imported from where it lies and only
arrays of what it returns are written.  Harness shim (shim 6 of make_golden.py, copied): inert placeholder modules for `cv2`
and `albumentations.augmentations.functional`, which that file imports at its top and which are not installed; any attribute
reads as 0 (cv2.INTER_LINEAR etc. are default arguments).  One addition: the placeholder's `hflip` / `hflip_cv2` are callables
that return None.  VideoOverSampleCrop builds its flipped list even under flip=False and throws it away (:494-506), so the
name must be callable; nothing of what it returns reaches a recorded array.  VideoRandomHorizontalFlip returns
[F.hflip(img) ...] when it decides to flip (:356-362), so a list of None IS the recorded decision.

Recorded, for (img_h, img_w, input_size) in SIZES:
  <tag>:pairs                 the (crop_w, crop_h) candidates of VideoMultiScaleCrop._sample_crop_size, in its order (read out
                              by steering np.random.randint: the first draw picks the pair, the second picks offset 0)
  <tag>:offsets:more|few      fill_fix_offset(more_fix_crop, img_w, img_h, w, h) of every pair: (pairs, 13 | 5, 2) float64
  <tag>:trace:more|few        64 calls of _sample_crop_size under np.random.seed(SEED): (64, 4) {crop_w, crop_h, off_w, off_h}
and once
  flip:trace                  64 decisions of VideoRandomHorizontalFlip(p=0.5) under random.seed(SEED)
and, for (img_h, img_w, crop_h, crop_w) in CROPS, on 3 index-coded frames (pixel = (y, x, frame)):
  <tag>:over | <tag>:full     VideoOverSampleCrop(crop, None, flip=False) / VideoFullResSample(crop, None, flip=False):
                              one row per emitted array {frame, y0, x0, h, w}, in the order emitted
"""
import importlib.util
import os
import random
import sys
import types
from unittest import mock

import numpy as np

sys.dont_write_bytecode = True
REF = os.environ.get('GCA_REFERENCE') or sys.exit('set GCA_REFERENCE to the root of the reference checkout')
HERE = os.path.dirname(os.path.abspath(__file__))

SEED = 11
SIZES = ((20, 27, 16), (27, 20, 16), (128, 171, 112), (240, 320, 224))
CROPS = ((18, 27, 16, 16), (18, 27, 16, 12), (128, 171, 112, 112))


def load_reference():
    class _Inert(types.ModuleType):                               # shim 6
        def __getattr__(self, name):
            if name.startswith('__'):
                raise AttributeError(name)
            return 0
    for name in ('cv2', 'albumentations', 'albumentations.augmentations', 'albumentations.augmentations.functional'):
        sys.modules.setdefault(name, _Inert(name))
        if '.' in name:                                           # `import a.b.c as F` walks the attributes
            parent, leaf = name.rsplit('.', 1)
            setattr(sys.modules[parent], leaf, sys.modules[name])
    fn = sys.modules['albumentations.augmentations.functional']
    fn.hflip = fn.hflip_cv2 = lambda img: None                    # callable, inert (see the module docstring)
    spec = importlib.util.spec_from_file_location('ref_consistency_transforms',
                                                  os.path.join(REF, 'lib', 'data', 'transform', 'consistency_transforms.py'))
    ct = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ct)
    return ct


def ref_pairs(msc, im_size):
    """The pairs list of _sample_crop_size, which it does not return: pick entry k with a steered first draw."""
    seen = []

    def steered(k):
        calls = []

        def randint(*a):
            calls.append(a)
            return k if len(calls) == 1 else 0
        with mock.patch.object(np.random, 'randint', randint):
            w, h, ow, oh = msc._sample_crop_size(im_size)
        assert len(calls) == 2 and (ow, oh) == (0, 0)
        return calls[0][0], (w, h)
    n, first = steered(0)
    seen.append(first)
    for k in range(1, n):
        seen.append(steered(k)[1])
    return np.array(seen, dtype=np.int64)


def main():
    ct = load_reference()
    out = {}
    for img_h, img_w, size in SIZES:
        tag = '%dx%d:%d' % (img_h, img_w, size)
        pairs = ref_pairs(ct.VideoMultiScaleCrop(size), (img_h, img_w))
        out[tag + ':pairs'] = pairs
        for name, more in (('more', True), ('few', False)):
            out[tag + ':offsets:' + name] = np.array(
                [ct.VideoMultiScaleCrop.fill_fix_offset(more, img_w, img_h, int(w), int(h)) for w, h in pairs], dtype=np.float64)
            msc = ct.VideoMultiScaleCrop(size, more_fix_crop=more)
            np.random.seed(SEED)
            out[tag + ':trace:' + name] = np.array([msc._sample_crop_size((img_h, img_w)) for _ in range(64)], dtype=np.int64)
    flipper = ct.VideoRandomHorizontalFlip(p=0.5)
    random.seed(SEED)
    clip = [np.zeros((2, 2, 3), dtype=np.int16)]
    out['flip:trace'] = np.array([flipper(clip)[0] is None for _ in range(64)], dtype=np.bool_)
    for img_h, img_w, ch, cw in CROPS:
        tag = '%dx%d:%dx%d' % (img_h, img_w, ch, cw)
        yy, xx = np.meshgrid(np.arange(img_h), np.arange(img_w), indexing='ij')
        frames = [np.stack([yy, xx, np.full_like(yy, f)], axis=-1).astype(np.int16) for f in range(3)]
        for name, cls in (('over', ct.VideoOverSampleCrop), ('full', ct.VideoFullResSample)):
            got = cls((ch, cw), None, flip=False)(frames)
            rows = []
            for a in got:
                y0, x0, f = (int(v) for v in a[0, 0])
                want = frames[f][y0:y0 + a.shape[0], x0:x0 + a.shape[1]]
                assert np.array_equal(a, want)                       # a plain window of frame f
                rows.append((f, y0, x0, a.shape[0], a.shape[1]))
            out[tag + ':' + name] = np.array(rows, dtype=np.int64)
    out['seed'] = np.array(SEED, dtype=np.int64)
    path = os.path.join(HERE, 'views.npz')
    np.savez_compressed(path, **out)
    print('views.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
