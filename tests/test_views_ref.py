"""tests/views_ref.py (the numpy specification of gca_clip_views) against the reference's own classes (tests/golden/views.npz,
written by tests/golden/make_golden_views.py), against tests/augment_ref.py where the two overlap, and the product's host
layer (engine.input.sample_multiscale_crop / test_view_layout / pack_views) against views_ref.  No GPU."""
import random

import numpy as np
import pytest
import torch

import augment_ref as ar
import views_ref as vr
from oracle import input as oinput

SIZES = ((20, 27, 16), (27, 20, 16), (128, 171, 112), (240, 320, 224))
CROPS = ((18, 27, 16, 16), (18, 27, 16, 12), (128, 171, 112, 112))


@pytest.fixture(scope='module')
def gold(golden):
    return golden('views').z


# ------------------------------------------------------------------------------------------------ pinned to the reference
def test_golden_holds_what_is_compared(gold):
    want = {'seed', 'flip:trace'}
    for h, w, s in SIZES:
        want |= {'%dx%d:%d:%s' % (h, w, s, k) for k in ('pairs', 'offsets:more', 'offsets:few', 'trace:more', 'trace:few')}
    for h, w, ch, cw in CROPS:
        want |= {'%dx%d:%dx%d:%s' % (h, w, ch, cw, k) for k in ('over', 'full')}
    assert set(gold.files) == want                                  # every array below is compared, none is left out


@pytest.mark.parametrize('img_h,img_w,size', SIZES)
def test_pairs_and_offsets_equal_the_reference(gold, img_h, img_w, size):
    tag = '%dx%d:%d' % (img_h, img_w, size)
    pairs = vr.multiscale_pairs(img_h, img_w, size)
    assert np.array_equal(np.array(pairs), gold[tag + ':pairs'])
    for name, more in (('more', True), ('few', False)):
        got = np.array([vr.fix_offsets(more, img_w, img_h, w, h) for w, h in pairs], dtype=np.float64)
        assert got.shape == gold[tag + ':offsets:' + name].shape and np.array_equal(got, gold[tag + ':offsets:' + name])
    assert len(vr.fix_offsets(True, 27, 20, 16, 16)) == 13 and len(vr.fix_offsets(False, 27, 20, 16, 16)) == 5


@pytest.mark.parametrize('img_h,img_w,size', SIZES)
def test_sample_train_replays_the_recorded_traces(gold, pkg, img_h, img_w, size):
    seed = int(gold['seed'])
    for name, more in (('more', True), ('few', False)):
        trace = gold['%dx%d:%d:trace:%s' % (img_h, img_w, size, name)]
        for sampler in (vr.sample_train, pkg.engine.input.sample_multiscale_crop):
            nprnd, rnd = np.random.RandomState(seed), random.Random(seed)
            got = [sampler(img_h, img_w, size, nprnd, rnd, more_fix_crop=more) for _ in range(len(trace))]
            assert np.array_equal(np.array([(p['cw'], p['ch'], p['x0'], p['y0']) for p in got]), trace)
            assert np.array_equal(np.array([p['flip'] for p in got]), gold['flip:trace'])
            for p in got:
                vr.check_box(p, img_h, img_w)
    assert len(set(map(tuple, gold['%dx%d:%d:trace:more' % (img_h, img_w, size)]))) > 8       # the traces do vary
    assert gold['flip:trace'].any() and not gold['flip:trace'].all()


def test_sample_train_without_fix_crop_draws_width_first():
    """fix_crop off is restated from the source (:428-430), not pinned: randint(0, img_w - w), then randint(0, img_h - h)."""
    class Rec(object):
        def __init__(self):
            self.calls = []

        def randint(self, *a):
            self.calls.append(a)
            return 0 if len(a) == 1 else a[1] - 1
    r = Rec()
    p = vr.sample_train(128, 171, 112, r, random.Random(0), fix_crop=False)
    assert r.calls == [(10,), (0, 171 - 128), (0, 128 - 128)] and (p['x0'], p['y0'], p['cw'], p['ch']) == (42, -1, 128, 128)
    with pytest.raises(ValueError):
        vr.check_box(p, 128, 171)


@pytest.mark.parametrize('img_h,img_w,ch,cw', CROPS)
def test_test_layouts_equal_the_reference(gold, img_h, img_w, ch, cw):
    """Origins, truncation and emission order of the 5-crop and 3-crop layouts: the reference got 3 frames, so with
    test_clips = 3, T = 1 every record of test_layout must name the frame, origin and size of the array emitted at its place."""
    for name, crops in (('over', 5), ('full', 3)):
        want = gold['%dx%d:%dx%d:%s' % (img_h, img_w, ch, cw, name)]
        rec, taps = vr.test_layout(img_h, img_w, (img_h, img_w), (ch, cw), crops, 3, 1)
        assert rec.shape == (3 * crops, 8) and taps.shape == (1, img_h + img_w, 4)
        assert np.array_equal(rec[:, [1, 3, 4]], want[:, :3]) and (want[:, 3] == ch).all() and (want[:, 4] == cw).all()
        assert not rec[:, [0, 2, 5, 6, 7]].any()
    # the 10-crop layout (restated, not pinned): the 5-crop layout with every origin once more, flipped
    r5 = vr.test_layout(img_h, img_w, (img_h, img_w), (ch, cw), 5, 3, 1)[0]
    r10 = vr.test_layout(img_h, img_w, (img_h, img_w), (ch, cw), 10, 3, 1)[0].reshape(5, 2, 3, 8)
    plain, flipped = r10[:, 0].reshape(-1, 8), r10[:, 1].reshape(-1, 8).copy()
    assert np.array_equal(plain, r5) and (flipped[:, 5] == 1).all()
    flipped[:, 5] = 0
    assert np.array_equal(flipped, r5)


def test_center_crop_and_refusals():
    rec, _ = vr.test_layout(20, 30, (18, 27), (16, 12), 1, 2, 4)
    assert rec.tolist() == [[0, 0, 0, 1, 7, 0, 0, 0], [0, 4, 0, 1, 7, 0, 0, 0]]
    for crops in (0, 2, 4, 6, 20):
        with pytest.raises(ValueError):
            vr.test_layout(20, 30, (18, 27), 16, crops, 1, 2)
    with pytest.raises(ValueError):
        vr.test_layout(20, 30, (18, 27), 19, 5, 1, 2)


# ------------------------------------------------------------------------------------------------ the arithmetic
def _frames(seed, n, F, Hs, Ws):
    return np.random.RandomState(seed).randint(0, 256, size=(n, F, Hs, Ws, 3)).astype(np.uint8)


TRAIN_BOXES = [dict(y0=0, x0=3, ch=20, cw=20, flip=False), dict(y0=2, x0=11, ch=16, cw=16, flip=True),
               dict(y0=7, x0=0, ch=13, cw=13, flip=False)]


@pytest.mark.parametrize('H,W', [(16, 16), (14, 13)])
def test_training_record_is_augment_ref_identity_jitter(H, W):
    """A training view == augment_ref.augment_batch under the identity-jitter record of the same box and flip, bit for bit."""
    Hs, Ws, T = 20, 27, 2
    assert all((p['cw'], p['ch']) in vr.multiscale_pairs(Hs, Ws, 16) for p in TRAIN_BOXES)
    frames = _frames(3, 3, T, Hs, Ws)
    rec, taps = vr.pack_train(TRAIN_BOXES, Hs, Ws, H, W)
    got = vr.clip_views(frames, rec, taps, H, W, T, H, W)
    params = [[dict(ar.identity_params(p['y0'], p['x0'], 0, 0, p['flip']), ch=p['ch'], cw=p['cw'])] for p in TRAIN_BOXES]
    want = ar.augment_batch(frames[:, None], ar.pack(params, Hs, Ws, H, W), H, W)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    if H == 16:                                                                            # the 16 -> 16 box is the identity
        assert np.array_equal(taps[1, :16, 0], 2 + np.arange(16)) and not taps[1, :, 3].any()
    assert taps[2, :H, 1].max() == 7 + 13 - 1 and taps[2, H:, 1].max() == 13 - 1          # upscale: taps clamp at the box edge


@pytest.mark.parametrize('crops', [1, 3, 5, 10])
def test_a_crop_of_the_resized_frame_is_a_window_of_its_taps(crops):
    """The sentence test mode rests on: resize the whole frame, crop (and flip) the uint8 result, normalise == clip_views."""
    Hs, Ws, T, clips = 20, 30, 2, 2
    frames = _frames(4, 2, clips * T, Hs, Ws)
    rec1, taps = vr.test_layout(Hs, Ws, (18, 27), (16, 12), crops, clips, T)
    rec = vr.tile_videos(rec1, 2)
    got = vr.clip_views(frames, rec, taps, 18, 27, T, 16, 12)
    assert got.shape == (2 * len(rec1), 3, T, 16, 12)
    full = [[ar.resize(f, taps[0, :18], taps[0, 18:]) for f in video] for video in frames]
    for v, (src, t0, _, oy, ox, flip, _, _) in enumerate(rec):
        want = oinput.make_view(np.stack(full[src][t0:t0 + T]), oy, ox, bool(flip), 16, 12)
        assert torch.equal(got[v], want), v
    assert sorted(set(rec[:, 1])) == [0, 2] and sorted(set(rec[:, 0])) == [0, 1]


# ------------------------------------------------------------------------------------------------ the product's host layer
def test_product_layouts_and_tables_equal_views_ref(pkg):
    inp = pkg.engine.input
    for crops in (1, 3, 5, 10):
        for scale, crop in (((18, 27), (16, 16)), ((18, 27), (16, 12)), (128, 112), ((128, 171), 112)):
            a, b = vr.test_layout(20, 30, scale, crop, crops, 2, 2), inp.test_view_layout(20, 30, scale, crop, crops, 2, 2)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].dtype == b[0].dtype and a[1].dtype == b[1].dtype
    H, W = vr._pair((16, 12))
    rec, taps, Lh = inp.pack_views(dict(scale_size=(18, 27), test_crops=10, test_clips=2), 3, 4, 20, 30, 2, H, W)
    r1, t1 = vr.test_layout(20, 30, (18, 27), (16, 12), 10, 2, 2)
    assert Lh == 18 and np.array_equal(rec, vr.tile_videos(r1, 3)) and np.array_equal(taps, t1) and rec.dtype == np.int32
    for H, W in ((16, 16), (14, 13)):
        rec, taps, Lh = inp.pack_views(TRAIN_BOXES, 3, 2, 20, 27, 2, H, W)
        r, t = vr.pack_train(TRAIN_BOXES, 20, 27, H, W)
        assert Lh == H and np.array_equal(rec, r) and np.array_equal(taps, t) and taps.dtype == np.int16
    # in place, into buffers the caller owns
    out = (np.full((3, 8), 9, np.int32), np.full((3, 27, 4), 9, np.int16))
    rec2, taps2, _ = inp.pack_views(TRAIN_BOXES, 3, 2, 20, 27, 2, 14, 13, out=out)
    assert rec2 is out[0] and taps2 is out[1] and np.array_equal(out[0], rec) and np.array_equal(out[1], taps)


def test_pack_views_refusals(pkg):
    inp = pkg.engine.input
    Hs, Ws, T, H, W = 20, 27, 2, 16, 16
    rec, taps, Lh = inp.pack_views(TRAIN_BOXES, 3, T, Hs, Ws, T, H, W)

    def refused(r=rec, t=taps, F=T, lh=Lh):
        with pytest.raises(ValueError):
            inp.pack_views((r, t, lh), 3, F, Hs, Ws, T, H, W)
    inp.pack_views((rec, taps, Lh), 3, T, Hs, Ws, T, H, W)              # the tables as they are pass
    for idx, val in (((0, 0, 0), Hs), ((0, 3, 1), -1), ((1, H, 0), Ws), ((2, H + W - 1, 1), Ws)):
        t = taps.copy()
        t[idx] = val
        refused(t=t)                                                     # taps outside the frame
    for word, val in ((3, 1), (4, 1), (3, -1), (4, -1)):
        r = rec.copy()
        r[1, word] = val
        refused(r=r)                                                     # a window outside the table
    refused(lh=H + 1)
    r = rec.copy()
    r[2, 1] = 1
    refused(r=r)                                                         # t0 + T > F
    refused(F=T - 1)
    for word, val in ((0, 3), (0, -1), (2, 3), (5, 2)):
        r = rec.copy()
        r[0, word] = val
        refused(r=r)                                                     # source / table / flip
    with pytest.raises(ValueError):
        inp.pack_views(dict(scale_size=(18, 27), test_crops=10, test_clips=3), 2, 4, 20, 30, 2, 16, 16)     # 3 clips of 2 > F = 4
    for crops in (0, 2, 4, 7):
        with pytest.raises(ValueError):
            inp.pack_views(dict(scale_size=(18, 27), test_crops=crops, test_clips=2), 2, 4, 20, 30, 2, 16, 16)   # unsupported test_crops
        with pytest.raises(ValueError):
            inp.test_view_layout(20, 30, (18, 27), 16, crops, 2, 2)
    with pytest.raises(ValueError):
        inp.pack_views([dict(TRAIN_BOXES[0], y0=1)] + TRAIN_BOXES[1:], 3, T, Hs, Ws, T, H, W)              # crop box outside the frame
    with pytest.raises(ValueError):
        inp.pack_views(TRAIN_BOXES[:2], 3, T, Hs, Ws, T, H, W)


def test_entry_refuses_before_it_touches_a_device(pkg):
    """gca_clip_views validates sizes and the HOST copy of the records before anything is launched, so its refusals can be
    exercised here, on host buffers (tests/test_gpu_views.py repeats them with a sentinel-filled output on the device)."""
    lib = pkg._hip.lib
    Hs, Ws, Lh, Lw, T, H, W = 20, 30, 18, 27, 2, 16, 16
    rec1, taps = vr.test_layout(Hs, Ws, (Lh, Lw), (H, W), 10, 2, T)
    rec = vr.tile_videos(rec1, 2)
    frames = _frames(5, 2, 2 * T, Hs, Ws)
    out = np.full((len(rec), 3, T, H, W), 77.0, dtype=np.float32)
    m, d = pkg.engine.input.normalize_constants((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    base = dict(n_src=2, F=2 * T, Hs=Hs, Ws=Ws, n_views=len(rec), n_tab=1, Lh=Lh, Lw=Lw, T=T, H=H, W=W)

    def entry(r=rec, **kw):
        a = dict(base, **kw)
        r = np.ascontiguousarray(r, dtype=np.int32)
        return lib.gca_clip_views(frames.ctypes.data, a['n_src'], a['F'], a['Hs'], a['Ws'], r.ctypes.data, r.ctypes.data, a['n_views'],
                                  taps.ctypes.data, a['n_tab'], a['Lh'], a['Lw'], m.ctypes.data, d.ctypes.data, a['T'], a['H'], a['W'],
                                  out.ctypes.data, None)
    for word, val in ((0, 2), (0, -1), (2, 1), (2, -1), (1, -1), (1, 3), (3, -1), (3, 3), (4, -1), (4, 12), (5, 2), (5, -1)):
        for view in (0, len(rec) - 1):
            r = rec.copy()
            r[view, word] = val
            assert entry(r) == -1, (word, val, view)
    for key in base:
        assert entry(**{key: -1}) == -1 and (key == 'n_views' or entry(**{key: 0}) == -1), key
    assert entry(F=T - 1) == -1 and entry(Lh=H - 1) == -1 and entry(Lw=W - 1) == -1 and entry(Hs=32768) == -1
    assert entry(T=65536, F=65536) == -1
    assert entry(n_src=2 ** 31 // (2 * T * Hs * Ws * 3) + 1) == -1 and entry(n_tab=2 ** 31 // ((Lh + Lw) * 4) + 1) == -1
    assert entry(n_views=2 ** 31 // 8) == -1 and entry(n_views=2 ** 31 // (3 * T * H * W) + 1) == -1 and entry(n_src=2 ** 62) == -1
    assert entry(n_views=0) == 0
    assert (out == 77.0).all()
