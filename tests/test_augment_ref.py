"""tests/augment_ref.py (the numpy specification of gca_clip_augment) against facts that can be checked by hand, and the
product's host side (engine.input: sampler, table packing) against it.  No GPU.  Nothing here compares with cv2 or
albumentations: neither is available, and the specification does not claim their bits."""
import random

import numpy as np
import pytest
import torch

import augment_ref as ar
from oracle import input as oinput


def _frames(seed, *shape):
    return np.random.RandomState(seed).randint(0, 256, size=shape + (3,)).astype(np.uint8)


def test_identity_record_is_make_batch():
    b, views, T, Hs, Ws, H, W = 2, 2, 2, 13, 17, 9, 11
    rng = np.random.RandomState(0)
    frames = _frames(1, b, views, T, Hs, Ws)
    params = np.zeros((b, views, 4), dtype=np.int32)
    params[..., 0] = rng.randint(0, Hs - H + 1, size=(b, views))
    params[..., 1] = rng.randint(0, Ws - W + 1, size=(b, views))
    params[..., 2] = [[0, 1], [1, 0]]
    recs = [[ar.identity_params(int(params[n, v, 0]), int(params[n, v, 1]), H, W, int(params[n, v, 2])) for v in range(views)]
            for n in range(b)]
    for mean, std in (((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), ((0.5, 0.45, 0.4), (0.25, 0.3, 0.2))):
        got = ar.augment_batch(frames, ar.pack(recs, Hs, Ws, H, W), H, W, mean, std)
        assert torch.equal(got, oinput.make_batch(frames, params, H, W, mean, std))


def test_resize_facts():
    img = _frames(2, 20, 30)
    # crop == output size: the crop itself (every tap has weight 2048 on its first index)
    t = ar.resize_taps(3, 9, 9, 20), ar.resize_taps(5, 11, 11, 30)
    assert np.array_equal(ar.resize(img, *t), img[3:12, 5:16])
    for taps in t:
        assert (taps[:, 2] == 2048).all() and (taps[:, 3] == 0).all()
    # a constant image stays constant, down- and up-scaling, for every value that can round badly
    for crop, out in ((20, 7), (4, 13), (17, 16)):
        ty, tx = ar.resize_taps(0, crop, out, 20), ar.resize_taps(2, crop, out, 30)
        assert (ty[:, 2] + ty[:, 3] == 2048).all() and ty[:, :2].min() >= 0 and ty[:, :2].max() < crop
        assert tx[:, :2].min() >= 2 and tx[:, :2].max() < 2 + crop                       # clamped to the crop box
        for val in (0, 1, 127, 128, 254, 255):
            assert (ar.resize(np.full((20, 30, 3), val, np.uint8), ty, tx) == val).all()
    # 2 -> 4 upscaling with half-pixel centres: src = -0.25, 0.25, 0.75, 1.25 -> weights of the second sample 0, 1/4, 3/4, 0
    assert ar.resize_taps(0, 2, 4, 2).tolist() == [[0, 1, 2048, 0], [0, 1, 1536, 512], [0, 1, 512, 1536], [1, 1, 2048, 0]]
    line = np.zeros((1, 2, 3), np.uint8)
    line[0, 1] = 200
    assert ar.resize(line, ar.resize_taps(0, 1, 1, 1), ar.resize_taps(0, 2, 4, 2))[0, :, 0].tolist() == [0, 50, 150, 200]


def test_blur_facts():
    for k in (3, 5, 7):
        for sigma in (0.1, 0.5, 1.0, 2.0, 1.234567):
            w = ar.blur_weights(k, sigma)
            assert w.sum() == 1 << ar.BLUR_SHIFT and w.min() >= 0 and np.array_equal(w, w[::-1]) and w.argmax() == k // 2
            for val in (0, 1, 128, 255):
                assert (ar.gaussian_blur(np.full((5, 6, 3), val, np.uint8), w) == val).all()
    assert ar.blur_weights(3, 0.1).tolist() == [0, 4096, 0]                              # a very narrow Gaussian: identity
    # reflect-101 on a plane smaller than the window: index -1 -> 1, n -> n - 2
    img = np.zeros((4, 4, 3), np.uint8)
    img[0, 0] = 255
    w = np.array([0, 0, 0, 0, 0, 0, 4096], dtype=np.int32)                               # picks the sample 3 to the right / below
    assert ar.gaussian_blur(img, w)[..., 0].tolist() == [[0, 0, 0, 0]] * 3 + [[0, 0, 0, 255]]
    w = np.array([4096, 0, 0, 0, 0, 0, 0], dtype=np.int32)                               # 3 to the left / above: (3,3) <- (0,0)
    assert ar.gaussian_blur(img, w)[3, 3, 0] == 255 and ar.gaussian_blur(img, w)[1, 1, 0] == 0


def test_colour_facts():
    div = ar.hsv_div_tables()
    v = np.arange(256, dtype=np.uint8)
    grays = np.stack([v, v, v], axis=-1)[None]
    assert np.array_equal(ar.gray_of(grays)[0], v)                                       # gray of (v, v, v) is v
    assert np.array_equal(ar.to_gray(grays), grays)
    assert 4899 + 9617 + 1868 == 1 << 14
    # saturated primaries and secondaries: H = 0, 60, 120 (and 30, 90, 150), S = V = 255, and back exactly
    prim = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]]], np.uint8)
    h, s, val = ar.rgb_to_hsv(prim, div)
    assert h[0].tolist() == [0, 60, 120, 30, 90, 150] and (s == 255).all() and (val == 255).all()
    assert np.array_equal(ar.hsv_to_rgb(h, s, val), prim)
    assert np.array_equal(ar.adjust_hue(prim, ar.hue_lut(0.0), div), prim)
    # a third of a turn moves red to green to blue to red
    assert np.array_equal(ar.adjust_hue(prim[:, :3], ar.hue_lut(1.0 / 3.0), div), prim[:, [1, 2, 0]])
    # grays have no hue: any shift leaves them alone
    assert np.array_equal(ar.adjust_hue(grays, ar.hue_lut(0.1), div), grays)
    assert np.array_equal(ar.hue_lut(0.0)[:180], np.arange(180)) and ar.hue_lut(-0.1)[0] == 162 and ar.hue_lut(0.1)[179] == 17
    assert np.array_equal(ar.brightness_lut(1.0), v) and ar.brightness_lut(1.4)[200] == 255 and ar.brightness_lut(0.6)[255] == 153
    img = _frames(3, 6, 7)
    one, zero = np.float32(1), np.float32(0)
    # the formulas at factor 1 happen to be identities too (the record leaves such ops out by definition)
    assert np.array_equal(ar.adjust_contrast(img, one, zero), img) and np.array_equal(ar.adjust_saturation(img, one, zero), img)
    # contrast 0: every channel becomes the truncated mean gray; saturation 0: the gray image
    mean = np.float32(int(ar.gray_of(img).sum())) * (one / np.float32(42))
    assert (ar.adjust_contrast(img, zero, one) == int(mean)).all()
    assert np.array_equal(ar.adjust_saturation(img, zero, one), ar.to_gray(img))
    assert (ar.adjust_contrast(np.full((3, 3, 3), 255, np.uint8), np.float32(1.4), one - np.float32(1.4)) == 255).all()


def test_factor_one_ops_are_left_out_and_change_nothing():
    Hs, Ws, H, W = 12, 14, 8, 10
    frames = _frames(4, 1, 1, 2, Hs, Ws)
    base = ar.identity_params(1, 2, H, W)
    same = dict(base, jitter=True, perm=(3, 1, 0, 2))                                    # jitter on, every factor neutral
    pk = ar.pack([[same]], Hs, Ws, H, W)
    assert pk[0][0, 0, 11] == 0
    assert torch.equal(ar.augment_batch(frames, pk, H, W), ar.augment_batch(frames, ar.pack([[base]], Hs, Ws, H, W), H, W))
    on = dict(same, brightness=1.4, contrast=0.6, saturation=1.4, hue=-0.1)
    assert ar.pack([[on]], Hs, Ws, H, W)[0][0, 0, 11] == 15
    off = dict(on, jitter=False)                                                         # VideoRandomApply said no
    assert ar.pack([[off]], Hs, Ws, H, W)[0][0, 0, 11] == 0
    assert not torch.equal(ar.augment_batch(frames, ar.pack([[on]], Hs, Ws, H, W), H, W), ar.augment_batch(frames, pk, H, W))


def _same(a, b):
    assert set(a) == set(b)
    for key in a:
        assert a[key] == b[key] and type(a[key]) is type(b[key]), key


@pytest.mark.parametrize('Hs,Ws,fallback', [(128, 171, False), (40, 56, False), (20, 200, True), (300, 30, True)])
def test_sampler_matches_product(pkg, Hs, Ws, fallback):
    inp = pkg.engine.input
    hit = {'jitter': 0, 'gray': 0, 'blur': 0, 'flip': 0, 'central': 0}
    for seed in range(40):
        r1, r2 = random.Random(seed), random.Random(seed)
        n1, n2 = np.random.RandomState(seed), np.random.RandomState(seed)
        for _ in range(3):                                    # consecutive draws: the two samplers consume the same stream
            a, b = ar.sample_params(Hs, Ws, r1, n1), inp.sample_augment(Hs, Ws, r2, n2)
            _same(a, b)
            ar.check_params(a, Hs, Ws, 16, 16)
            assert a['k'] in (0, 3, 5, 7) and sorted(a['perm']) == [0, 1, 2, 3]
            hit['jitter'] += a['jitter']; hit['gray'] += a['gray']; hit['blur'] += a['k'] > 0; hit['flip'] += a['flip']
            ci, cj = (Hs - a['ch']) // 2, (Ws - a['cw']) // 2        # (the fraction round trip of the origin may lose 1)
            hit['central'] += (a['ch'] == Hs or a['cw'] == Ws) and a['y0'] in (ci, ci - 1) and a['x0'] in (cj, cj - 1)
        assert r1.getstate() == r2.getstate()
    assert all(hit[key] for key in ('jitter', 'gray', 'blur', 'flip'))
    if fallback:
        # a frame this elongated admits no crop of an allowed aspect ratio and 20 % of the area: every draw ends in the
        # central crop, Hs x round(Hs * 4/3) or round(Ws * 4/3) x Ws
        assert hit['central'] == 120
        p = ar.sample_params(Hs, Ws, random.Random(0), np.random.RandomState(0))
        assert (p['ch'], p['cw']) == ((Hs, int(round(Hs * 4 / 3))) if Ws > Hs else (int(round(Ws / 0.75)), Ws))


def test_sampler_follows_the_reference_draw_order():
    """The first view of seed 0, replayed by hand with the draws the reference's classes make."""
    Hs, Ws = 128, 171
    r = random.Random(0)
    p = ar.sample_params(Hs, Ws, random.Random(0), np.random.RandomState(0))
    import math
    for _ in range(10):
        ta = r.uniform(0.2, 1.0) * Hs * Ws
        asp = math.exp(r.uniform(math.log(0.75), math.log(1.3333333333333333)))
        w, h = int(round(math.sqrt(ta * asp))), int(round(math.sqrt(ta / asp)))
        if 0 < w <= Ws and 0 < h <= Hs:
            i, j = r.randint(0, Hs - h), r.randint(0, Ws - w)
            break
    assert (p['ch'], p['cw']) == (h, w) and p['y0'] in (i, i - 1) and p['x0'] in (j, j - 1)
    assert p['y0'] == int((Hs - h) * (i * 1.0 / (Hs - h + 1e-10)))
    jit = r.random() < 0.8
    assert p['jitter'] == jit
    if jit:
        assert [p['brightness'], p['contrast'], p['saturation']] == [r.uniform(0.6, 1.4) for _ in range(3)]
        assert p['hue'] == r.uniform(-0.1, 0.1)
        order = [0, 1, 2, 3]
        r.shuffle(order)
        assert p['perm'] == tuple(order)


def test_product_tables_match_the_specification(pkg):
    inp = pkg.engine.input
    Hs, Ws, H, W = 128, 171, 112, 112
    rnd, nprnd = random.Random(7), np.random.RandomState(7)
    params = ar.sample_batch(6, 2, Hs, Ws, rnd, nprnd)
    params[0][0] = dict(params[0][0], jitter=True, brightness=1.0, contrast=1.0, saturation=1.4, hue=0.0)
    params[0][1] = ar.identity_params(3, 5, 20, 30, 1)                                     # upscaling identity colour
    want, got = ar.pack(params, Hs, Ws, H, W), inp.pack_augment(params, Hs, Ws, H, W)
    for a, b in zip(want, got):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(ar.hsv_div_tables(), inp.hsv_div_tables())
    _same(ar.identity_params(1, 2, 3, 4, 1), inp.augment_identity(1, 2, 3, 4, True))
    assert inp.AUG_REC == ar.REC
    # in-place packing into caller-owned buffers (the stage's pinned slot)
    out = tuple(np.full_like(a, 77) for a in want)
    inp.pack_augment(params, Hs, Ws, H, W, out=out)
    for a, b in zip(want, out):
        assert np.array_equal(a, b)


def test_bad_records_raise_on_the_host(pkg):
    inp = pkg.engine.input
    Hs, Ws, H, W = 20, 24, 8, 8
    ok = ar.identity_params(2, 3, 10, 12)
    inp.pack_augment([[ok]], Hs, Ws, H, W)
    for bad in (dict(ok, y0=11), dict(ok, x0=-1), dict(ok, cw=25), dict(ok, ch=0), dict(ok, k=4, sigma=1.0), dict(ok, k=9, sigma=1.0),
                dict(ok, perm=(0, 1, 2, 2)), dict(ok, perm=(0, 1, 2, 4))):
        with pytest.raises(ValueError):
            inp.pack_augment([[bad]], Hs, Ws, H, W)
        with pytest.raises(ValueError):
            ar.pack([[bad]], Hs, Ws, H, W)
    with pytest.raises(ValueError):
        inp.pack_augment([[dict(ok, k=7, sigma=1.0)]], Hs, Ws, 3, 8)                       # radius 3 needs more than 3 rows
    rec = inp.pack_augment([[dict(ok, k=5, sigma=1.0)]], Hs, Ws, H, W)[0]
    inp.check_augment_records(rec, Hs, Ws, H, W)
    for word, val in ((0, 11), (6, 6), (8, 0), (16, rec[0, 0, 16] + 1), (22, 1), (11, 16), (4, 2)):
        r = rec.copy()
        r[0, 0, word] = val
        with pytest.raises(ValueError):
            inp.check_augment_records(r, Hs, Ws, H, W)
