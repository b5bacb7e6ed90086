"""Device-side contrastive augmentations (gca_clip_augment + engine.input.clip_augment / DeviceInputStage(augment=True))
against tests/augment_ref.py.  The specification is integer / fixed-point arithmetic and fp32 with one rounding per written
operation, so the bar is BIT-EXACT for fp32 output and one fp16 rounding of the exact fp32 value for fp16 output, as for
test_gpu_input.py.  (The specification itself is NOT checked against cv2 / albumentations: neither is available.)"""
import functools
import random

import numpy as np
import pytest
import torch

import augment_ref as ar
import parity

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _p(y0, x0, ch, cw, perm=(0, 1, 2, 3), b=1.0, c=1.0, s=1.0, h=0.0, jitter=True, gray=False, k=0, sigma=0.0, flip=False):
    return dict(y0=y0, x0=x0, ch=ch, cw=cw, jitter=jitter, perm=perm, brightness=b, contrast=c, saturation=s, hue=h, gray=gray,
                k=k, sigma=sigma, flip=flip)


def _frames(seed, b, views, T, Hs, Ws):
    return np.random.RandomState(seed).randint(0, 256, size=(b, views, T, Hs, Ws, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (frames, params, (Hs, Ws, H, W), reference fp32 batch); each reference is computed once and shared."""
    if name == 'all_on':
        # every stage on; crop boxes on the top / left and the bottom / right borders, an upscaling crop (10 x 12 -> 16 x 24),
        # the full frame; contrast first, last, in the middle and absent; factors at the ends of the reference's ranges;
        # k = 3, 5, 7; gray on and off; flip on and off; an all-0 and an all-255 frame (look-up table and clamp edges)
        geo = (40, 56, 16, 24)
        frames = _frames(11, 2, 2, 3, 40, 56)
        frames[0, 0, 0] = 0
        frames[0, 1, 1] = 255
        frames[1, 1, 2, :, :28] = (255, 0, 0)
        params = [[_p(0, 0, 30, 40, (1, 0, 2, 3), 0.6, 1.4, 0.6, 0.1, k=3, sigma=0.5, flip=True),
                   _p(20, 26, 20, 30, (0, 2, 3, 1), 1.4, 0.6, 1.4, -0.1, gray=True, k=5, sigma=2.0)],
                  [_p(15, 20, 10, 12, (3, 1, 2, 0), 1.4, 1.0, 0.6, -0.1, k=7, sigma=1.0, flip=True),
                   _p(0, 0, 40, 56, (2, 3, 0, 1), 0.6, 0.6, 1.4, 0.1, k=7, sigma=2.0)]]
    elif name == 'ragged':
        # W = 11: scalar stores and a ragged last column group; 9 x 11 output under k = 7: the window reaches past both
        # borders of a row of the tile at once
        geo = (13, 17, 9, 11)
        frames = _frames(12, 2, 1, 2, 13, 17)
        params = [[_p(1, 2, 12, 15, (2, 0, 1, 3), 1.2, 1.4, 0.8, 0.05, k=7, sigma=2.0, flip=True)],
                  [_p(0, 0, 13, 17, jitter=False, gray=True, k=7, sigma=0.7)]]
    elif name == 'identity':
        geo = (8, 8, 8, 8)
        frames = _frames(13, 1, 2, 2, 8, 8)
        params = [[ar.identity_params(0, 0, 8, 8), ar.identity_params(0, 0, 8, 8, 1)]]
    elif name == 'reference_geometry':
        geo = (128, 171, 112, 112)
        frames = _frames(14, 4, 2, 8, 128, 171)
        params = ar.sample_batch(4, 2, 128, 171, random.Random(5), np.random.RandomState(5))
        # (seed 5 draws jitter, gray, blur and flip each at least once over the eight records; checked below)
    Hs, Ws, H, W = geo
    want = ar.augment_batch(frames, ar.pack(params, Hs, Ws, H, W), H, W, MEAN, STD)
    return frames, params, geo, want


def _run(pkg, name, out_dtype=torch.float32):
    inp = pkg.engine.input
    frames, params, (Hs, Ws, H, W), want = _case(name)
    m, d = inp.normalize_constants(MEAN, STD)
    tables = inp.pack_augment(params, Hs, Ws, H, W)
    got = inp.clip_augment(torch.from_numpy(frames).to(DEV), tables, m, d, H, W, out_dtype=out_dtype)
    b, views, T = frames.shape[:3]
    assert got.dtype is out_dtype and tuple(got.shape) == (b, 3 * views, T, H, W)
    return got, want


@pytest.mark.parametrize('name', ['all_on', 'ragged', 'identity', 'reference_geometry'])
def test_clip_augment_bit_exact_vs_reference(pkg, name):
    got, want = _run(pkg, name)
    bad = (got.cpu() != want)
    print('%s: %d of %d values differ' % (name, int(bad.sum()), bad.numel()))
    assert torch.equal(got.cpu(), want)                                       # bit for bit
    if name == 'reference_geometry':
        params = [p for clip in _case(name)[1] for p in clip]
        assert any(p['jitter'] for p in params) and any(p['gray'] for p in params) and any(p['k'] for p in params)
        assert any(p['flip'] for p in params) and not all(p['flip'] for p in params)


def test_clip_augment_fp16_is_one_rounding(pkg):
    got, want = _run(pkg, 'all_on', torch.float16)
    assert torch.equal(got.cpu(), want.half())                                # the exact fp32 value, rounded once
    got, want = _run(pkg, 'ragged', torch.float16)
    assert torch.equal(got.cpu(), want.half())


def test_identity_record_is_clip_prepare(pkg):
    inp = pkg.engine.input
    got, want = _run(pkg, 'identity')
    frames = _case('identity')[0]
    m, d = inp.normalize_constants(MEAN, STD)
    prm = torch.tensor([[[0, 0, 0, 0], [0, 0, 1, 0]]], dtype=torch.int32, device=DEV)
    assert torch.equal(got, inp.clip_prepare(torch.from_numpy(frames).to(DEV), prm, m, d, 8, 8))
    # and with a crop window, ragged width and an fp16 result
    f = _frames(15, 2, 2, 2, 13, 17)
    prm = torch.tensor([[[1, 2, 0, 0], [4, 6, 1, 0]], [[0, 0, 1, 0], [3, 1, 0, 0]]], dtype=torch.int32)
    params = [[ar.identity_params(*[int(x) for x in prm[n, v, :2]], 9, 11, int(prm[n, v, 2])) for v in range(2)] for n in range(2)]
    for dt in (torch.float32, torch.float16):
        a = inp.clip_augment(torch.from_numpy(f).to(DEV), inp.pack_augment(params, 13, 17, 9, 11), m, d, 9, 11, out_dtype=dt)
        assert torch.equal(a, inp.clip_prepare(torch.from_numpy(f).to(DEV), prm.to(DEV), m, d, 9, 11, out_dtype=dt))


def test_two_calls_give_the_same_bits(pkg):
    """The per-frame gray sums of the contrast op are integer atomics: any arrival order gives the same sum."""
    inp = pkg.engine.input
    frames, params, (Hs, Ws, H, W), want = _case('reference_geometry')
    m, d = inp.normalize_constants(MEAN, STD)
    tables = inp.pack_augment(params, Hs, Ws, H, W)
    assert (tables[0][..., 11] & 2).any()                                     # some record does have a contrast op
    f = torch.from_numpy(frames).to(DEV)
    ws = torch.full((int(pkg._hip.lib.gca_clip_augment_ws_bytes(4, 2, 8)),), 0xA5, dtype=torch.uint8, device=DEV)
    a = inp.clip_augment(f, tables, m, d, H, W, ws=ws)                        # a dirty workspace: the entry clears what it uses
    b = inp.clip_augment(f, tables, m, d, H, W, ws=ws)
    assert torch.equal(a, b) and torch.equal(a.cpu(), want)


def test_trainer_consumes_staged_source_frames(pkg):
    """DeviceInputStage(augment=True) -> train_step(StagedBatch) == train_step on the reference-computed batch, bit for bit,
    over enough steps to wrap the two slots and to run eager, capture and replay."""
    parity.register_tiny(pkg)
    b, T, Hs, Ws, S = 8, 8, 40, 56, 48
    rnd, nprnd = random.Random(9), np.random.RandomState(9)
    batches = [(_frames(20 + i, b, 2, T, Hs, Ws), ar.sample_batch(b, 2, Hs, Ws, rnd, nprnd)) for i in range(4)]
    shs = [torch.randperm(b, generator=torch.Generator().manual_seed(i)) for i in range(4)]

    def make():
        return pkg.MoCoTrainer(parity.make_cfg(pkg, 'R2P1D10T', 'moco', 32, 64, T), DEV, use_graph=True, seed=4)
    ref, tr = make(), make()
    stage = pkg.engine.input.DeviceInputStage(b, T, (Hs, Ws), S, DEV, augment=True)
    assert stage.out_shape() == (b, 6, T, S, S)
    nxt = stage.stage(*batches[0])
    for i, (frames, params) in enumerate(batches):
        cur = nxt
        if i + 1 < len(batches):
            nxt = stage.stage(*batches[i + 1])                   # batch i+1 is copied while step i runs
        o1 = tr.train_step(cur, shuffle_ids=shs[i])
        want = ar.augment_batch(frames, ar.pack(params, Hs, Ws, S, S), S, S)
        o2 = ref.train_step(want.to(DEV), shuffle_ids=shs[i])
        assert torch.equal(o1['loss'], o2['loss']), i
        assert torch.equal(o1['logits'], o2['logits']) and torch.equal(o1['q'], o2['q']), i
    assert torch.equal(tr.arena_q.flat, ref.arena_q.flat)
    assert tr._segments[0].graph is not None
    with pytest.raises(ValueError):
        bad = [list(clip) for clip in batches[0][1]]
        bad[0][0] = dict(bad[0][0], y0=Hs)                       # crop box outside the frame
        stage.stage(batches[0][0], bad)
    tr.close(); ref.close()


def test_bad_geometry_is_refused(pkg):
    """ValueError from the host wrappers, GCA_EINVAL from the entry itself (it validates the host copy of the records before
    anything is launched)."""
    inp, lib = pkg.engine.input, pkg._hip.lib
    Hs, Ws, H, W = 13, 17, 9, 11
    f = torch.from_numpy(_frames(16, 1, 1, 2, Hs, Ws)).to(DEV)
    m, d = inp.normalize_constants(MEAN, STD)
    rec, taps, luts = inp.pack_augment([[_p(1, 2, 10, 12, (2, 0, 1, 3), 1.2, 1.4, 0.8, 0.05, k=5, sigma=1.0)]], Hs, Ws, H, W)
    drec, dtaps, dluts = (torch.from_numpy(a).to(DEV) for a in (rec, taps, luts))
    div = torch.from_numpy(inp.hsv_div_tables()).to(DEV)
    ws = torch.zeros(int(lib.gca_clip_augment_ws_bytes(1, 1, 2)), dtype=torch.uint8, device=DEV)
    out = torch.zeros((1, 3, 2, H, W), device=DEV)

    def entry(r):
        return lib.gca_clip_augment(f.data_ptr(), 1, 1, 2, Hs, Ws, r.ctypes.data, drec.data_ptr(), dtaps.data_ptr(),
                                    dluts.data_ptr(), div.data_ptr(), m.ctypes.data, d.ctypes.data, H, W, out.data_ptr(), 0,
                                    ws.data_ptr(), pkg._hip.stream())
    assert lib.gca_clip_augment_ws_bytes(1, 1, 2) == 8
    assert entry(rec) == 0
    for word, val in ((0, 4), (1, -1), (3, 18), (2, 0),            # crop box outside the frame / empty
                      (6, 4), (6, 9), (6, 1),                      # k not in {0, 3, 5, 7}
                      (8, 2), (10, 4)):                            # perm not a permutation
        r = rec.copy()
        r[0, 0, word] = val
        assert entry(r) == -1, (word, val)                         # GCA_EINVAL
        with pytest.raises(ValueError):
            inp.clip_augment(f, (r, taps, luts), m, d, H, W)
    torch.cuda.synchronize()
    assert torch.equal(out, inp.clip_augment(f, (rec, taps, luts), m, d, H, W))      # the refused calls wrote nothing
    with pytest.raises(RuntimeError):
        inp.clip_augment(f.cpu(), (rec, taps, luts), m, d, H, W)                     # host frames: no CPU fallback
    with pytest.raises(ValueError):
        inp.clip_augment(f, (rec, taps[:, :, :-1], luts), m, d, H, W)
