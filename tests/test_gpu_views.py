"""gca_clip_views, engine.input.clip_views / ActionInputStage and the staged paths of ActionTrainer / eval_video / evaluate
against tests/views_ref.py.  The specification is integer / fixed-point arithmetic followed by two fp32 roundings, so the bar
is BIT-EXACT everywhere (torch.equal on fp32), as in test_gpu_augment.py.  The shapes are the smallest that reach each path:
a downscale, an identity and an upscale whose taps clamp at the box edge; 16-byte stores (W = 16) and scalar stores (W = 13,
and W = 16 into an output that is not 16-byte aligned); windows that end exactly at the right and bottom edge of the tap
table; two temporal clips; more views than grid.z holds."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as ar                 # noqa: E402
import classify_model as cm              # noqa: E402
import classify_ref as cref              # noqa: E402
import views_ref as vr                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
EINVAL = -1
TRAIN_BOXES = [dict(y0=0, x0=3, ch=20, cw=20, flip=False), dict(y0=2, x0=11, ch=16, cw=16, flip=True),
               dict(y0=7, x0=0, ch=13, cw=13, flip=False)]


def _frames(seed, n, F, Hs, Ws):
    return np.random.RandomState(seed).randint(0, 256, size=(n, F, Hs, Ws, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (frames, records, taps, Lh, (T, H, W), reference fp32 views); each reference is computed once and shared."""
    if name in ('train16', 'train13'):
        # boxes from multiscale_pairs(20, 27, 16): 20 -> 16 down, 16 -> 16 identity (flipped), 13 -> 16 up (taps clamp at the box)
        assert all((p['cw'], p['ch']) in vr.multiscale_pairs(20, 27, 16) for p in TRAIN_BOXES)
        T, H, W = (2, 16, 16) if name == 'train16' else (2, 14, 13)
        frames = _frames(31, 3, T, 20, 27)
        rec, taps = vr.pack_train(TRAIN_BOXES, 20, 27, H, W)
        Lh = H
    else:
        crops, (H, W) = (10, (16, 16)) if name == 'test10' else (3, (16, 12))
        T = 2
        frames = _frames(32, 2, 2 * T, 20, 30)
        rec1, taps = vr.test_layout(20, 30, (18, 27), (H, W), crops, 2, T)
        rec, Lh = vr.tile_videos(rec1, 2), 18
        if name == 'test10':
            assert len(rec) == 40 and rec[:, 4].max() == 11 and rec[:, 3].max() == 2 and sorted(set(rec[:, 1])) == [0, 2]
            assert 11 + W == 27 and 2 + H == 18                       # windows end exactly at the right / bottom edge
    want = vr.clip_views(frames, rec, taps, Lh, taps.shape[1] - Lh, T, H, W, MEAN, STD)
    return frames, rec, taps, Lh, (T, H, W), want


def _consts(pkg):
    return pkg.engine.input.normalize_constants(MEAN, STD)


# ----------------------------------------------------------------------------- 1. bit-exact against views_ref
@pytest.mark.parametrize('name', ['train16', 'train13', 'test10', 'test3'])
def test_clip_views_bit_exact_vs_reference(pkg, name):
    inp = pkg.engine.input
    frames, rec, taps, Lh, (T, H, W), want = _case(name)
    m, d = _consts(pkg)
    got = inp.clip_views(torch.from_numpy(frames).to(DEV), (rec, taps, Lh), m, d, T, H, W)
    assert got.dtype is torch.float32 and tuple(got.shape) == (len(rec), 3, T, H, W)
    bad = got.cpu() != want
    print('%s: %d of %d values differ' % (name, int(bad.sum()), bad.numel()))
    assert torch.equal(got.cpu(), want)                                       # bit for bit


def test_clip_views_into_an_unaligned_output(pkg):
    """W % 4 == 0 but the output starts 4 bytes past a 16-byte boundary: the scalar-store kernel, same bits, no byte outside."""
    inp = pkg.engine.input
    frames, rec, taps, Lh, (T, H, W), want = _case('train16')
    m, d = _consts(pkg)
    buf = torch.full((want.numel() + 8,), 77.0, device=DEV)
    out = buf[1:1 + want.numel()].view(want.shape)
    assert out.data_ptr() % 16 == 4
    inp.clip_views(torch.from_numpy(frames).to(DEV), (rec, taps, Lh), m, d, T, H, W, out=out)
    assert torch.equal(out.cpu(), want) and float(buf[0]) == 77.0 and bool((buf[1 + want.numel():] == 77.0).all())


def test_more_views_than_grid_z(pkg):
    """n_views > 65535 folds into grid.x: 65544 views of 4 x 4 cycling over 12 records; the 12 are held to views_ref, the rest
    to the 12."""
    inp = pkg.engine.input
    T, H, W, Hs, Ws, Lh, Lw = 1, 4, 4, 6, 7, 5, 6
    frames = _frames(33, 2, 2, Hs, Ws)
    taps = np.stack([np.concatenate([ar.resize_taps(0, Hs, Lh, Hs), ar.resize_taps(0, Ws, Lw, Ws)]),
                     np.concatenate([ar.resize_taps(1, 4, Lh, Hs), ar.resize_taps(2, 5, Lw, Ws)])])
    r = np.random.RandomState(34)
    rec12 = np.zeros((12, 8), dtype=np.int32)
    rec12[:, 0], rec12[:, 1], rec12[:, 2] = r.randint(0, 2, 12), r.randint(0, 2, 12), r.randint(0, 2, 12)
    rec12[:, 3], rec12[:, 4], rec12[:, 5] = r.randint(0, Lh - H + 1, 12), r.randint(0, Lw - W + 1, 12), r.randint(0, 2, 12)
    want = vr.clip_views(frames, rec12, taps, Lh, Lw, T, H, W, MEAN, STD)
    n = 65535 + 9
    rec = np.tile(rec12, (n // 12 + 1, 1))[:n]
    m, d = _consts(pkg)
    f = torch.from_numpy(frames).to(DEV)
    small = inp.clip_views(f, (rec12, taps, Lh), m, d, T, H, W)
    assert torch.equal(small.cpu(), want)
    big = inp.clip_views(f, (rec, taps, Lh), m, d, T, H, W)
    assert tuple(big.shape) == (n, 3, T, H, W)
    idx = torch.arange(n, device=DEV) % 12
    assert torch.equal(big, small[idx])


# ----------------------------------------------------------------------------- 2. tied to gca_clip_augment
@pytest.mark.parametrize('name', ['train16', 'train13'])
def test_training_records_equal_clip_augment_identity(pkg, name):
    inp = pkg.engine.input
    frames, rec, taps, Lh, (T, H, W), want = _case(name)
    m, d = _consts(pkg)
    f = torch.from_numpy(frames).to(DEV)
    got = inp.clip_views(f, inp.pack_views(TRAIN_BOXES, 3, T, 20, 27, T, H, W), m, d, T, H, W)
    params = [[dict(inp.augment_identity(p['y0'], p['x0'], 0, 0, p['flip']), ch=p['ch'], cw=p['cw'])] for p in TRAIN_BOXES]
    old = inp.clip_augment(f[:, None].contiguous(), inp.pack_augment(params, 20, 27, H, W), m, d, H, W)
    assert torch.equal(got, old) and torch.equal(got.cpu(), want)


# ----------------------------------------------------------------------------- 3. the entry's refusals
def test_invalid_arguments_launch_nothing(pkg):
    lib, hip = pkg._hip.lib, pkg._hip
    frames, rec, taps, Lh, (T, H, W), want = _case('test10')
    n_src, F, Hs, Ws = frames.shape[:4]
    Lw, n_views = taps.shape[1] - Lh, len(rec)
    m, d = _consts(pkg)
    f, drec, dtaps = (torch.from_numpy(a).to(DEV) for a in (frames, rec, taps))
    out = torch.full((n_views, 3, T, H, W), 77.0, device=DEV)
    base = dict(n_src=n_src, F=F, Hs=Hs, Ws=Ws, n_views=n_views, n_tab=1, Lh=Lh, Lw=Lw, T=T, H=H, W=W)

    def entry(r=rec, **kw):
        a = dict(base, **kw)
        r = np.ascontiguousarray(r, dtype=np.int32)
        return lib.gca_clip_views(f.data_ptr(), a['n_src'], a['F'], a['Hs'], a['Ws'], r.ctypes.data, drec.data_ptr(), a['n_views'],
                                  dtaps.data_ptr(), a['n_tab'], a['Lh'], a['Lw'], m.ctypes.data, d.ctypes.data, a['T'], a['H'],
                                  a['W'], out.data_ptr(), hip.stream())

    def with_word(word, val, view=7):
        r = rec.copy()
        r[view, word] = val
        return r
    torch.cuda.synchronize()
    for word, val in ((0, n_src), (0, -1),                           # src outside [0, n_src)
                      (2, 1), (2, -1),                               # tab outside [0, n_tab)
                      (1, -1), (1, F - T + 1),                       # t0 < 0, t0 + T > F
                      (3, -1), (3, Lh - H + 1), (4, -1), (4, Lw - W + 1),     # a window outside the table
                      (5, 2), (5, -1)):                              # flip not 0 or 1
        assert entry(with_word(word, val)) == EINVAL, (word, val)
    assert entry(with_word(5, 3, view=n_views - 1)) == EINVAL        # the last record is read too
    for key in base:
        if key != 'n_views':
            assert entry(**{key: 0}) == EINVAL and entry(**{key: -1}) == EINVAL, key         # any size below 1
    assert entry(n_views=-1) == EINVAL
    assert entry(F=T - 1) == EINVAL and entry(Lh=H - 1) == EINVAL and entry(Lw=W - 1) == EINVAL
    # a tensor of 2^31 elements or more: frames, taps, records, out
    assert entry(n_src=2 ** 31 // (F * Hs * Ws * 3) + 1) == EINVAL
    assert entry(n_tab=2 ** 31 // ((Lh + Lw) * 4) + 1) == EINVAL
    assert entry(n_views=2 ** 31 // 8) == EINVAL
    assert entry(n_views=2 ** 31 // (3 * T * H * W) + 1) == EINVAL
    assert entry(Hs=32768) == EINVAL and entry(n_src=2 ** 40) == EINVAL
    assert entry(n_views=0) == 0                                     # nothing to do, nothing launched
    torch.cuda.synchronize()
    assert bool((out == 77.0).all())                                 # nothing was written
    assert entry() == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)
    inp = pkg.engine.input
    with pytest.raises(RuntimeError):
        inp.clip_views(f.cpu(), (rec, taps, Lh), m, d, T, H, W)                          # host frames: no CPU fallback
    with pytest.raises(ValueError):
        inp.clip_views(f, (with_word(4, Lw - W + 1), taps, Lh), m, d, T, H, W)
    bad = taps.copy()
    bad[0, Lh + 3, 1] = Ws
    with pytest.raises(ValueError):
        inp.clip_views(f, (rec, bad, Lh), m, d, T, H, W)                                 # a tap outside the frame: host check
    empty = inp.clip_views(f, (rec[:0], taps, Lh), m, d, T, H, W)
    assert tuple(empty.shape) == (0, 3, T, H, W)


# ----------------------------------------------------------------------------- 4. ActionInputStage, test mode
def test_stage_test_mode_two_batches_and_the_full_pipeline(pkg):
    inp = pkg.engine.input
    frames, rec, taps, Lh, (T, H, W), want = _case('test10')
    m, d = _consts(pkg)
    stage = inp.ActionInputStage(2, 2 * T, (20, 30), (H, W), DEV, mode='test', scale_size=(18, 27), test_crops=10, test_clips=2)
    assert stage.out_shape() == (40, 3, T, H, W) and stage.views == 20 and stage.T == T
    other = np.ascontiguousarray(frames[::-1])
    s1 = stage.stage(frames)
    s2 = stage.stage(torch.from_numpy(other))
    with pytest.raises(RuntimeError):
        stage.stage(frames)                                          # both slots hold batches that were not prepared
    with pytest.raises(RuntimeError):
        stage.acquire()
    o1 = stage.prepare(s1, torch.empty(stage.out_shape(), device=DEV))
    o2 = stage.prepare(s2, torch.empty(stage.out_shape(), device=DEV))
    d1 = inp.clip_views(torch.from_numpy(frames).to(DEV), (rec, taps, Lh), m, d, T, H, W)
    d2 = inp.clip_views(torch.from_numpy(other).to(DEV), (rec, taps, Lh), m, d, T, H, W)
    assert torch.equal(o1, d1) and torch.equal(o2, d2) and torch.equal(o1.cpu(), want) and not torch.equal(o1, o2)
    s3 = stage.stage(other)                                          # prepared slots are handed out again
    assert s3.slot == s1.slot and torch.equal(stage.prepare(s3, torch.empty(stage.out_shape(), device=DEV)), d2)
    with pytest.raises(ValueError):
        stage.stage(frames[:, :T])
    with pytest.raises(ValueError):
        inp.ActionInputStage(2, 2 * T, (20, 30), (H, W), DEV, mode='test', scale_size=(18, 27), test_crops=4, test_clips=2)


def test_stage_train_mode(pkg):
    inp = pkg.engine.input
    frames, rec, taps, Lh, (T, H, W), want = _case('train13')
    stage = inp.ActionInputStage(3, T, (20, 27), (H, W), DEV, mode='train')
    assert stage.out_shape() == (3, 3, T, H, W)
    out = stage.prepare(stage.stage(frames, TRAIN_BOXES), torch.empty(stage.out_shape(), device=DEV))
    assert torch.equal(out.cpu(), want)
    hf, tables = stage.acquire()                                     # the loader's path: fill the pinned buffers in place
    hf.copy_(torch.from_numpy(frames))
    inp.pack_views(TRAIN_BOXES, 3, T, 20, 27, T, H, W, out=tables)
    out2 = stage.prepare(stage.submit(), torch.empty(stage.out_shape(), device=DEV))
    assert torch.equal(out2.cpu(), want)
    with pytest.raises(ValueError):
        stage.stage(frames, [dict(TRAIN_BOXES[0], x0=8)] + TRAIN_BOXES[1:])          # crop box outside the frame


# ----------------------------------------------------------------------------- 5. / 6. trainer and video-level test
@pytest.fixture(scope='module')
def tiny(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    cm.register()
    return parity


def action_cfg(pkg, tiny):
    cfg = tiny.make_cfg(pkg, cm.BACKBONE, 'moco', 32, 20, cm.T)
    cfg.merge_from_list(['DATASET.NUM_CLASS', cm.NUM_CLASS, 'MODEL.DROPOUT', 0.0, 'MODEL.LINEAR_PROBE', False,
                         'SOLVER.NO_PARTIALBN', True])
    return cfg


STEP_LABELS = torch.tensor([0, 3, 6, 1, 2, 5, 4, 3])


def test_train_step_and_validate_on_staged_batches(pkg, tiny):
    import random
    inp = pkg.engine.input
    b, T, Hs, Ws, S = 8, cm.T, 56, 64, 48
    frames = _frames(41, b, T, Hs, Ws)
    rnd, nprnd = random.Random(7), np.random.RandomState(7)
    params = [vr.sample_train(Hs, Ws, S, nprnd, rnd) for _ in range(b)]
    assert len(set((p['cw'], p['ch']) for p in params)) > 2 and any(p['flip'] for p in params) and not all(p['flip'] for p in params)
    rec, taps = vr.pack_train(params, Hs, Ws, S, S)
    want = vr.clip_views(frames, rec, taps, S, S, T, S, S, MEAN, STD)
    a, ref = pkg.ActionTrainer(action_cfg(pkg, tiny), DEV, seed=41), pkg.ActionTrainer(action_cfg(pkg, tiny), DEV, seed=41)
    stage = inp.ActionInputStage(b, T, (Hs, Ws), S, DEV, mode='train')
    o1 = a.train_step(stage.stage(frames, params), STEP_LABELS)
    o2 = ref.train_step(want.to(DEV), STEP_LABELS)
    torch.cuda.synchronize()
    assert torch.equal(o1['loss'], o2['loss']) and torch.equal(o1['logits'], o2['logits']) and bool(torch.isfinite(o1['loss']).all())
    sa, sb = a.model.state_dict(), ref.model.state_dict()
    assert len(sa) == len(sb) > 100
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    # validation: the reference's VideoResize + VideoCenterCrop (build_transform_cv2(is_train=False)) = test mode, one view
    vstage = inp.ActionInputStage(4, T, (Hs, Ws), S, DEV, mode='test', scale_size=(52, 60), test_crops=1, test_clips=1)
    r1, t1 = vr.test_layout(Hs, Ws, (52, 60), S, 1, 1, T)
    vwant = vr.clip_views(frames, vr.tile_videos(r1, b), t1, 52, 60, T, S, S, MEAN, STD)
    staged = [(vstage.stage(frames[:4]), STEP_LABELS[:4]), (vstage.stage(frames[4:]), STEP_LABELS[4:])]
    got = a.validate(staged)
    exp = ref.validate([(vwant[:4], STEP_LABELS[:4]), (vwant[4:], STEP_LABELS[4:])])
    assert got == exp and got['count'] == 8 and a.model.training
    with pytest.raises(RuntimeError):
        a.train_step(torch.from_numpy(frames), STEP_LABELS)              # a host tensor is still refused


def test_eval_video_and_evaluate_on_staged_batches(pkg, tiny):
    inp, C = pkg.engine.input, pkg.lib.evaluation.classify
    torch.manual_seed(61)
    model = pkg.lib.modeling.VideoModelWrapper(cm.NUM_CLASS, cm.T, 'RGB', backbone_name=cm.BACKBONE, backbone_type='3D',
                                               dropout=0.0, partial_bn=False).to(DEV).eval()
    B, crops, clips, T, Hs, Ws, S = 2, 3, 2, cm.T, 56, 72, 48
    frames = [_frames(51, B, clips * T, Hs, Ws), _frames(52, B, clips * T, Hs, Ws)]
    r1, taps = vr.test_layout(Hs, Ws, (52, 64), S, crops, clips, T)
    views = len(r1)
    assert views == crops * clips

    def laid_out(f):
        """views_ref's (B * views, 3, T, S, S) -> the (B, 3, views * T, S, S) block split_views takes apart"""
        v = vr.clip_views(f, vr.tile_videos(r1, B), taps, 52, 64, T, S, S, MEAN, STD)
        return v.reshape(B, views, 3, T, S, S).permute(0, 2, 1, 3, 4, 5).reshape(B, 3, views * T, S, S).contiguous()
    data = [laid_out(f) for f in frames]
    stage = inp.ActionInputStage(B, clips * T, (Hs, Ws), S, DEV, mode='test', scale_size=(52, 64), test_crops=crops, test_clips=clips)
    got = C.eval_video(model, stage.stage(frames[0]), crops, T)
    want = C.eval_video(model, data[0].to(DEV), crops, T)
    assert got.shape == (B, cm.NUM_CLASS) and torch.equal(got, want)
    assert torch.equal(C.eval_video(model, stage.stage(frames[0]), crops, T, softmax=True),
                       C.eval_video(model, data[0].to(DEV), crops, T, softmax=True))
    labels = [torch.tensor([2, 5]), torch.tensor([2, 0])]
    res = C.evaluate(model, [(stage.stage(frames[0]), labels[0]), (stage.stage(frames[1]), labels[1])], crops, T, device=DEV)
    exp = C.evaluate(model, [(data[0], labels[0]), (data[1], labels[1])], crops, T, device=DEV)
    assert res['top1'] == exp['top1'] and res['top5'] == exp['top5'] and np.array_equal(res['confusion'], exp['confusion'])
    assert np.array_equal(res['scores'], exp['scores']) and np.array_equal(res['labels'], exp['labels'])
    assert np.array_equal(res['confusion'], cref.confusion(np.array([2, 5, 2, 0]), res['scores'].argmax(1), cm.NUM_CLASS))
    with pytest.raises(ValueError):
        C.eval_video(model, stage.stage(frames[0]), crops, T + 1)
    train_stage = inp.ActionInputStage(B, T, (Hs, Ws), S, DEV, mode='train')
    with pytest.raises(RuntimeError):
        C.eval_video(model, train_stage.stage(frames[0][:, :T], [dict(y0=0, x0=0, ch=56, cw=56, flip=False)] * B), crops, T)
