"""Video-level top-1 / top-5 / mean per-class accuracy of a fine-tuned model: the reference's tools/test_ds.py on the HIP
engine.  The model is built from the config as in training and takes the `state_dict` of an ActionTrainer checkpoint.  Two
inputs, one of which must be given:

--clips names a torch file holding {'data': (N, 3, clips * crops * T, H, W) float tensor, already normalised, 'label': (N,)
int tensor}, in the frame order of tools/test_ds.py:134-140 (per clip, `test_crops` runs of `video_length` frames): frame
decoding, resizing and cropping were a host transform.

--frames names a torch file holding {'frames': (N, F, Hs, Ws, 3) uint8 tensor of decoded frames, F = test_clips * T, 'label':
(N,) int tensor}: VideoResize(--scale_size), the --test_crops crops (1, 3, 5 or 10), their flips, the --test_clips temporal
clips and the normalisation (INPUT.MEAN / INPUT.STD) run on the device (engine.input.ActionInputStage, gca_clip_views), as
tools/test_ds.py:95-120 composes them on the host.  Only decoding stays with the host.

Needs a GPU: there is no fallback.

  python tools/action_eval.py --config_file cfg.yaml --weights checkpoint.pth.tar --clips val_clips.pt \\
      [--test_crops 3] [--softmax] [--batch_size 4] [--save_scores scores.npz] [KEY VALUE ...]
  python tools/action_eval.py --config_file cfg.yaml --weights checkpoint.pth.tar --frames val_frames.pt \\
      --scale_size 128 171 --input_size 112 --test_crops 10 --test_clips 10 [...]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def get_parser():
    ap = argparse.ArgumentParser(description='video-level action-recognition test')
    ap.add_argument('--config_file', default='', help='YAML merged over the defaults')
    ap.add_argument('--weights', required=True, help='checkpoint written by ActionTrainer.state_dict (torch.save)')
    ap.add_argument('--clips', default=None, help='torch file with data / label: finished fp32 views (see the module docstring)')
    ap.add_argument('--frames', default=None, help='torch file with frames / label: decoded uint8 frames (see the module docstring)')
    ap.add_argument('--scale_size', type=int, nargs='+', default=None, help='--frames: VideoResize size, one int or H W')
    ap.add_argument('--input_size', type=int, nargs='+', default=None, help='--frames: crop size, one int or H W (default INPUT.CROP_SIZE)')
    ap.add_argument('--test_clips', type=int, default=1, help='--frames: temporal clips per video')
    ap.add_argument('--test_crops', type=int, default=1)
    ap.add_argument('--video_length', type=int, default=0, help='frames per view (0: INPUT.VIDEO_LENGTH)')
    ap.add_argument('--batch_size', type=int, default=0, help='videos per forward (0: TEST.BATCH_SIZE)')
    ap.add_argument('--softmax', action='store_true', default=False, help='softmax of the mean logits')
    ap.add_argument('--save_scores', default=None, help='.npz receiving scores and labels')
    ap.add_argument('opts', nargs=argparse.REMAINDER, default=None, help='KEY VALUE config overrides')
    return ap


def _size(v):
    return v[0] if len(v) == 1 else (v[0], v[1])


def frame_batches(pkg, cfg, a, bs, T, dev):
    """(StagedBatch, labels) pairs from a --frames file: one ActionInputStage per batch size (the last batch may be short), each
    batch staged when it is asked for, so at most one is in flight per stage."""
    blob = torch.load(a.frames, map_location='cpu', weights_only=False)
    frames, label = torch.as_tensor(blob['frames']), torch.as_tensor(blob['label']).reshape(-1)
    if frames.dtype is not torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3 or frames.shape[1] != a.test_clips * T:
        raise SystemExit('--frames: (N, test_clips * T = %d, Hs, Ws, 3) uint8 frames expected, got %s %r'
                         % (a.test_clips * T, frames.dtype, tuple(frames.shape)))
    if a.scale_size is None:
        raise SystemExit('--frames needs --scale_size')
    crop = _size(a.input_size if a.input_size else [int(v) for v in cfg.INPUT.CROP_SIZE])
    stages = {}
    for i in range(0, frames.shape[0], bs):
        f = frames[i:i + bs].contiguous()
        if f.shape[0] not in stages:
            stages[f.shape[0]] = pkg.engine.input.ActionInputStage(
                f.shape[0], f.shape[1], tuple(f.shape[2:4]), crop, dev, mode='test', scale_size=_size(a.scale_size),
                test_crops=a.test_crops, test_clips=a.test_clips, T=T, mean=tuple(cfg.INPUT.MEAN), std=tuple(cfg.INPUT.STD))
        yield stages[f.shape[0]].stage(f), label[i:i + bs]


def main(argv=None):
    ap = get_parser()
    a = ap.parse_args(argv)
    if (a.clips is None) == (a.frames is None):
        ap.error('exactly one of --clips and --frames is required')
    pkg = importlib.import_module('video-graph-ssl_amd')
    cfg = pkg.get_defaults()
    if a.config_file:
        cfg.merge_from_file(a.config_file)
    cfg.merge_from_list(a.opts or [])
    dev = torch.device('cuda:0')
    model = pkg.create_video_model(cfg)
    ckpt = torch.load(a.weights, map_location='cpu', weights_only=False)
    model.load_state_dict(ckpt['state_dict'])
    model.to(dev).eval()
    bs = a.batch_size or int(cfg.TEST.BATCH_SIZE)
    T = a.video_length or int(cfg.INPUT.VIDEO_LENGTH)
    if a.clips is not None:
        blob = torch.load(a.clips, map_location='cpu', weights_only=False)
        data, label = blob['data'], torch.as_tensor(blob['label']).reshape(-1)
        batches = ((data[i:i + bs], label[i:i + bs]) for i in range(0, data.shape[0], bs))
    else:
        batches = frame_batches(pkg, cfg, a, bs, T, dev)
    res = pkg.lib.evaluation.classify.evaluate(model, batches, a.test_crops, T, softmax=a.softmax, device=dev)
    print('-----Evaluation is finished------')
    print('Accuracy {:.02f}%'.format(res['mean_class_acc'] * 100))
    print('Overall Prec@1 {:.02f}% Prec@5 {:.02f}%'.format(res['top1'], res['top5']))
    if a.save_scores is not None:
        np.savez(a.save_scores, scores=res['scores'], labels=res['labels'])
    return res


if __name__ == '__main__':
    main()
