"""Video-level top-1 / top-5 / mean per-class accuracy of a fine-tuned model: the reference's tools/test_ds.py on the HIP
engine.  The model is built from the config as in training and takes the `state_dict` of an ActionTrainer checkpoint.  Frame
decoding, resizing and cropping stay a host transform: --clips names a torch file holding {'data': (N, 3, clips * crops * T,
H, W) float tensor, already normalised, 'label': (N,) int tensor}, in the frame order of tools/test_ds.py:134-140 (per clip,
`test_crops` runs of `video_length` frames).  Needs a GPU: there is no fallback.

  python tools/action_eval.py --config_file cfg.yaml --weights checkpoint.pth.tar --clips val_clips.pt \\
      [--test_crops 3] [--softmax] [--batch_size 4] [--save_scores scores.npz] [KEY VALUE ...]
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
    ap.add_argument('--clips', required=True, help='torch file with data / label (see the module docstring)')
    ap.add_argument('--test_crops', type=int, default=1)
    ap.add_argument('--video_length', type=int, default=0, help='frames per view (0: INPUT.VIDEO_LENGTH)')
    ap.add_argument('--batch_size', type=int, default=0, help='videos per forward (0: TEST.BATCH_SIZE)')
    ap.add_argument('--softmax', action='store_true', default=False, help='softmax of the mean logits')
    ap.add_argument('--save_scores', default=None, help='.npz receiving scores and labels')
    ap.add_argument('opts', nargs=argparse.REMAINDER, default=None, help='KEY VALUE config overrides')
    return ap


def main(argv=None):
    a = get_parser().parse_args(argv)
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
    blob = torch.load(a.clips, map_location='cpu', weights_only=False)
    data, label = blob['data'], torch.as_tensor(blob['label']).reshape(-1)
    bs = a.batch_size or int(cfg.TEST.BATCH_SIZE)
    T = a.video_length or int(cfg.INPUT.VIDEO_LENGTH)
    batches = ((data[i:i + bs], label[i:i + bs]) for i in range(0, data.shape[0], bs))
    res = pkg.lib.evaluation.classify.evaluate(model, batches, a.test_crops, T, softmax=a.softmax, device=dev)
    print('-----Evaluation is finished------')
    print('Accuracy {:.02f}%'.format(res['mean_class_acc'] * 100))
    print('Overall Prec@1 {:.02f}% Prec@5 {:.02f}%'.format(res['top1'], res['top5']))
    if a.save_scores is not None:
        np.savez(a.save_scores, scores=res['scores'], labels=res['labels'])
    return res


if __name__ == '__main__':
    main()
