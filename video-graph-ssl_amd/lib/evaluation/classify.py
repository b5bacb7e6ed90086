"""Video-level action-recognition test (reference: tools/test_ds.py).

The reference scores a video by running every crop of every clip through the eval-mode model, averaging the logits over all
views, optionally taking the softmax of that mean (:134-149), and reports accuracy(top1, top5), the confusion matrix and the
mean per-class accuracy (:165-196).  Here all views of a batch go through the engine in ONE eval-mode forward and the top-k
counts come from gca_rank_ge.  Two defects of the reference are not reproduced: its prediction ``np.argmax(x[0])`` flattens
the whole (B, C) score block and is only right for batch size 1 -- the argmax is taken per video; and its mean per-class
accuracy divides by the count of every class, NaN for a class that never occurs as a label -- the mean runs over the classes
that do occur.

Two inputs: finished fp32 views made by a host transform (as in lib/evaluation/retrieval.py), or decoded uint8 frames
staged by engine.input.ActionInputStage(mode='test'), whose resize, crops, flips and normalisation run on the device
(gca_clip_views); only frame decoding then stays with the host."""
import numpy as np
import torch

from ...engine.input import ActionInputStage, StagedBatch
from ...engine.tape import Tape, Var
from .metric import rank_ge
from .retrieval import split_views


def eval_video(model, data, num_crops, video_length, softmax=False):
    """data (B, 3, clips * crops * T, H, W), or a StagedBatch of a test-mode engine.input.ActionInputStage -> video-level
    scores (B, num_class) on data's device: one eval-mode forward over all clips x crops views, their mean, then optionally its
    softmax (tools/test_ds.py:134-149)."""
    if model.training:
        raise RuntimeError('eval_video needs the model in eval mode')
    if isinstance(data, StagedBatch):
        # uint8 source frames staged by a test-mode ActionInputStage: gca_clip_views writes the (B * views, 3, T, H, W) block
        # the forward takes, video-major -- no split_views; num_crops / video_length are the stage's own
        stage = data.stage
        if not isinstance(stage, ActionInputStage) or stage.mode != 'test':
            raise RuntimeError('eval_video takes batches staged by a test-mode ActionInputStage')
        if video_length != stage.T:
            raise ValueError('video_length %d, but the batch was staged as clips of %d frames' % (video_length, stage.T))
        B, views = stage.b, stage.views
        x = stage.prepare(data, torch.empty(stage.out_shape(), dtype=torch.float32, device=stage.device))
    else:
        v = split_views(data, num_crops, video_length)
        B, views = v.shape[:2]
        x = v.reshape((B * views,) + tuple(v.shape[2:])).contiguous().float()
    with torch.no_grad():
        out = model.fwd(Tape(False), Var(x, False)).t
        out = out.reshape(B, views, -1).mean(1)
        return torch.softmax(out, dim=-1) if softmax else out


def confusion(labels, pred, num_class):
    """(num_class, num_class) int64 counts, row = label, column = prediction (sklearn.metrics.confusion_matrix with
    labels=range(num_class))."""
    labels, pred = np.asarray(labels, dtype=np.int64).reshape(-1), np.asarray(pred, dtype=np.int64).reshape(-1)
    if labels.shape != pred.shape:
        raise ValueError('one prediction per label')
    if labels.size and (min(labels.min(), pred.min()) < 0 or max(labels.max(), pred.max()) >= num_class):
        raise ValueError('labels and predictions must lie in [0, %d)' % num_class)
    cf = np.zeros((num_class, num_class), dtype=np.int64)
    np.add.at(cf, (labels, pred), 1)
    return cf


def mean_class_acc(cf):
    """Mean over the classes that occur as a label of hits / count (tools/test_ds.py:190-195 without its NaN rows)."""
    cf = np.asarray(cf, dtype=np.float64)
    cnt = cf.sum(axis=1)
    seen = cnt > 0
    if not seen.any():
        raise ValueError('empty confusion matrix')
    return float((np.diag(cf)[seen] / cnt[seen]).mean())


def evaluate(model, batches, num_crops, video_length, softmax=False, device=None):
    """(data, label) batches -> dict(top1, top5 in percent, averaged by video count; confusion (C, C); mean_class_acc;
    scores (N, C) and labels (N,) as numpy arrays, the material of --save_scores)."""
    device = torch.device('cuda') if device is None else device
    scores, labels, hits, n = [], [], np.zeros(2), 0
    for data, label in batches:
        s = eval_video(model, data if isinstance(data, StagedBatch) else data.to(device), num_crops, video_length, softmax)
        lab = torch.as_tensor(label).reshape(-1).to(torch.int64)
        if lab.numel() != s.shape[0] or (lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= s.shape[1])):
            raise ValueError('one label in [0, %d) per video expected' % s.shape[1])
        r = rank_ge(s, lab.to(device)).cpu().numpy()
        hits += [(r < 1).sum(), (r < 5).sum()]
        n += lab.numel()
        scores.append(s.cpu().numpy())
        labels.append(lab.numpy())
    if n == 0:
        raise ValueError('evaluate: no videos')
    scores, labels = np.concatenate(scores, 0), np.concatenate(labels, 0)
    cf = confusion(labels, scores.argmax(axis=1), scores.shape[1])
    return dict(top1=100.0 * hits[0] / n, top5=100.0 * hits[1] / n, confusion=cf, mean_class_acc=mean_class_acc(cf),
                scores=scores, labels=labels)
