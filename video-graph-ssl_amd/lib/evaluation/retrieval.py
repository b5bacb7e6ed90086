"""Nearest-neighbour video retrieval (reference: tools/video_retrieval.py).

The reference extracts one feature per video with the pre-trained encoder (mean over crops x clips, :101-115), pickles
features and classes (:145-150), and ranks every validation video against the training set with sklearn's
cosine_distances / euclidean_distances and np.argsort of the full (nq, ng) matrix (:174-197).  Here the encoder runs on the
engine in eval mode and the search is ops.retrieval_topk (gca_retrieval_topk): fused distance + top-k with per-query
first-hit ranks, from which R@k for every k is a count.  Ties rank by gallery index (np.argsort(kind='stable')); the
reference's default argsort leaves them undefined.

Two inputs, as in lib/evaluation/classify.py: finished fp32 views made by a host transform (the reference's way), or
decoded uint8 frames staged by engine.input.ActionInputStage(mode='test'), whose resize, crops and normalisation run on the
device (gca_clip_views).  The mean over views and the optional softmax are torch reductions over (B, views, feature_dim).
"""
import os
import pickle

import numpy as np
import torch

from ...engine import ops
from ...engine.input import ActionInputStage, StagedBatch
from ...engine.tape import Tape, Var
from ..modeling.visual_wrappers import VisualModelWrapper

KS = (1, 5, 10, 20, 50)


def encoder_state_dict(state_dict):
    """The encoder's entries of a pre-training checkpoint's ``state_dict``: keys without ``proj_head``, with everything up
    to and including the first ``encoder.`` removed (tools/video_retrieval.py:42-43)."""
    return {k.split('encoder.', 1)[1]: v for k, v in state_dict.items() if 'proj_head' not in k and 'encoder.' in k}


def load_encoder(checkpoint, backbone_name, clip_length, dropout=0.):
    """VisualModelWrapper in eval mode with the encoder weights of `checkpoint`: a path (torch.load) or the checkpoint
    dict itself (``{'state_dict': ...}``, the trainers' format)."""
    if not isinstance(checkpoint, dict):
        checkpoint = torch.load(checkpoint, map_location='cpu', weights_only=False)
    model = VisualModelWrapper(clip_length, 'RGB', backbone_name=backbone_name, backbone_type='3D', agg_fun='avg',
                               dropout=dropout)
    model.load_state_dict(encoder_state_dict(checkpoint['state_dict']))
    return model.eval()


def split_views(data, num_crops, video_length):
    """(B, 3, clips * crops * T, H, W) -> (B, clips * crops, 3, T, H, W): dim 2 holds, per clip, `num_crops` runs of
    `video_length` frames (tools/video_retrieval.py:105-109)."""
    B, C, F = data.shape[:3]
    if F % (num_crops * video_length):
        raise ValueError('frame axis %d is no multiple of crops * video_length = %d' % (F, num_crops * video_length))
    views = F // video_length
    return data.reshape((B, C, views, video_length) + tuple(data.shape[3:])).transpose(1, 2)


def extract_feature_single(model, data, num_crops, video_length, softmax=False, views_buf=None):
    """One feature per video: a single eval-mode forward over all crops x clips views, then their mean
    (tools/video_retrieval.py:101-115).  -> (B, feature_dim) on data's device.

    data: (B, 3, clips * crops * T, H, W) finished views, or a StagedBatch of a test-mode engine.input.ActionInputStage
    (decoded uint8 frames): gca_clip_views then cuts the (B * views, 3, T, H, W) block on the device, video-major, into
    `views_buf` (a fp32 tensor of the stage's out_shape() that the caller keeps across batches; allocated here if None);
    num_crops is the stage's own, as in classify.eval_video."""
    if model.training:
        raise RuntimeError('extract_feature_single needs the encoder in eval mode')
    if isinstance(data, StagedBatch):
        stage = data.stage
        if not isinstance(stage, ActionInputStage) or stage.mode != 'test':
            raise RuntimeError('extract_feature_single takes batches staged by a test-mode ActionInputStage')
        if video_length != stage.T:
            raise ValueError('video_length %d, but the batch was staged as clips of %d frames' % (video_length, stage.T))
        if views_buf is None:
            views_buf = torch.empty(stage.out_shape(), dtype=torch.float32, device=stage.device)
        elif tuple(views_buf.shape) != tuple(stage.out_shape()) or views_buf.dtype is not torch.float32:
            raise ValueError('views_buf must be a fp32 tensor of the stage\'s out_shape() %s' % (tuple(stage.out_shape()),))
        B, views = stage.b, stage.views
        x = stage.prepare(data, views_buf)
    else:
        v = split_views(data, num_crops, video_length)
        B, views = v.shape[:2]
        x = v.reshape((B * views,) + tuple(v.shape[2:])).contiguous().float()
    with torch.no_grad():
        out = model.fwd(Tape(False), Var(x, False)).t
        out = out.reshape(B, views, -1).mean(1)
        return torch.softmax(out, dim=-1) if softmax else out


def batch_features(model, clips, num_crops, video_length, device, softmax=False, views_buf=None):
    """extract_feature_single of one batch of a feature pass -> (features, views_buf): a tensor batch is moved to `device`;
    a StagedBatch has its views cut into `views_buf`, which is (re)allocated when it does not fit the batch's stage and
    handed back for the next batch."""
    if not isinstance(clips, StagedBatch):
        return extract_feature_single(model, clips.to(device), num_crops, video_length, softmax), views_buf
    stage = clips.stage
    if views_buf is None or tuple(views_buf.shape) != tuple(stage.out_shape()) or views_buf.device != stage.device:
        views_buf = torch.empty(stage.out_shape(), dtype=torch.float32, device=stage.device)
    return extract_feature_single(model, clips, num_crops, video_length, softmax, views_buf=views_buf), views_buf


def feature_files(out_dir, split, features_file='features.pkl', classes_file='classes.pkl'):
    return os.path.join(out_dir, '%s_%s' % (split, features_file)), os.path.join(out_dir, '%s_%s' % (split, classes_file))


def extract_features(model, batches, num_crops, video_length, out_dir, split, softmax=False, device=None,
                     features_file='features.pkl', classes_file='classes.pkl'):
    """Features of every (clips, target) batch -> ``{split}_features.pkl`` / ``{split}_classes.pkl`` in out_dir, pickled
    numpy arrays as the reference writes them (:145-150).  -> (features, classes).  `clips` may be a StagedBatch of a
    test-mode ActionInputStage (see extract_feature_single); the views of every such batch are cut into one buffer."""
    device = torch.device('cuda') if device is None else device
    feats, classes, buf = [], [], None
    for clips, target in batches:
        f, buf = batch_features(model, clips, num_crops, video_length, device, softmax, buf)
        feats.append(f.cpu())
        classes.append(torch.as_tensor(target).reshape(-1).cpu())
    feats, classes = torch.cat(feats, 0).numpy(), torch.cat(classes, 0).numpy()
    fpath, cpath = feature_files(out_dir, split, features_file, classes_file)
    for path, arr in ((fpath, feats), (cpath, classes)):
        with open(path, 'wb') as fh:
            pickle.dump(arr, fh, protocol=pickle.HIGHEST_PROTOCOL)
    return feats, classes


def recall_counts(first_hit, ks=KS):
    """{k: number of queries whose first same-class neighbour has rank <= k}."""
    first_hit = np.asarray(first_hit)
    return {int(k): int((first_hit <= k).sum()) for k in ks}


def search_first_hit(val_features, val_classes, train_features, train_classes, k, metric, norm=False, device=None):
    """first_hit (nq,) of the validation rows against the training rows, on the device."""
    device = torch.device('cuda') if device is None else device
    q = torch.from_numpy(np.ascontiguousarray(val_features, dtype=np.float32)).to(device)
    g = torch.from_numpy(np.ascontiguousarray(train_features, dtype=np.float32)).to(device)
    if norm:        # F.normalize(dim=1), :174-176
        q, g = ops.l2norm_fwd(q)[0], ops.l2norm_fwd(g)[0]
    ql = torch.from_numpy(np.ascontiguousarray(val_classes, dtype=np.int64).reshape(-1)).to(device)
    gl = torch.from_numpy(np.ascontiguousarray(train_classes, dtype=np.int64).reshape(-1)).to(device)
    return ops.retrieval_topk(q, g, k, metric, ql, gl)[2].cpu().numpy()


def topk_retrieval(train_features, train_classes, val_features, val_classes, metric='cosine', norm=False, ks=KS,
                   device=None):
    """Validation videos searched in the training set (tools/video_retrieval.py:154-208) -> ({k: correct}, total): the
    dict the reference dumps as topk_correct.json, and the number of validation videos."""
    ks = tuple(int(k) for k in ks)
    if not ks or min(ks) < 1 or max(ks) > 64:
        raise ValueError('topk_retrieval: every k must lie in [1, 64] (got %r)' % (ks,))
    if len(val_features) != len(val_classes) or len(train_features) != len(train_classes):
        raise ValueError('topk_retrieval: one class per feature row')
    first_hit = search_first_hit(val_features, val_classes, train_features, train_classes, max(ks), metric, norm, device)
    return recall_counts(first_hit, ks), int(len(val_classes))
