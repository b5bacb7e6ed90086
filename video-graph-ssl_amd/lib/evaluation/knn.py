"""Weighted k-NN classification on frozen features: the evaluation self-supervised code bases plot per epoch (InstDisc's
kNN monitor, MoCo / SimSiam's knn_predict, solo-learn's WeightedKNNClassifier).

Embed a labelled bank, find the k nearest bank rows of every query (ops.retrieval_topk, cosine distance), let each neighbour
vote for its class with weight exp(sim / T) and report top-1 / top-5 of the vote (ops.knn_vote).  Nothing is trained.  The
kernel's weight is exp(-dist / T) = exp(sim / T) / exp(1 / T): the same ranking without the overflow.  Features, labels and
all intermediate lists stay on the device; the host sees counts.

Limits: k <= 64, the list length of the search kernel (the InstDisc protocol's k = 200 needs another search kernel; the
default here is k = 20), and the exp weight is defined on cosine distance only.
"""
import numpy as np
import torch

from ...engine import ops
from ..modeling.visual_wrappers import VisualModelWrapper
from .retrieval import batch_features, encoder_state_dict

KS = (1, 5, 10, 20)
LOO_CHUNK = 4096


def _features(f, device=None):
    """numpy array or tensor -> contiguous fp32 (n, D) on the device."""
    t = torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)) if isinstance(f, np.ndarray) else torch.as_tensor(f)
    if t.dim() != 2:
        raise ValueError('features are (n, D) matrices (got %s)' % (tuple(t.shape),))
    if device is None:
        device = t.device if t.is_cuda else torch.device('cuda')
    return t.to(device=device, dtype=torch.float32).contiguous()


def _labels(c, n, device):
    t = torch.from_numpy(np.ascontiguousarray(c)) if isinstance(c, np.ndarray) else torch.as_tensor(c)
    t = t.reshape(-1)
    if t.is_floating_point() or t.dtype is torch.bool:
        raise ValueError('class labels are integers (got %s)' % t.dtype)
    if t.numel() != n:
        raise ValueError('one class per feature row expected (%d labels, %d rows)' % (t.numel(), n))
    t = t.to(device=device, dtype=torch.int64).contiguous()
    if n and int(t.min()) < 0:
        raise ValueError('class labels must not be negative')
    return t


def _num_class(num_class, *labels):
    top = max([int(t.max()) for t in labels if t.numel()] + [-1])
    if num_class is None:
        num_class = top + 1
    num_class = int(num_class)
    if num_class < 1 or top >= num_class:
        raise ValueError('labels must lie in [0, num_class = %d) (largest label %d)' % (num_class, top))
    return num_class


def _ks(ks, limit=64):
    ks = tuple(int(k) for k in ks)
    if not ks or min(ks) < 1 or max(ks) > limit:
        raise ValueError('every k must lie in [1, %d] (got %r)' % (limit, ks))
    return ks


def _check_weighting(weighting, metric='cosine'):
    if weighting not in ops.KNN_WEIGHTINGS:
        raise ValueError('weighting must be one of %s (got %r)' % (sorted(ops.KNN_WEIGHTINGS), weighting))
    if metric not in ops.RETRIEVAL_METRICS:
        raise ValueError('metric must be one of %s (got %r)' % (sorted(ops.RETRIEVAL_METRICS), metric))
    if weighting == 'exp' and metric != 'cosine':
        raise ValueError('the exp weight exp(-dist / T) is defined on cosine distances only (metric=%r)' % metric)


def knn_predict(train_f, train_c, val_f, num_class, k=20, T=0.07, weighting='exp', metric='cosine', device=None):
    """Predicted class (nq,) int32 on the device of every row of val_f: one search of the bank, one vote.  -1 for a row
    without a neighbour (an empty bank)."""
    _check_weighting(weighting, metric)
    k = _ks((k,))[0]
    g = _features(train_f, device)
    q = _features(val_f, g.device)
    gl = _labels(train_c, g.shape[0], g.device)
    num_class = _num_class(num_class, gl)
    idx, dist, _ = ops.retrieval_topk(q, g, k, metric)
    return ops.knn_vote(idx, dist, gl, num_class, weighting=weighting, T=T)[0]


def _count(rank):
    return {'top1': int((rank < 1).sum()), 'top5': int((rank < 5).sum())}


def knn_classify(train_f, train_c, val_f, val_c, num_class=None, ks=KS, T=0.07, weighting='exp', device=None):
    """Validation rows classified by their nearest training rows -> ({k: {'top1': n, 'top5': n}}, total): for every k the
    number of validation rows whose class is the first / among the first five of the vote of the k nearest neighbours.
    One cosine search at max(ks) serves every k (the lists are sorted: the first k slots are the k nearest)."""
    _check_weighting(weighting)
    ks = _ks(ks)
    g = _features(train_f, device)
    q = _features(val_f, g.device)
    gl, ql = _labels(train_c, g.shape[0], g.device), _labels(val_c, q.shape[0], g.device)
    num_class = _num_class(num_class, gl, ql)
    idx, dist, _ = ops.retrieval_topk(q, g, max(ks), 'cosine')
    out = {}
    for k in ks:
        rank = ops.knn_vote(idx, dist, gl, num_class, kvote=k, q_label=ql, weighting=weighting, T=T)[1]
        out[k] = _count(rank)
    return out, int(q.shape[0])


def knn_classify_loo(f, c, num_class=None, ks=KS, T=0.07, weighting='exp', chunk=LOO_CHUNK, device=None):
    """Leave-one-out on one labelled set: every row is classified by its nearest OTHER rows.  The search asks for
    max(ks) + 1 <= 64 neighbours and the vote drops the row itself (self_base), wherever it ranks among equal rows.  Runs in
    chunks of `chunk` queries so the search workspace stays bounded.  -> ({k: {'top1': n, 'top5': n}}, total)."""
    _check_weighting(weighting)
    ks = _ks(ks, 63)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError('chunk must be positive')
    g = _features(f, device)
    gl = _labels(c, g.shape[0], g.device)
    num_class = _num_class(num_class, gl)
    out = {k: {'top1': 0, 'top5': 0} for k in ks}
    for lo in range(0, g.shape[0], chunk):
        hi = min(lo + chunk, g.shape[0])
        idx, dist, _ = ops.retrieval_topk(g[lo:hi], g, max(ks) + 1, 'cosine')
        for k in ks:
            rank = ops.knn_vote(idx, dist, gl, num_class, kvote=k, q_label=gl[lo:hi], self_base=lo, weighting=weighting, T=T)[1]
            for key, n in _count(rank).items():
                out[k][key] += n
    return out, int(g.shape[0])


def features_of(model, batches, num_crops, video_length, device=None):
    """The feature pass of retrieval.extract_features with everything left on the device and no files: (clips, target)
    batches -> (features (N, feature_dim) fp32, classes (N,) int64).  `clips` is a (B, 3, clips * crops * T, H, W) tensor or a
    StagedBatch of a test-mode ActionInputStage; the views of staged batches are cut into one buffer kept across batches."""
    device = torch.device('cuda') if device is None else torch.device(device)
    feats, classes, buf = [], [], None
    for clips, target in batches:
        f, buf = batch_features(model, clips, num_crops, video_length, device, views_buf=buf)
        feats.append(f)
        classes.append(torch.as_tensor(target).reshape(-1).to(device=device, dtype=torch.int64))
    if not feats:
        raise ValueError('features_of: no batches')
    return torch.cat(feats, 0), torch.cat(classes, 0)


class KNNMonitor(object):
    """k-NN accuracy of a pre-training run's encoder while the run is going.

    evaluate(source) takes a pre-training trainer (anything with .state_dict(): MoCoTrainer, SimSiamTrainer), a checkpoint
    dict ({'state_dict': ...}) or a checkpoint path, copies the ``encoder.*`` entries (retrieval.encoder_state_dict) into an
    encoder of the monitor's OWN -- built from cfg.MODEL.BACKBONE, cfg.INPUT.VIDEO_LENGTH and aug_flag=cfg.MODEL.AUG_FLAG, so
    every key loads by name -- embeds bank and queries with features_of in eval mode and returns
    dict(top1, top5, r1 in percent, count): the weighted vote of the k nearest bank rows, and recall@1 of the same search.

    The live model is only read (state_dict()): its train / eval modes, BatchNorm statistics, tape and captured graphs are
    never touched, and the monitor's work runs under torch.random.fork_rng, so the run's random streams continue as if it
    had not been called.

    AUG_FLAG models: the temporal-graph blocks of this package sample their adjacency (RelaxedBernoulli uniforms from
    torch.rand) in eval mode exactly as in train mode -- there is no deterministic eval branch.  The features of such an
    encoder are therefore one random draw per evaluate() (from the forked stream, so equal states give equal numbers), and
    the blocks' BatchNorm layers use their running statistics.

    bank_batches / query_batches: iterables of (clips, target) as features_of takes them, or callables returning one (for
    staged batches, which are consumed as they are prepared).  They are embedded again on every evaluate()."""

    def __init__(self, cfg, bank_batches, query_batches, num_class, k=20, T=0.07, num_crops=1, device=None):
        self.k = _ks((k,))[0]
        self.T, self.num_class, self.num_crops = float(T), int(num_class), int(num_crops)
        if self.num_class < 1 or not self.T > 0:
            raise ValueError('KNNMonitor: num_class >= 1 and T > 0 required')
        self.device = torch.device('cuda') if device is None else torch.device(device)
        self.video_length = int(cfg.INPUT.VIDEO_LENGTH)
        self.bank_batches, self.query_batches = bank_batches, query_batches
        with torch.random.fork_rng(devices=self._rng_devices()):
            self.encoder = VisualModelWrapper(self.video_length, 'RGB', backbone_name=cfg.MODEL.BACKBONE, backbone_type='3D',
                                              agg_fun='avg', dropout=0., aug_flag=bool(cfg.MODEL.AUG_FLAG))
        self.encoder.to(self.device).eval()

    def _rng_devices(self):
        return [self.device] if self.device.type == 'cuda' else []

    @staticmethod
    def _state(source):
        if hasattr(source, 'state_dict') and not isinstance(source, dict):
            source = source.state_dict()
        elif not isinstance(source, dict):
            source = torch.load(source, map_location='cpu', weights_only=False)
        if 'state_dict' not in source:
            raise ValueError('KNNMonitor: a trainer, a checkpoint dict with \'state_dict\' or a path expected')
        return encoder_state_dict(source['state_dict'])

    @staticmethod
    def _iter(batches):
        return batches() if callable(batches) else batches

    def evaluate(self, source):
        with torch.random.fork_rng(devices=self._rng_devices()), torch.no_grad():
            self.encoder.load_state_dict(self._state(source))
            self.encoder.eval()
            g, gl = features_of(self.encoder, self._iter(self.bank_batches), self.num_crops, self.video_length, self.device)
            q, ql = features_of(self.encoder, self._iter(self.query_batches), self.num_crops, self.video_length, self.device)
            if not gl.numel() or not ql.numel():
                raise ValueError('KNNMonitor: an empty bank or query set')
            for lab in (gl, ql):
                if int(lab.min()) < 0 or int(lab.max()) >= self.num_class:
                    raise ValueError('KNNMonitor: labels must lie in [0, %d)' % self.num_class)
            idx, dist, hit = ops.retrieval_topk(q, g, self.k, 'cosine', ql, gl)
            rank = ops.knn_vote(idx, dist, gl, self.num_class, q_label=ql, weighting='exp', T=self.T)[1]
            n = int(ql.numel())
            return dict(top1=100.0 * int((rank < 1).sum()) / n, top5=100.0 * int((rank < 5).sum()) / n,
                        r1=100.0 * int((hit <= 1).sum()) / n, count=n)
