"""The NNCLR oracle of the tests: the oracle's encoder (oracle.wrappers.VisualModelWrapper), its ProjectionMLP and PredictionMLP
under the product's state-dict keys (``model.encoder.*``, ``model.projection.*``, ``model.prediction.*``); projection z and
prediction p are L2-normalised rows; the loss is the literal one of Algorithm 1 (tests/nnclr_ref.py: torch_chain) against a
support set Q.  One step, as the product's trainer documents it: both views through the model, view 1 first; the search sees the
PRE-enqueue support set; SGD; z1 (detached) is written at rows (index + i) % K and the pointer advances."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import moco as omoco
from oracle import wrappers as owrap
from nnclr_ref import torch_chain


class NNCLR(nn.Module):
    def __init__(self, encoder, out_dim, hid_dim):
        super().__init__()
        self.encoder = encoder
        self.projection = owrap.ProjectionMLP(encoder.feature_dim, hid_dim, out_dim)
        self.prediction = owrap.PredictionMLP(out_dim, hid_dim, out_dim)

    def forward(self, x):
        z = self.projection(self.encoder(x))
        return F.normalize(z, dim=1), F.normalize(self.prediction(z), dim=1)


class Wrapper(nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x):
        return self.model(x)


def oracle_nnclr(backbone, clip_length, out_dim, hid_dim, state=None, double=True):
    model = Wrapper(NNCLR(owrap.VisualModelWrapper(clip_length, backbone), out_dim, hid_dim))
    if state is not None:
        model.load_state_dict(state)
    if double:
        model = model.double()
    model.train()
    return model


def model_loss(model, x, Q, T):
    """x (b, 6, T, H, W), Q (K, D) -> (loss, (z1, z2, p1, p2), (idx (2, b), top-2 gap (2, b)))."""
    x1, x2 = torch.chunk(x, 2, dim=1)
    z1, p1 = model(x1)
    z2, p2 = model(x2)
    z1, z2 = z1.detach(), z2.detach()
    s = torch.stack([z1 @ Q.t(), z2 @ Q.t()])
    top = s.topk(min(2, Q.shape[0]), dim=2).values
    gap = top[..., 0] - top[..., -1] if Q.shape[0] > 1 else torch.full(s.shape[:2], float('inf'))
    return torch_chain(z1, z2, p1, p2, Q, T), (z1, z2, p1, p2), (s.argmax(dim=2), gap)


def oracle_steps(model, Q, index, xs, base_lr, T):
    """One step per batch of `xs` (SGD with the reference's parameter groups: momentum 0.9, weight decay 5e-4, biases at twice
    the rate without decay; a constant rate), the support set Q (K, D) updated in place from pointer `index` -> (losses, idx per
    step, smallest top-2 gap per step, (z1, z2) per step, final index)."""
    opt = omoco.make_optimizer(model, base_lr, 0.9, 5e-4)
    K = Q.shape[0]
    losses, idxs, gaps, zs = [], [], [], []
    for x in xs:
        opt.zero_grad()
        loss, rows, (idx, gap) = model_loss(model, x, Q, T)
        loss.backward()
        opt.step()
        with torch.no_grad():
            z1 = rows[0]
            for i in range(z1.shape[0]):
                Q[(index + i) % K] = z1[i]
            index = (index + z1.shape[0]) % K
        losses.append(float(loss.detach()))
        idxs.append(idx.clone())
        gaps.append(float(gap.min()))
        zs.append((rows[0].clone(), rows[1].clone()))
    return losses, idxs, gaps, zs, index


def planted_queue(model, xs, base_lr, T, K, seed=0):
    """The support set of the step tests.  Against random rows the nearest neighbour of a projection is decided by a few 1e-3 of
    cosine, which the 1e-3 feature bar cannot hold exactly.  So a COPY of the oracle is run over the batches once, against a random
    unit queue, and the projections of every step and view, rounded to fp32, become the LAST rows of that queue, out of reach of
    the enqueues of len(xs) steps: every row then has one neighbour at cosine about 1 (the run that counts moves the projections
    by the difference of two tiny SGD steps only) -> (K, D) fp32 unit rows."""
    import copy
    b = xs[0].shape[0]
    n = 2 * b * len(xs)
    if K < n + b * len(xs):
        raise ValueError('planted_queue: K too small')
    pre = copy.deepcopy(model)
    rows = oracle_steps(pre, queue0(seed, K, OUT).to(xs[0].dtype), 0, xs, base_lr, T)[3]
    Q = queue0(seed, K, OUT)
    Q[K - n:] = torch.cat([z for pair in rows for z in pair]).float()
    return Q


# ----------------------------------------------------------------------------- the tiny configuration of the model / trainer tests
CLIP = (8, 6, 8, 48, 48)
OUT, HID, TEMP, QUEUE_K = 32, 48, 0.2, 80          # three steps enqueue rows 0 .. 23; planted_queue fills rows 32 .. 79
LR = 3e-6                                          # this tiny model on 8 clips is badly conditioned over several steps: the ORACLE's own fp32
                                                   # run leaves its fp64 run by 2.0e-3 on the support set after three steps at a rate of
                                                   # 3e-5 and by 1.8e-3 at 1e-5, by 7.9e-5 at 3e-6 (third loss: 1.7e-6) -- checked on the
                                                   # CPU -- a twelfth of the 1e-3 bar
GAP_BAR = 100 * 1e-3                               # the oracle's top-2 gap of every row of every step must exceed 100x the feature bar
MODEL_SEED, CLIP_SEED, QUEUE_SEED = 7, 33, 0


def clip_batches(n=3, seed=CLIP_SEED):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*CLIP, generator=gen) for _ in range(n)]


def queue0(seed=QUEUE_SEED, K=QUEUE_K, D=OUT):
    return F.normalize(torch.randn(K, D, generator=torch.Generator().manual_seed(seed)))
