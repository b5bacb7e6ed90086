"""The Barlow Twins oracle of the tests: the oracle's encoder (oracle.wrappers.VisualModelWrapper) + a plain-torch projector
with the product's state-dict keys (``model.encoder.*``, ``model.projection.l{1,2}.{0,1}.*``, ``model.projection.l3.weight``),
and the loss written as torch ops on ``F.batch_norm(training=True)`` of each view's features.  The two views go through the
model in two passes -- BatchNorm statistics per view, as the product's wrapper documents -- and the running statistics
therefore update twice per step."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import wrappers as owrap


class Projector(nn.Module):
    def __init__(self, in_dim, hid, out):
        super().__init__()
        self.l1 = nn.Sequential(nn.Linear(in_dim, hid), nn.BatchNorm1d(hid), nn.ReLU(inplace=True))
        self.l2 = nn.Sequential(nn.Linear(hid, hid), nn.BatchNorm1d(hid), nn.ReLU(inplace=True))
        self.l3 = nn.Linear(hid, out, bias=False)

    def forward(self, x):
        return self.l3(self.l2(self.l1(x)))


class BarlowTwins(nn.Module):
    def __init__(self, encoder, hid_dim):
        super().__init__()
        self.encoder = encoder
        self.projection = Projector(encoder.feature_dim, hid_dim, hid_dim)

    def forward(self, x):
        return self.projection(self.encoder(x))


class Wrapper(nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model


def oracle_barlow(backbone, clip_length, feat_dim, state=None, double=True):
    model = Wrapper(BarlowTwins(owrap.VisualModelWrapper(clip_length, backbone), feat_dim))
    if state is not None:
        model.load_state_dict(state)
    return (model.double() if double else model).train()


def barlow_loss(z1, z2, lambd, eps=1e-5):
    N, D = z1.shape
    a = F.batch_norm(z1, None, None, training=True, eps=eps)
    b = F.batch_norm(z2, None, None, training=True, eps=eps)
    c = (a.t() @ b) / N
    on = (torch.diagonal(c) - 1).pow(2).sum()
    off = c.masked_fill(torch.eye(D, dtype=torch.bool), 0).pow(2).sum()
    return on + lambd * off, on, off


def model_loss(model, x, lambd, eps=1e-5):
    """x (b, 6, T, H, W) -> (loss, on, off, z1, z2) through `model` (train mode), view 1 first."""
    x1, x2 = torch.chunk(x, 2, dim=1)
    z1 = model.model(x1)
    z2 = model.model(x2)
    loss, on, off = barlow_loss(z1, z2, lambd, eps)
    return loss, on, off, z1, z2
