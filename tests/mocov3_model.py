"""The MoCo v3 oracle of the tests: the oracle's encoder (oracle.wrappers.VisualModelWrapper), its ProjectionMLP and, for the
student, its PredictionMLP, under the product's state-dict keys (``model.encoder.*``, ``model.projection.*``,
``model.prediction.*``); rows are L2-normalised; the loss is the literal one of Algorithm 1 (tests/mocov3_ref.py: torch_chain).
One step, as the product's trainer documents it: the teacher (BatchNorm in train mode, no gradient) and the student see both
views in two passes each, view 1 first; SGD on the student; THEN the teacher follows as an EMA over encoder and projector --
the parameters it has -- and its BatchNorm buffers are its own."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import moco as omoco
from oracle import wrappers as owrap
from mocov3_ref import torch_chain


class MoCoV3(nn.Module):
    def __init__(self, encoder, out_dim, hid_dim, predictor=True):
        super().__init__()
        self.encoder = encoder
        self.projection = owrap.ProjectionMLP(encoder.feature_dim, hid_dim, out_dim)
        if predictor:
            self.prediction = owrap.PredictionMLP(out_dim, hid_dim, out_dim)
        self.has_predictor = predictor

    def forward(self, x):
        z = self.projection(self.encoder(x))
        if self.has_predictor:
            z = self.prediction(z)
        return F.normalize(z, dim=1)


class Wrapper(nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x):
        return self.model(x)


def oracle_mocov3(backbone, clip_length, out_dim, hid_dim, state=None, state_ema=None, double=True):
    """-> (student, teacher), loaded from `state` / `state_ema` (default: the student's state without the predictor)."""
    model = Wrapper(MoCoV3(owrap.VisualModelWrapper(clip_length, backbone), out_dim, hid_dim, True))
    ema = Wrapper(MoCoV3(owrap.VisualModelWrapper(clip_length, backbone), out_dim, hid_dim, False))
    if state is not None:
        model.load_state_dict(state)
        ema.load_state_dict({k: v for k, v in state.items() if '.prediction.' not in k} if state_ema is None else state_ema)
    if double:
        model, ema = model.double(), ema.double()
    model.train()
    omoco.set_key_encoder_mode(ema)
    return model, ema


def model_loss(model, ema, x, T):
    """x (b, 6, T, H, W) -> (loss, (q1, q2, k1, k2)) through teacher and student."""
    x1, x2 = torch.chunk(x, 2, dim=1)
    with torch.no_grad():
        k1 = ema(x1)
        k2 = ema(x2)
    q1 = model(x1)
    q2 = model(x2)
    return torch_chain(q1, q2, k1, k2, T), (q1, q2, k1, k2)


def oracle_steps(model, ema, x, steps, base_lr, alpha, T):
    """`steps` steps (SGD with the reference's parameter groups: momentum 0.9, weight decay 5e-4, biases at twice the rate
    without decay; a constant rate; teacher momentum `alpha`) on the one batch x -> the loss before each step."""
    opt = omoco.make_optimizer(model, base_lr, 0.9, 5e-4)
    student = dict(model.named_parameters())
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss, _ = model_loss(model, ema, x, T)
        loss.backward()
        opt.step()
        with torch.no_grad():                                            # EMA over the parameters the teacher has
            for n, p in ema.named_parameters():
                p.mul_(alpha).add_(student[n].detach(), alpha=1 - alpha)
        losses.append(float(loss.detach()))
    return losses
