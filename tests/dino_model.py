"""The DINO oracle of the tests: student and teacher are the oracle's MoCo-format model (oracle.wrappers.create_visual_model(...,
'mlp', 'moco'): encoder + 'mlp' projection head + Normalize, state-dict keys ``model.encoder.*`` / ``model.proj_head.*``), each
with a ``model.prototypes.weight`` parameter; the loss is tests/dino_ref.py's torch_chain.  One step, as the product's trainer
documents it: the teacher (BatchNorm in train mode, no gradient) and the student see both views in two passes each, view 1
first; both prototype matrices are renormalised without gradient; the loss uses the centre and then moves it; SGD on the
student; the teacher follows as an EMA over ALL parameters, prototypes included."""
import torch
import torch.nn as nn

from oracle import moco as omoco
from oracle import wrappers as owrap
from dino_ref import torch_chain


class Prototypes(nn.Module):
    def __init__(self, dim, K):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(K, dim))


def oracle_dino(backbone, clip_length, feat_dim, K, state=None, state_ema=None, double=True):
    """-> (student, teacher), the teacher loaded from `state_ema` (default: the student's state)."""
    model, ema = owrap.create_visual_model(backbone, clip_length, feat_dim, 'mlp', 'moco')
    for m in (model, ema):
        m.model.prototypes = Prototypes(feat_dim, K)
    if state is not None:
        model.load_state_dict(state)
        ema.load_state_dict(state if state_ema is None else state_ema)
    if double:
        model, ema = model.double(), ema.double()
    model.train()
    omoco.set_key_encoder_mode(ema)
    return model, ema


def model_loss(model, ema, x, center, Ts=0.1, Tt=0.04, cm=0.9):
    """x (b, 6, T, H, W) -> (loss, l12, l21, ent, new centre) through teacher and student."""
    Cs, Ct = model.model.prototypes.weight, ema.model.prototypes.weight
    x1, x2 = torch.chunk(x, 2, dim=1)
    with torch.no_grad():
        zt1 = ema(x1)
        zt2 = ema(x2)
    z1 = model(x1)
    z2 = model(x2)
    with torch.no_grad():
        Cs.copy_(Cs / Cs.norm(dim=1, keepdim=True))
        Ct.copy_(Ct / Ct.norm(dim=1, keepdim=True))
    return torch_chain(z1, z2, Cs, zt1, zt2, Ct, center, Ts, Tt, cm)


def oracle_steps(model, ema, x, steps, base_lr, alpha, K, Ts=0.1, Tt=0.04, cm=0.9):
    """`steps` steps (SGD with the reference's parameter groups: momentum 0.9, weight decay 5e-4, biases at twice the rate
    without decay; a constant rate; teacher momentum `alpha`) on the one batch x -> (the loss before each step, the centre and
    the teacher's prototypes after the last)."""
    opt = omoco.make_optimizer(model, base_lr, 0.9, 5e-4)
    center = torch.zeros(K, dtype=x.dtype)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss, _, _, _, center = model_loss(model, ema, x, center, Ts, Tt, cm)
        loss.backward()
        opt.step()
        omoco.momentum_update(model, ema, alpha)
        losses.append(float(loss.detach()))
    return losses, center, ema.model.prototypes.weight.detach().clone()
