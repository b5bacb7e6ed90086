"""The SwAV oracle of the tests: the oracle's MoCo-format model (oracle.wrappers.create_visual_model(..., 'mlp', 'moco'):
encoder + 'mlp' projection head + Normalize, state-dict keys ``model.encoder.*`` / ``model.proj_head.*``) with a
``model.prototypes.weight`` parameter, and the published loss as torch ops (tests/swav_ref.py: torch_chain).  As the authors'
training loop does, a step first renormalises the prototype rows without gradient.  The two views go through the model in two
passes -- BatchNorm statistics per view, as the product's wrapper documents -- and the running statistics therefore update twice
per step."""
import torch
import torch.nn as nn

from oracle import wrappers as owrap
from swav_ref import torch_chain


class Prototypes(nn.Module):
    def __init__(self, dim, K):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(K, dim))


def oracle_swav(backbone, clip_length, feat_dim, K, state=None, double=True):
    model, _ = owrap.create_visual_model(backbone, clip_length, feat_dim, 'mlp', 'moco')
    model.model.prototypes = Prototypes(feat_dim, K)
    if state is not None:
        model.load_state_dict(state)
    return (model.double() if double else model).train()


def model_loss(model, x, eps=0.05, T=0.1, iters=3):
    """x (b, 6, T, H, W) -> (loss, l12, l21, z1, z2) through `model` (train mode), view 1 first."""
    C = model.model.prototypes.weight
    with torch.no_grad():
        C.copy_(C / C.norm(dim=1, keepdim=True))
    x1, x2 = torch.chunk(x, 2, dim=1)
    z1 = model(x1)
    z2 = model(x2)
    return torch_chain(z1, z2, C, eps, T, iters) + (z1, z2)


def oracle_steps(model, x, steps, base_lr, eps=0.05, T=0.1, iters=3):
    """`steps` SGD steps (the reference's parameter groups: momentum 0.9, weight decay 5e-4, biases at twice the rate without
    decay; a constant rate) on the one batch x -> the loss before each step."""
    from oracle import moco as omoco
    opt = omoco.make_optimizer(model, base_lr, 0.9, 5e-4)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = model_loss(model, x, eps, T, iters)[0]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses
