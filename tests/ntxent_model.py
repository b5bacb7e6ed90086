"""The SimCLR oracle of the tests: the oracle's MoCo-format model (oracle.wrappers.create_visual_model(..., 'mlp', 'moco'):
encoder + 'mlp' projection head + Normalize, state-dict keys ``model.encoder.*`` / ``model.proj_head.*``) with the NT-Xent loss
written as plain torch ops.  The two views go through the model in two passes -- BatchNorm statistics per view, as the
product's SimCLR wrapper documents -- and the running statistics therefore update twice per step."""
import torch
import torch.nn.functional as F

from oracle import wrappers as owrap


def oracle_simclr(backbone, clip_length, feat_dim, state=None, double=True):
    model, _ = owrap.create_visual_model(backbone, clip_length, feat_dim, 'mlp', 'moco')
    if state is not None:
        model.load_state_dict(state)
    return (model.double() if double else model).train()


def nt_xent(z1, z2, T):
    z = torch.cat([z1, z2], 0)
    N = z.shape[0]
    s = (z @ z.t()) / T
    s = s.masked_fill(torch.eye(N, dtype=torch.bool), float('-inf'))
    target = (torch.arange(N) + N // 2) % N
    return F.cross_entropy(s, target), s, target


def simclr_loss(model, x, T):
    """x (b, 6, T, H, W) -> (loss, z (2b, D)) through `model` (train mode), view 1 first."""
    x1, x2 = torch.chunk(x, 2, dim=1)
    z1 = model(x1)
    z2 = model(x2)
    loss, _, _ = nt_xent(z1, z2, T)
    return loss, torch.cat([z1, z2], 0)
