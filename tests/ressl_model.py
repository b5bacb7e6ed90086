"""The ReSSL oracle of the tests: MoCo's oracle model and key encoder (oracle.wrappers.create_visual_model, 'moco') under the
product's state-dict keys, the queue as a plain (K, D) tensor, and the literal loss (tests/ressl_ref.py: torch_chain).  One step,
as the product's trainer documents it: the teacher (BatchNorm in train mode, no gradient) sees view 2, the student view 1; the
loss is taken against the PRE-enqueue queue; SGD on the student; the teacher follows as an EMA of the parameters; the teacher's
rows, in the order `shuffle_ids` (MoCo's all_k), are written at rows (index + i) % K and the pointer advances."""
import torch
import torch.nn.functional as F

from oracle import moco as omoco
from oracle import wrappers as owrap
from ressl_ref import torch_chain


def oracle_ressl(backbone, clip_length, out_dim, state=None, state_ema=None, double=True):
    """-> (student, teacher), both loaded from `state` (the teacher from `state_ema` if given)."""
    model, ema = owrap.create_visual_model(backbone, clip_length, out_dim, 'mlp', 'moco')
    if state is not None:
        model.load_state_dict(state)
        ema.load_state_dict(state if state_ema is None else state_ema)
    if double:
        model, ema = model.double(), ema.double()
    model.train()
    omoco.set_key_encoder_mode(ema)
    return model, ema


def model_loss(model, ema, x, Q, Ts, Tt):
    """x (b, 6, T, H, W), Q (K, D) -> (loss, q, k)."""
    x1, x2 = torch.chunk(x, 2, dim=1)
    with torch.no_grad():
        k = ema(x2)
    q = model(x1)
    return torch_chain(q, k, Q, Ts, Tt), q, k


def oracle_steps(model, ema, Q, index, xs, shuffles, base_lr, alpha, Ts, Tt):
    """One step per batch of `xs` (SGD with the reference's parameter groups: momentum 0.9, weight decay 5e-4, biases at twice
    the rate without decay; a constant rate), the queue Q updated in place from pointer `index` -> (losses, final index)."""
    opt = omoco.make_optimizer(model, base_lr, 0.9, 5e-4)
    K = Q.shape[0]
    losses = []
    for x, sh in zip(xs, shuffles):
        opt.zero_grad()
        loss, _, k = model_loss(model, ema, x, Q, Ts, Tt)
        loss.backward()
        opt.step()
        omoco.momentum_update(model, ema, alpha)
        with torch.no_grad():
            all_k = k[sh]
            for i in range(all_k.shape[0]):
                Q[(index + i) % K] = all_k[i]
            index = (index + all_k.shape[0]) % K
        losses.append(float(loss.detach()))
    return losses, index


# ----------------------------------------------------------------------------- the tiny configuration of the model / trainer tests
CLIP = (8, 6, 8, 48, 48)
OUT, QUEUE_K, TS, TT, ALPHA = 32, 20, 0.1, 0.04, 0.9     # three steps of 8 rows wrap the pointer (24 % 20 = 4); a momentum far from 1,
LR = 3e-6                                                 # so the EMA shows; the rate of tests/nnclr_model.py (this tiny model on
MODEL_SEED, CLIP_SEED, QUEUE_SEED = 11, 35, 2             # 8 clips is badly conditioned over several steps at larger ones)


def clip_batches(n=3, seed=CLIP_SEED):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*CLIP, generator=gen) for _ in range(n)]


def shuffles(n=3, seed=CLIP_SEED):
    gen = torch.Generator().manual_seed(seed + 1)
    return [torch.randperm(CLIP[0], generator=gen) for _ in range(n)]


def queue0(seed=QUEUE_SEED, K=QUEUE_K, D=OUT):
    return F.normalize(torch.randn(K, D, generator=torch.Generator().manual_seed(seed)))
