"""Factories (reference: lib/memory/build.py).  Only what the pre-training configs select is on the
HIP path: MEM_TYPE 'moco' (visual) / 'simsiam' / 'simclr' (in-batch NT-Xent: no memory, the loss module itself) /
'barlow' (Barlow Twins' cross-correlation loss, likewise the loss module itself) / 'vicreg' (the variance / invariance /
covariance loss, likewise) / 'swav' (the swapped-prediction loss, likewise; the prototypes live in the model) / 'dino' (the centred-teacher
self-distillation loss; its centre is the module's one buffer) / 'mocov3' (MoCo v3's symmetrised cross-view InfoNCE at
CONTRAST.NCE_T: no queue, the loss module itself; the momentum teacher is the second model of create_visual_model) / 'nnclr' (nearest-neighbour contrast against a support set:
a FIFO of CONTRAST.NCE_K projections of width CROSS.FEAT_DIM, temperature CONTRAST.NCE_T) / 'ressl' (the relational loss over
the MoCo queue: CONTRAST.NCE_K anchors of width CROSS.FEAT_DIM, student / teacher temperatures CONTRAST.RESSL_TS / RESSL_TT; the
momentum teacher is the second model of create_visual_model), CRITERION 'crossentropy'."""
from .barlow import BarlowTwinsLoss
from .criterion import NCESoftmaxLoss
from .dino import DINOLoss
from .mem_moco import RGBMoCo
from .mocov3 import MoCoV3Loss
from .nnclr import NNCLRLoss
from .ntxent import NTXent
from .ressl import ReSSLLoss
from .swav import SwAVLoss
from .vicreg import VICRegLoss


def create_contrast(cfg, n_data):
    if cfg.CONTRAST.MEM_TYPE == 'moco':
        if cfg.CROSS.MODALITY != 'visual':
            raise NotImplementedError('two-modality CMCMoCo is outside the hot path (CROSS.MODALITY is always visual)')
        return RGBMoCo(cfg.CROSS.FEAT_DIM, cfg.CONTRAST.NCE_K, cfg.CONTRAST.NCE_T)
    if cfg.CONTRAST.MEM_TYPE == 'simsiam':
        return None
    if cfg.CONTRAST.MEM_TYPE == 'simclr':
        return NTXent(cfg.CONTRAST.NCE_T)
    if cfg.CONTRAST.MEM_TYPE == 'barlow':
        return BarlowTwinsLoss(cfg.CONTRAST.BT_LAMBDA)
    if cfg.CONTRAST.MEM_TYPE == 'vicreg':
        return VICRegLoss(cfg.CONTRAST.VIC_SIM, cfg.CONTRAST.VIC_STD, cfg.CONTRAST.VIC_COV)
    if cfg.CONTRAST.MEM_TYPE == 'swav':
        return SwAVLoss(cfg.CONTRAST.SWAV_EPS, cfg.CONTRAST.SWAV_T, cfg.CONTRAST.SWAV_ITERS)
    if cfg.CONTRAST.MEM_TYPE == 'dino':
        return DINOLoss(cfg.CONTRAST.DINO_K, cfg.CONTRAST.DINO_TS, cfg.CONTRAST.DINO_TT, cfg.CONTRAST.DINO_CM)
    if cfg.CONTRAST.MEM_TYPE == 'mocov3':
        return MoCoV3Loss(cfg.CONTRAST.NCE_T)
    if cfg.CONTRAST.MEM_TYPE == 'nnclr':
        return NNCLRLoss(cfg.CROSS.FEAT_DIM, cfg.CONTRAST.NCE_K, cfg.CONTRAST.NCE_T)
    if cfg.CONTRAST.MEM_TYPE == 'ressl':
        return ReSSLLoss(cfg.CROSS.FEAT_DIM, cfg.CONTRAST.NCE_K, cfg.CONTRAST.RESSL_TS, cfg.CONTRAST.RESSL_TT)
    raise NotImplementedError('mem not suported: {}'.format(cfg.CONTRAST.MEM_TYPE))


def create_criterion(cfg, n_data):
    if cfg.CROSS.CRITERION == 'crossentropy':
        return NCESoftmaxLoss()
    raise NotImplementedError('criterion not suported: {}'.format(cfg.CROSS.CRITERION))
