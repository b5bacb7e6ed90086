"""Model factory (reference: lib/modeling/build.py:16-32).  Same cfg keys, same return value."""
from .graph_wrappers import GraphWrapper
from .model_wrappers import VideoModelWrapper
from .visual_wrappers import VisualModelWrapper


def _encoder(cfg):
    return VisualModelWrapper(cfg.INPUT.VIDEO_LENGTH, cfg.INPUT.MODALITY, backbone_name=cfg.MODEL.BACKBONE,
                              backbone_type=cfg.MODEL.BACKBONE_TYPE, agg_fun=cfg.MODEL.POOLING_TYPE,
                              dropout=cfg.MODEL.DROPOUT, partial_bn=not cfg.SOLVER.NO_PARTIALBN,
                              pretrained=cfg.MODEL.PRETRAINED, pretrain_path=cfg.MODEL.PRETRAIN_PATH,
                              aug_flag=bool(getattr(cfg.MODEL, 'AUG_FLAG', False)))


def create_video_model(cfg):
    """The downstream model (reference: lib/modeling/build.py:5-14): backbone + class head."""
    return VideoModelWrapper(cfg.DATASET.NUM_CLASS, cfg.INPUT.VIDEO_LENGTH, cfg.INPUT.MODALITY, backbone_name=cfg.MODEL.BACKBONE,
                             backbone_type=cfg.MODEL.BACKBONE_TYPE, agg_fun=cfg.MODEL.POOLING_TYPE, dropout=cfg.MODEL.DROPOUT,
                             partial_bn=not cfg.SOLVER.NO_PARTIALBN, pretrained=cfg.MODEL.PRETRAINED,
                             pretrain_path=cfg.MODEL.PRETRAIN_PATH)


def create_visual_model(cfg):
    """-> (model, model_ema | None); MoCo has a key encoder and DINO a momentum teacher, a second wrapper of the same layout
    (prototypes included); MoCo v3 ('mocov3': out = CROSS.FEAT_DIM, hidden width CONTRAST.V3_HID) has a momentum teacher without
    the predictor; NNCLR ('nnclr': out = CROSS.FEAT_DIM, hidden width CONTRAST.NN_HID) has no second model; ReSSL ('ressl') has MoCo's model and MoCo's key encoder as
    its momentum teacher; every other MEM_TYPE returns None.  NOTE: the
    reference never forwards MODEL.AUG_FLAG (dead code); here the flag is honoured so the graph block can actually be
    switched on."""
    model = GraphWrapper(_encoder(cfg), cfg.CROSS.FEAT_DIM, cfg.CROSS.HEAD_TYPE, cfg.CONTRAST.MEM_TYPE,
                         nce_t=cfg.CONTRAST.NCE_T, bt_lambda=getattr(cfg.CONTRAST, 'BT_LAMBDA', 0.0051),
                         vic_coeffs=tuple(getattr(cfg.CONTRAST, k, d)
                                          for k, d in (('VIC_SIM', 25.0), ('VIC_STD', 25.0), ('VIC_COV', 1.0))),
                         swav_args=tuple(getattr(cfg.CONTRAST, k, d)
                                         for k, d in (('SWAV_K', 3000), ('SWAV_EPS', 0.05), ('SWAV_T', 0.1), ('SWAV_ITERS', 3))),
                         dino_k=getattr(cfg.CONTRAST, 'DINO_K', 4096), v3_hid=getattr(cfg.CONTRAST, 'V3_HID', 4096),
                         nn_hid=getattr(cfg.CONTRAST, 'NN_HID', 2048))
    model_ema = None
    if cfg.CONTRAST.MEM_TYPE in ('moco', 'ressl'):
        model_ema = GraphWrapper(_encoder(cfg), cfg.CROSS.FEAT_DIM, cfg.CROSS.HEAD_TYPE, cfg.CONTRAST.MEM_TYPE)
    elif cfg.CONTRAST.MEM_TYPE == 'dino':
        model_ema = GraphWrapper(_encoder(cfg), cfg.CROSS.FEAT_DIM, cfg.CROSS.HEAD_TYPE, cfg.CONTRAST.MEM_TYPE,
                                 dino_k=getattr(cfg.CONTRAST, 'DINO_K', 4096))
    elif cfg.CONTRAST.MEM_TYPE == 'mocov3':
        model_ema = GraphWrapper(_encoder(cfg), cfg.CROSS.FEAT_DIM, cfg.CROSS.HEAD_TYPE, cfg.CONTRAST.MEM_TYPE,
                                 v3_hid=getattr(cfg.CONTRAST, 'V3_HID', 4096), v3_predictor=False)
    return model, model_ema
