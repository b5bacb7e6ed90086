from .metric import AverageMeter, accuracy, accuracy_from_rank, rank_ge  # noqa: F401
from .retrieval import (encoder_state_dict, extract_feature_single, extract_features, load_encoder,  # noqa: F401
                        recall_counts, topk_retrieval)
from . import retrieval  # noqa: F401
from .classify import eval_video, evaluate  # noqa: F401
from . import classify  # noqa: F401
from .knn import KNNMonitor, features_of, knn_classify, knn_classify_loo, knn_predict  # noqa: F401
from . import knn  # noqa: F401
