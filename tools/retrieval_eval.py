"""R@1/5/10/20/50 of pickled validation features against pickled training features: the search half of the reference's
tools/video_retrieval.py (its mode without --extract_feature), on the fused distance / top-k kernel.  Argument and file
names are the reference's; features come from lib.evaluation.retrieval.extract_features (or from the reference itself:
the pickles are plain numpy arrays).  Needs a GPU: there is no fallback.

  python tools/retrieval_eval.py --train_feature_path train_features.pkl --train_classes_path train_classes.pkl \\
      --val_feature_path val_features.pkl --val_classes_path val_classes.pkl [--distance_metric cosine|euclidean] [--norm] \\
      --save_scores OUT_DIR
"""
import argparse
import importlib
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def get_parser():
    ap = argparse.ArgumentParser(description='video retrieval: top-k search of validation features in training features')
    ap.add_argument('--train_feature_path', required=True)
    ap.add_argument('--train_classes_path', required=True)
    ap.add_argument('--val_feature_path', required=True)
    ap.add_argument('--val_classes_path', required=True)
    ap.add_argument('--distance_metric', default='cosine', choices=['cosine', 'euclidean'])
    ap.add_argument('--norm', action='store_true', default=False, help='L2-normalise both feature sets first')
    ap.add_argument('--save_scores', default='.', help='directory that receives topk_correct.json')
    return ap


def load_pickle(path):
    with open(path, 'rb') as fh:
        return pickle.load(fh)


def main(argv=None):
    a = get_parser().parse_args(argv)
    retrieval = importlib.import_module('video-graph-ssl_amd').lib.evaluation.retrieval
    correct, total = retrieval.topk_retrieval(load_pickle(a.train_feature_path), load_pickle(a.train_classes_path),
                                              load_pickle(a.val_feature_path), load_pickle(a.val_classes_path),
                                              metric=a.distance_metric, norm=a.norm)
    for k, c in correct.items():
        print('Top-%d, correct = %d, total = %d, acc = %.3f' % (k, c, total, c / max(total, 1)))
    os.makedirs(a.save_scores, exist_ok=True)
    out = os.path.join(a.save_scores, 'topk_correct.json')
    with open(out, 'w') as fh:
        json.dump(correct, fh)
    return out


if __name__ == '__main__':
    main()
