"""Weighted k-NN classification of pickled validation features by pickled training features: the evaluation
self-supervised code bases report next to the linear probe (each of the k nearest training videos votes for its class with
weight exp(sim / T); top-1 / top-5 of the vote).  The four pickle arguments are those of tools/retrieval_eval.py; the
features come from lib.evaluation.retrieval.extract_features.  Cosine distance; k <= 64.  Needs a GPU: there is no fallback.

  python tools/knn_eval.py --train_feature_path train_features.pkl --train_classes_path train_classes.pkl \\
      --val_feature_path val_features.pkl --val_classes_path val_classes.pkl [--k 20 --k 10 ...] [--temperature 0.07] \\
      [--weighting exp|uniform] [--num_class N] --save_scores OUT_DIR
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

DEFAULT_KS = (1, 5, 10, 20)


def get_parser():
    ap = argparse.ArgumentParser(description='weighted k-NN classification of validation features by training features')
    ap.add_argument('--train_feature_path', required=True)
    ap.add_argument('--train_classes_path', required=True)
    ap.add_argument('--val_feature_path', required=True)
    ap.add_argument('--val_classes_path', required=True)
    ap.add_argument('--k', type=int, action='append', default=None,
                    help='neighbours that vote, in [1, 64]; repeat for several (default: %s)' % ' '.join(map(str, DEFAULT_KS)))
    ap.add_argument('--temperature', type=float, default=0.07)
    ap.add_argument('--weighting', default='exp', choices=['exp', 'uniform'])
    ap.add_argument('--num_class', type=int, default=None, help='default: the largest label + 1')
    ap.add_argument('--save_scores', default='.', help='directory that receives knn_correct.json')
    return ap


def ks_of(args):
    return tuple(args.k) if args.k else DEFAULT_KS


def report(correct, total, temperature, weighting):
    """What knn_correct.json holds: {'total', 'temperature', 'weighting', 'k': {'<k>': {'top1': n, 'top5': n}}}."""
    return {'total': int(total), 'temperature': float(temperature), 'weighting': weighting,
            'k': {str(int(k)): {'top1': int(v['top1']), 'top5': int(v['top5'])} for k, v in correct.items()}}


def lines(correct, total):
    return ['k = %d: top-1 correct = %d, top-5 correct = %d, total = %d, top-1 = %.3f, top-5 = %.3f'
            % (k, v['top1'], v['top5'], total, v['top1'] / max(total, 1), v['top5'] / max(total, 1)) for k, v in correct.items()]


def load_pickle(path):
    with open(path, 'rb') as fh:
        return pickle.load(fh)


def main(argv=None):
    a = get_parser().parse_args(argv)
    knn = importlib.import_module('video-graph-ssl_amd').lib.evaluation.knn
    correct, total = knn.knn_classify(load_pickle(a.train_feature_path), load_pickle(a.train_classes_path),
                                      load_pickle(a.val_feature_path), load_pickle(a.val_classes_path), num_class=a.num_class,
                                      ks=ks_of(a), T=a.temperature, weighting=a.weighting)
    for line in lines(correct, total):
        print(line)
    os.makedirs(a.save_scores, exist_ok=True)
    out = os.path.join(a.save_scores, 'knn_correct.json')
    with open(out, 'w') as fh:
        json.dump(report(correct, total, a.temperature, a.weighting), fh)
    return out


if __name__ == '__main__':
    main()
