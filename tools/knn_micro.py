"""Micro-benchmark of ops.knn_vote (gca_knn_vote) next to the search it follows (ops.retrieval_topk), same device, same
process, on the lists that very search wrote.

Shapes: UCF101 split 1 (nq = 3783, ng = 9537, C = 101) at D = 512 and D = 1024, and a Kinetics-400-like shape (nq = 19761,
ng = 240000, D = 2048, C = 400); k = 20, cosine, exp weights at T = 0.07; the vote with and without the (nq, C) score block.
Timing: HIP events around `reps` back-to-back calls after a warm-up of every side, the sides alternating over `rounds`
rounds, median round reported with the spread.  Bytes: what the vote has to move, from the shapes -- nq * k * 8 of lists,
nq * k * 8 of gathered labels, nq * 8 of query labels, nq * 8 of pred / rank, and nq * C * 4 of scores when asked for;
GB/s is that over the median call time (a call is one or two launches: for the small shape mostly launch overhead).
No time here is a bar.  Needs a GPU: there is no fallback.

  python tools/knn_micro.py [--out profiles/knn_micro.json] [--rounds 5] [--skip-large]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# name, nq, ng, D, C, search reps, vote reps
SHAPES = [('ucf101_D512', 3783, 9537, 512, 101, 20, 200), ('ucf101_D1024', 3783, 9537, 1024, 101, 20, 200),
          ('kinetics400_D2048', 19761, 240000, 2048, 400, 1, 200)]
K, TEMPERATURE = 20, 0.07


def vote_bytes(nq, k, C, scores):
    return nq * k * 8 + nq * k * 8 + nq * 8 + nq * 8 + (nq * C * 4 if scores else 0)


def get_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'knn_micro.json'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--skip-large', action='store_true', help='leave out the 240000-row gallery')
    return ap


def main(argv=None):
    a = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('knn_micro needs a GPU (a CPU run measures nothing)')
    pkg = importlib.import_module('video-graph-ssl_amd')
    ops, dev = pkg.engine.ops, torch.device('cuda:0')
    res = {'tool': 'tools/knn_micro.py', 'device': torch.cuda.get_device_name(0), 'k': K, 'metric': 'cosine', 'weighting': 'exp',
           'temperature': TEMPERATURE, 'shapes': {},
           'timing': 'HIP events around back-to-back calls after warm-up, median of %d alternating rounds' % a.rounds}
    for name, nq, ng, D, C, sreps, vreps in SHAPES:
        if a.skip_large and ng > 100000:
            continue
        gen = torch.Generator(device=dev).manual_seed(1)
        q = torch.randn(nq, D, device=dev, generator=gen)
        g = torch.randn(ng, D, device=dev, generator=gen)
        gl = torch.randint(0, C, (ng,), device=dev, generator=gen)
        ql = torch.randint(0, C, (nq,), device=dev, generator=gen)
        ops.WS.get(int(pkg._hip.lib.gca_retrieval_ws_bytes(nq, ng, D, K, 0)), dev)      # the arena grows outside the timed region
        idx, dist, _ = ops.retrieval_topk(q, g, K, 'cosine')
        calls = {'search': (sreps, lambda: ops.retrieval_topk(q, g, K, 'cosine')),
                 'vote': (vreps, lambda: ops.knn_vote(idx, dist, gl, C, q_label=ql, T=TEMPERATURE)),
                 'vote_scores': (vreps, lambda: ops.knn_vote(idx, dist, gl, C, q_label=ql, T=TEMPERATURE, want_scores=True))}
        for _, fn in calls.values():                        # warm-up: code objects, the caching allocator's blocks
            fn()
            fn()
        torch.cuda.synchronize()
        times = {side: [] for side in calls}
        for _ in range(a.rounds):
            for side, (reps, fn) in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                times[side].append(e0.elapsed_time(e1) / reps)
        entry = {'nq': nq, 'ng': ng, 'D': D, 'C': C}
        for side, ts in times.items():
            med = statistics.median(ts)
            entry[side] = {'reps': calls[side][0], 'ms_median': round(med, 5), 'ms_min': round(min(ts), 5), 'ms_max': round(max(ts), 5)}
            if side != 'search':
                nbytes = vote_bytes(nq, K, C, side == 'vote_scores')
                entry[side].update(bytes=nbytes, gb_per_s=round(nbytes / med * 1e-6, 2))
        entry['vote_over_search_time'] = round(entry['vote']['ms_median'] / entry['search']['ms_median'], 6)
        entry['vote_scores_over_search_time'] = round(entry['vote_scores']['ms_median'] / entry['search']['ms_median'], 6)
        res['shapes'][name] = entry
        print(json.dumps({name: entry}), flush=True)
        del q, g, idx, dist
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
