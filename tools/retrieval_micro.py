"""Micro-benchmark of ops.retrieval_topk (gca_retrieval_topk: fused distance + top-k) next to the unfused baseline on the same
device in the same process: row-normalise, torch.matmul -> the full (nq, ng) distance matrix, torch.topk.

Shapes: UCF101 split 1 with S3D features (nq = 3783, ng = 9537, D = 1024), the same at D = 512 and D = 128, and a
Kinetics-sized gallery (nq = 4096, ng = 240000, D = 1024); k = 50, cosine.  Timing: HIP events around `reps` back-to-back
calls after a warm-up of both sides, the two sides alternating over `rounds` rounds, median round reported with the
spread.  TF/s counts 2 nq ng D and is quoted against the 157.3 TF/s fp32-MFMA peak.  Peak bytes: the growth of
torch.cuda.max_memory_allocated over the inputs (fused: workspace + outputs; baseline: normalised copies + the matrix +
top-k outputs).  Needs a GPU: there is no fallback.

  python tools/retrieval_micro.py [--out profiles/retrieval_micro.json] [--rounds 5] [--skip-large]
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
PEAK_TFLOPS = 157.3
SHAPES = [('ucf101_s3d_D1024', 3783, 9537, 1024, 20), ('ucf101_D512', 3783, 9537, 512, 20), ('ucf101_D128', 3783, 9537, 128, 20),
          ('kinetics_gallery_D1024', 4096, 240000, 1024, 2)]


def baseline(q, g, k):
    qn = torch.nn.functional.normalize(q, dim=1)
    gn = torch.nn.functional.normalize(g, dim=1)
    d = torch.matmul(qn, gn.t()).mul_(-1.0).add_(1.0)
    return torch.topk(d, k, dim=1, largest=False, sorted=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'retrieval_micro.json'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--skip-large', action='store_true', help='leave out the 240000-row gallery')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('retrieval_micro needs a GPU (a CPU run measures nothing)')
    pkg = importlib.import_module('video-graph-ssl_amd')
    ops, dev, k = pkg.engine.ops, torch.device('cuda:0'), a.k
    res = {'tool': 'tools/retrieval_micro.py', 'device': torch.cuda.get_device_name(0), 'k': k, 'metric': 'cosine',
           'peak_tflops_fp32_mfma': PEAK_TFLOPS, 'shapes': {},
           'timing': 'HIP events around back-to-back calls after warm-up, median of %d alternating rounds' % a.rounds}
    for name, nq, ng, D, reps in SHAPES:
        if a.skip_large and ng > 100000:
            continue
        gen = torch.Generator(device=dev).manual_seed(1)
        q = torch.randn(nq, D, device=dev, generator=gen)
        g = torch.randn(ng, D, device=dev, generator=gen)
        ws_bytes = int(pkg._hip.lib.gca_retrieval_ws_bytes(nq, ng, D, k, 0))
        ops.WS.get(ws_bytes, dev)                       # the arena grows once, outside the timed region
        calls = {'fused': lambda: ops.retrieval_topk(q, g, k, 'cosine'), 'matmul_topk': lambda: baseline(q, g, k)}
        peak = {}
        for side, fn in calls.items():                  # warm-up (code objects, GEMM selection) and peak bytes
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = fn()
            torch.cuda.synchronize()
            peak[side] = int(torch.cuda.max_memory_allocated() - base)
            del out
            fn()
        peak['fused'] += ws_bytes                       # the arena was allocated before `base`
        torch.cuda.synchronize()
        times = {side: [] for side in calls}
        for _ in range(a.rounds):
            for side, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                times[side].append(e0.elapsed_time(e1) / reps)
        fi, bi = ops.retrieval_topk(q, g, k, 'cosine')[0], baseline(q, g, k)[1]
        agree = float((fi.long() == bi).float().mean())
        flop = 2.0 * nq * ng * D
        entry = {'nq': nq, 'ng': ng, 'D': D, 'reps': reps, 'matrix_bytes': nq * ng * 4, 'fused_ws_bytes': ws_bytes,
                 'index_agreement_with_baseline': round(agree, 6)}
        for side, ts in times.items():
            med = statistics.median(ts)
            entry[side] = {'ms_median': round(med, 4), 'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4),
                           'tflops': round(flop / med * 1e-9, 2), 'fraction_of_fp32_mfma_peak': round(flop / med * 1e-9 / PEAK_TFLOPS, 4),
                           'peak_bytes': peak[side]}
        entry['fused_over_baseline_time'] = round(entry['fused']['ms_median'] / entry['matmul_topk']['ms_median'], 3)
        res['shapes'][name] = entry
        print(json.dumps({name: entry}), flush=True)
        del q, g, fi, bi
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
