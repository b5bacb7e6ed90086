"""Micro-benchmark of the fused class head (ops.classifier_fwd + ops.classifier_bwd: logits, cross-entropy, ranks, dw, dbias,
dx in five launches) next to torch on the same device in the same process: F.linear + F.cross_entropy + autograd for the
same three gradients.

Shapes (b, F, C): (32, 512, 101), (32, 1024, 101), (32, 2048, 400), (128, 2048, 400) and the eval-sized (4096, 1024, 101).
Timing: HIP events around `reps` back-to-back calls after a warm-up of both sides, the two sides alternating, rounds repeated
until each side has been timed for at least --window seconds; median round reported with the spread.  Needs a GPU.

  python tools/classifier_micro.py [--out profiles/classifier_micro.json] [--window 0.5]
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
SHAPES = [(32, 512, 101), (32, 1024, 101), (32, 2048, 400), (128, 2048, 400), (4096, 1024, 101)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'classifier_micro.json'))
    ap.add_argument('--window', type=float, default=0.5, help='seconds of timed calls per side and shape, at least')
    ap.add_argument('--reps', type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('classifier_micro needs a GPU (a CPU run measures nothing)')
    pkg = importlib.import_module('video-graph-ssl_amd')
    ops, dev = pkg.engine.ops, torch.device('cuda:0')
    res = {'tool': 'tools/classifier_micro.py', 'device': torch.cuda.get_device_name(0), 'shapes': {},
           'timing': 'HIP events around %d back-to-back forward + backward calls after warm-up, alternating sides, '
                     'at least %.2f s per side; median round' % (a.reps, a.window)}
    for b, Fd, Cc in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(b, Fd, device=dev, generator=gen).abs_()
        w = torch.randn(Cc, Fd, device=dev, generator=gen).mul_(0.05)
        bias = torch.randn(Cc, device=dev, generator=gen).mul_(0.1)
        tgt = torch.randint(0, Cc, (b,), device=dev, generator=gen)
        dw, db, dx = torch.empty_like(w), torch.empty_like(bias), torch.empty_like(x)
        xa, wa, ba = x.clone().requires_grad_(True), w.clone().requires_grad_(True), bias.clone().requires_grad_(True)

        def fused():
            logits, lse, rank, loss = ops.classifier_fwd(x, w, bias, tgt)
            ops.classifier_bwd(x, w, logits, lse, tgt, dw, db, False, dx, False)
            return loss

        def eager():
            loss = torch.nn.functional.cross_entropy(torch.nn.functional.linear(xa, wa, ba), tgt)
            return loss, torch.autograd.grad(loss, (wa, ba, xa))

        calls = {'fused': fused, 'torch_autograd': eager}
        for fn in calls.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        gw = eager()[1][0]
        fused()
        err = float((dw - gw).abs().max() / gw.abs().max())
        times = {side: [] for side in calls}
        while min(sum(t) for t in times.values()) * a.reps * 1e-3 < a.window:
            for side, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                e1.synchronize()
                times[side].append(e0.elapsed_time(e1) / a.reps)
        entry = {'b': b, 'F': Fd, 'C': Cc, 'reps': a.reps, 'rounds': len(times['fused']), 'dw_rel_diff_vs_torch': err}
        for side, ts in times.items():
            entry[side] = {'us_median': round(statistics.median(ts) * 1e3, 2), 'us_min': round(min(ts) * 1e3, 2),
                           'us_max': round(max(ts) * 1e3, 2)}
        entry['fused_over_torch_time'] = round(entry['fused']['us_median'] / entry['torch_autograd']['us_median'], 3)
        res['shapes']['b%d_F%d_C%d' % (b, Fd, Cc)] = entry
        print(json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
