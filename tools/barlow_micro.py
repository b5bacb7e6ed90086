"""Micro-benchmark of the fused Barlow Twins kernels (ops.barlow_fwd + ops.barlow_bwd: gca_barlow_fwd / gca_barlow_bwd) next to
the same loss written as a chain of fp32 torch ops (batch_norm of each view, matmul, diagonal / off-diagonal sums and their
autograd backward), same device, same process, same inputs.

Sizes (N, D) in {32, 64, 256} x {128, 512, 2048}; inputs as a projector produces them (tests/barlow_ref.py: float_inputs),
lambda = 0.0051.  Timing: HIP events around `reps` back-to-back calls after a warm-up of every side, the sides alternating over
`rounds` rounds, median round reported with the spread.  `launches` is the number of device kernels one forward + backward
call issues, counted by torch.profiler over one call of each side.  The three products of a step (2 N D^2 FLOP each) are
quoted against the 157.3 TF/s fp32-matrix peak.  No time here is a bar.  Needs a GPU: there is no fallback.

  python tools/barlow_micro.py [--out profiles/barlow_micro.json] [--rounds 5]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
SIZES = [(N, D, 200 if D < 2048 else 50) for N in (32, 64, 256) for D in (128, 512, 2048)]        # N, D, reps
LAMBDA = 0.0051
PEAK_TFLOPS = 157.3


def torch_chain(z1, z2, lambd, eps=1e-5):
    N, D = z1.shape
    a = F.batch_norm(z1, None, None, training=True, eps=eps)
    b = F.batch_norm(z2, None, None, training=True, eps=eps)
    c = (a.t() @ b) / N
    on = (torch.diagonal(c) - 1).pow(2).sum()
    off = c.masked_fill(torch.eye(D, dtype=torch.bool, device=c.device), 0).pow(2).sum()
    return on + lambd * off


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower()
               and 'memset' not in e.name.lower())


def get_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'barlow_micro.json'))
    ap.add_argument('--rounds', type=int, default=5)
    return ap


def main(argv=None):
    a = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('barlow_micro needs a GPU (a CPU run measures nothing)')
    import barlow_ref as br
    pkg = importlib.import_module('video-graph-ssl_amd')
    ops, dev = pkg.engine.ops, torch.device('cuda:0')
    res = {'tool': 'tools/barlow_micro.py', 'device': torch.cuda.get_device_name(0), 'lambda': LAMBDA,
           'peak_tflops_fp32_matrix': PEAK_TFLOPS, 'sizes': {},
           'timing': 'HIP events around back-to-back calls after warm-up, median of %d alternating rounds' % a.rounds}
    for N, D, reps in SIZES:
        n1, n2 = br.float_inputs(N, D)
        z1, z2 = torch.from_numpy(n1).to(dev), torch.from_numpy(n2).to(dev)
        g1, g2 = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
        ops.WS.get(int(pkg._hip.lib.gca_barlow_ws_bytes(N, D)), dev)          # the arena grows outside the timed region
        _, st0, c0, r0 = ops.barlow_fwd(z1, z2, LAMBDA)

        def fused():
            loss3, st, c, r = ops.barlow_fwd(z1, z2, LAMBDA)
            return loss3[0], ops.barlow_bwd(z1, z2, st, c, r, LAMBDA)

        def chain():
            g1.grad = g2.grad = None
            loss = torch_chain(g1, g2, LAMBDA)
            loss.backward()
            return loss, (g1.grad, g2.grad)

        calls = {'fused': fused, 'torch_chain': chain, 'fused_fwd': lambda: ops.barlow_fwd(z1, z2, LAMBDA),
                 'fused_bwd': lambda: ops.barlow_bwd(z1, z2, st0, c0, r0, LAMBDA)}
        for fn in calls.values():                            # warm-up: code objects, the caching allocator's blocks
            fn()
            fn()
        torch.cuda.synchronize()
        (lf, gf), (lc, gc) = fused(), chain()
        agree = {'loss_rel_diff': abs(float(lf) - float(lc.detach())) / abs(float(lc.detach())),
                 'dz_rel_diff': max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(gf, gc))}
        launches = {side: count_launches(calls[side]) for side in ('fused', 'torch_chain')}
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
        entry = {'N': N, 'D': D, 'reps': reps, 'fused_vs_chain': agree}
        for side, ts in times.items():
            med = statistics.median(ts)
            entry[side] = {'ms_median': round(med, 5), 'ms_min': round(min(ts), 5), 'ms_max': round(max(ts), 5)}
            if side in launches:
                entry[side]['launches'] = launches[side]
        for side, flop in (('fused_fwd', 2.0 * N * D * D), ('fused_bwd', 4.0 * N * D * D)):
            tf = flop / entry[side]['ms_median'] * 1e-9
            entry[side].update(tflops=round(tf, 2), fraction_of_peak=round(tf / PEAK_TFLOPS, 4))
        entry['chain_over_fused_time'] = round(entry['torch_chain']['ms_median'] / entry['fused']['ms_median'], 3)
        res['sizes']['%dx%d' % (N, D)] = entry
        print(json.dumps({'%dx%d' % (N, D): entry}), flush=True)
        del z1, z2, g1, g2, gf, gc
        torch.cuda.empty_cache()
    slower = [k for k, e in res['sizes'].items() if e['chain_over_fused_time'] < 1.0]
    res['fused_slower_than_chain_at'] = slower
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
