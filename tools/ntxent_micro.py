"""Micro-benchmark of the fused NT-Xent kernels (ops.ntxent_fwd + ops.ntxent_bwd: gca_ntxent_fwd / gca_ntxent_bwd) next to the
same loss written as a chain of torch ops (matmul, diagonal mask, cross_entropy and their autograd backward), same device,
same process, same inputs.

Sizes (N, D) = (64, 128), (512, 128), (2048, 128), (8192, 128): unit rows, T = 0.07.  Timing: HIP events around `reps`
back-to-back calls after a warm-up of every side, the sides alternating over `rounds` rounds, median round reported with the
spread.  `launches` is the number of device kernels one forward + backward call issues, counted by torch.profiler over one
call of each side.  The forward's 2 N^2 D FLOP (and the backward's two products, 4 N^2 D) are quoted against the 157.3 TF/s
fp32-matrix peak.  No time here is a bar.  Needs a GPU: there is no fallback.

  python tools/ntxent_micro.py [--out profiles/ntxent_micro.json] [--rounds 5]
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
SIZES = [(64, 128, 200), (512, 128, 200), (2048, 128, 50), (8192, 128, 10)]        # N, D, reps
TEMPERATURE = 0.07
PEAK_TFLOPS = 157.3


def torch_chain(z, inv_T):
    N = z.shape[0]
    s = (z @ z.t()) * inv_T
    s = s.masked_fill(torch.eye(N, dtype=torch.bool, device=z.device), float('-inf'))
    return F.cross_entropy(s, (torch.arange(N, device=z.device) + N // 2) % N)


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ntxent_micro.json'))
    ap.add_argument('--rounds', type=int, default=5)
    return ap


def main(argv=None):
    a = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('ntxent_micro needs a GPU (a CPU run measures nothing)')
    pkg = importlib.import_module('video-graph-ssl_amd')
    ops, dev = pkg.engine.ops, torch.device('cuda:0')
    inv_T = 1.0 / TEMPERATURE
    res = {'tool': 'tools/ntxent_micro.py', 'device': torch.cuda.get_device_name(0), 'temperature': TEMPERATURE,
           'peak_tflops_fp32_matrix': PEAK_TFLOPS, 'sizes': {},
           'timing': 'HIP events around back-to-back calls after warm-up, median of %d alternating rounds' % a.rounds}
    for N, D, reps in SIZES:
        gen = torch.Generator(device=dev).manual_seed(1)
        z = F.normalize(torch.randn(N, D, device=dev, generator=gen))
        zg = z.clone().requires_grad_(True)
        ops.WS.get(int(pkg._hip.lib.gca_ntxent_ws_bytes(N, D)), dev)          # the arena grows outside the timed region
        _, lse0, _ = ops.ntxent_fwd(z, inv_T)

        def fused():
            loss, lse, _ = ops.ntxent_fwd(z, inv_T, want_rank=True)
            return loss, ops.ntxent_bwd(z, lse, inv_T)

        def chain():
            zg.grad = None
            loss = torch_chain(zg, inv_T)
            loss.backward()
            return loss, zg.grad

        calls = {'fused': fused, 'torch_chain': chain, 'fused_fwd': lambda: ops.ntxent_fwd(z, inv_T, want_rank=True),
                 'fused_bwd': lambda: ops.ntxent_bwd(z, lse0, inv_T)}
        for fn in calls.values():                            # warm-up: code objects, the caching allocator's blocks
            fn()
            fn()
        torch.cuda.synchronize()
        (lf, gf), (lc, gc) = fused(), chain()
        agree = {'loss_abs_diff': abs(float(lf) - float(lc.detach())), 'dz_rel_diff': float((gf - gc).abs().max() / gc.abs().max())}
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
        for side, flop in (('fused_fwd', 2.0 * N * N * D), ('fused_bwd', 4.0 * N * N * D)):
            tf = flop / entry[side]['ms_median'] * 1e-9
            entry[side].update(tflops=round(tf, 2), fraction_of_peak=round(tf / PEAK_TFLOPS, 4))
        entry['chain_over_fused_time'] = round(entry['torch_chain']['ms_median'] / entry['fused']['ms_median'], 3)
        res['sizes']['%dx%d' % (N, D)] = entry
        print(json.dumps({'%dx%d' % (N, D): entry}), flush=True)
        del z, zg, gf, gc
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
