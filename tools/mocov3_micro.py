"""Micro-benchmark of the fused MoCo v3 loss kernels (ops.mocov3_fwd + ops.mocov3_bwd: gca_mocov3_fwd / gca_mocov3_bwd) next to the
same loss written as a chain of fp32 torch ops (two matmuls, two cross_entropy and their autograd backward: tests/mocov3_ref.py's
torch_chain), same device, same process, same inputs.

Sizes (N, D) = (256, 256), (1024, 256), (4096, 256) on the fast path and (256, 1024) on the generic one: unit rows with
cos(q, k) about 0.9, T = 0.2.  Timing: HIP events around `reps`
back-to-back calls after a warm-up of every side, the sides alternating over `rounds` rounds, median round reported with the
spread.  `launches` is the number of device kernels one forward + backward call issues, counted by torch.profiler over one
call of each side; `peak_bytes` is what one call of each side allocates at its peak (the caching allocator's high-water mark
above the inputs: the chain's N x N matrices, the fused pair's row vectors and gradients; the fused pair's workspace is
reported next to it).  The forward's 4 N^2 D FLOP over both directions (and the backward's two products each, 8 N^2 D) are
quoted against the 157.3 TF/s fp32-matrix peak.  No time here is a bar.  Needs a GPU: there is no fallback.  One process;
run it under a time limit, and start nothing on the device after it if it fails.

  python tools/mocov3_micro.py [--out profiles/mocov3_micro.json] [--rounds 5]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = [(256, 256, 200), (1024, 256, 100), (4096, 256, 20), (256, 1024, 100)]        # N, D, reps
TEMPERATURE = 0.2
PEAK_TFLOPS = 157.3


def torch_chain(q1, q2, k1, k2, T):
    target = torch.arange(q1.shape[0], device=q1.device)
    return 2 * T * (F.cross_entropy(q1 @ k2.t() / T, target) + F.cross_entropy(q2 @ k1.t() / T, target))


def unit_inputs(N, D, dev):
    """Four (N, D) matrices of unit rows, each a perturbed copy of its clip's direction (cos(q[i], k[i]) about 0.9)."""
    gen = torch.Generator(device=dev).manual_seed(1)
    base = F.normalize(torch.randn(N, D, device=dev, generator=gen))
    return [F.normalize(base + torch.randn(N, D, device=dev, generator=gen) * (0.11 / D) ** 0.5) for _ in range(4)]


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mocov3_micro.json'))
    ap.add_argument('--rounds', type=int, default=5)
    return ap


def main(argv=None):
    a = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('mocov3_micro needs a GPU (a CPU run measures nothing)')
    pkg = importlib.import_module('video-graph-ssl_amd')
    ops, dev = pkg.engine.ops, torch.device('cuda:0')
    inv_T = 1.0 / TEMPERATURE
    res = {'tool': 'tools/mocov3_micro.py', 'device': torch.cuda.get_device_name(0), 'temperature': TEMPERATURE,
           'peak_tflops_fp32_matrix': PEAK_TFLOPS, 'sizes': {},
           'timing': 'HIP events around back-to-back calls after warm-up, median of %d alternating rounds' % a.rounds}
    for N, D, reps in SIZES:
        q1, q2, k1, k2 = unit_inputs(N, D, dev)
        qg1, qg2 = q1.clone().requires_grad_(True), q2.clone().requires_grad_(True)
        ws_bytes = int(pkg._hip.lib.gca_mocov3_ws_bytes(N, D))
        ops.WS.get(ws_bytes, dev)                                        # the arena grows outside the timed region
        waves, splits = C.c_int32(-1), C.c_int32(-1)
        path = pkg._hip.lib.gca_mocov3_path(N, D, 1, C.addressof(waves), C.addressof(splits))
        _, lse0, _, _ = ops.mocov3_fwd(q1, q2, k1, k2, inv_T)

        def fused():
            loss, lse, _, _ = ops.mocov3_fwd(q1, q2, k1, k2, inv_T, want_rank=True)
            return loss, ops.mocov3_bwd(q1, q2, k1, k2, lse, inv_T)

        def chain():
            qg1.grad = qg2.grad = None
            loss = torch_chain(qg1, qg2, k1, k2, TEMPERATURE)
            loss.backward()
            return loss, (qg1.grad, qg2.grad)

        calls = {'fused': fused, 'torch_chain': chain, 'fused_fwd': lambda: ops.mocov3_fwd(q1, q2, k1, k2, inv_T, want_rank=True),
                 'fused_bwd': lambda: ops.mocov3_bwd(q1, q2, k1, k2, lse0, inv_T)}
        for fn in calls.values():                            # warm-up: code objects, the caching allocator's blocks
            fn()
            fn()
        torch.cuda.synchronize()
        (lf, gf), (lc, gc) = fused(), chain()
        agree = {'loss_abs_diff': abs(float(lf[0]) - float(lc.detach())),
                 'dq_rel_diff': max(float((a_ - b_).abs().max() / b_.abs().max()) for a_, b_ in zip(gf, gc))}
        peaks = {side: peak_bytes(calls[side]) for side in ('fused', 'torch_chain')}
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
        entry = {'N': N, 'D': D, 'reps': reps, 'path': ('generic', 'fast')[path], 'waves': waves.value, 'splits': splits.value,
                 'fused_workspace_bytes': ws_bytes, 'fused_vs_chain': agree}
        for side, ts in times.items():
            med = statistics.median(ts)
            entry[side] = {'ms_median': round(med, 5), 'ms_min': round(min(ts), 5), 'ms_max': round(max(ts), 5)}
            if side in launches:
                entry[side]['launches'] = launches[side]
                entry[side]['peak_bytes'] = peaks[side]
        for side, flop in (('fused_fwd', 4.0 * N * N * D), ('fused_bwd', 8.0 * N * N * D)):
            tf = flop / entry[side]['ms_median'] * 1e-9
            entry[side].update(tflops=round(tf, 2), fraction_of_peak=round(tf / PEAK_TFLOPS, 4))
        entry['chain_over_fused_time'] = round(entry['torch_chain']['ms_median'] / entry['fused']['ms_median'], 3)
        res['sizes']['%dx%d' % (N, D)] = entry
        print(json.dumps({'%dx%d' % (N, D): entry}), flush=True)
        del q1, q2, k1, k2, qg1, qg2, gf, gc
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
