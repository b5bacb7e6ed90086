"""Micro-benchmark of the fused VICReg kernels (ops.vicreg_fwd + ops.vicreg_bwd: gca_vicreg_fwd / gca_vicreg_bwd) next to the
published loss written as a chain of fp32 torch ops (mse_loss, var, relu, two matmuls, masked off-diagonal sums and their
autograd backward), same device, same process, same inputs.

Sizes (N, D) in {32, 64, 256} x {128, 512, 2048}; inputs as a projector produces them (tests/vicreg_ref.py: float_inputs),
coefficients 25 / 25 / 1.  Timing: HIP events around `reps` back-to-back calls after a warm-up of every side, the sides
alternating over `rounds` rounds, median round reported with the spread.  `launches` is the number of device kernels one
forward + backward call issues, counted by torch.profiler over one call of each side.  The products of a step (forward: the
upper triangle of two Cov matrices, N D^2 FLOP for both views together plus the diagonal tiles; backward: 4 N D^2) are quoted
against the 157.3 TF/s fp32-matrix peak.  `cov_vs_barlow_corr` puts vicreg_cov_kernel next to barlow_corr_kernel at equal
(N, D): device time of each kernel from torch.profiler's trace, mean over `reps` forward calls, taken in a pass of its own
after the event timings (two symmetric matrices at half the tiles each against one full matrix).  No time here is a bar.
Needs a GPU: there is no fallback.

  python tools/vicreg_micro.py [--out profiles/vicreg_micro.json] [--rounds 5]
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
SIZES = [(N, D, 200 if D < 2048 else 50) for N in (32, 64, 256) for D in (128, 512, 2048)]        # N, D, reps
COEFFS = (25.0, 25.0, 1.0)
BT_LAMBDA = 0.0051
PEAK_TFLOPS = 157.3


def device_events(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower()
            and 'memset' not in e.name.lower()]


def kernel_us(fn, reps, name):
    """Mean device time (us) of the kernels whose name contains `name` over `reps` calls of fn."""
    def many():
        for _ in range(reps):
            fn()
    ts = [e.device_time for e in device_events(many) if name in e.name]
    if len(ts) != reps:
        raise RuntimeError('expected %d launches of %s in the trace, found %d' % (reps, name, len(ts)))
    return sum(ts) / len(ts)


def get_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vicreg_micro.json'))
    ap.add_argument('--rounds', type=int, default=5)
    return ap


def main(argv=None):
    a = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('vicreg_micro needs a GPU (a CPU run measures nothing)')
    import vicreg_ref as vr
    pkg = importlib.import_module('video-graph-ssl_amd')
    ops, dev = pkg.engine.ops, torch.device('cuda:0')
    res = {'tool': 'tools/vicreg_micro.py', 'device': torch.cuda.get_device_name(0), 'coeffs': COEFFS,
           'peak_tflops_fp32_matrix': PEAK_TFLOPS, 'sizes': {},
           'timing': 'HIP events around back-to-back calls after warm-up, median of %d alternating rounds; kernel times from '
                     'torch.profiler\'s device trace in a separate pass' % a.rounds}
    for N, D, reps in SIZES:
        n1, n2 = vr.float_inputs(N, D)
        z1, z2 = torch.from_numpy(n1).to(dev), torch.from_numpy(n2).to(dev)
        g1, g2 = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
        ops.WS.get(max(int(pkg._hip.lib.gca_vicreg_ws_bytes(N, D)), int(pkg._hip.lib.gca_barlow_ws_bytes(N, D))), dev)
        _, st0, c0 = ops.vicreg_fwd(z1, z2, *COEFFS)                      # (the arena grows outside the timed region)

        def fused():
            loss4, st, c = ops.vicreg_fwd(z1, z2, *COEFFS)
            return loss4[0], ops.vicreg_bwd(z1, z2, st, c, *COEFFS)

        def chain():
            g1.grad = g2.grad = None
            loss = vr.torch_chain(g1, g2, *COEFFS)[0]
            loss.backward()
            return loss, (g1.grad, g2.grad)

        calls = {'fused': fused, 'torch_chain': chain, 'fused_fwd': lambda: ops.vicreg_fwd(z1, z2, *COEFFS),
                 'fused_bwd': lambda: ops.vicreg_bwd(z1, z2, st0, c0, *COEFFS),
                 'barlow_fwd': lambda: ops.barlow_fwd(z1, z2, BT_LAMBDA)}
        for fn in calls.values():                            # warm-up: code objects, the caching allocator's blocks
            fn()
            fn()
        torch.cuda.synchronize()
        (lf, gf), (lc, gc) = fused(), chain()
        agree = {'loss_rel_diff': abs(float(lf) - float(lc.detach())) / abs(float(lc.detach())),
                 'dz_rel_diff': max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(gf, gc))}
        launches = {side: len(device_events(calls[side])) for side in ('fused', 'torch_chain')}
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
        T = -(-D // 64)
        for side, flop in (('fused_fwd', 2.0 * 2 * N * 64 * 64 * (T * (T + 1) // 2)), ('fused_bwd', 4.0 * N * D * D)):
            tf = flop / entry[side]['ms_median'] * 1e-9
            entry[side].update(tflops=round(tf, 2), fraction_of_peak=round(tf / PEAK_TFLOPS, 4))
        entry['chain_over_fused_time'] = round(entry['torch_chain']['ms_median'] / entry['fused']['ms_median'], 3)
        cov_us = kernel_us(calls['fused_fwd'], reps, 'vicreg_cov_kernel')
        corr_us = kernel_us(calls['barlow_fwd'], reps, 'barlow_corr_kernel')
        entry['cov_vs_barlow_corr'] = {'vicreg_cov_kernel_us': round(cov_us, 2), 'barlow_corr_kernel_us': round(corr_us, 2),
                                       'cov_over_corr_time': round(cov_us / corr_us, 3)}
        res['sizes']['%dx%d' % (N, D)] = entry
        print(json.dumps({'%dx%d' % (N, D): entry}), flush=True)
        del z1, z2, g1, g2, gf, gc, st0, c0
        torch.cuda.empty_cache()
    res['fused_slower_than_chain_at'] = [k for k, e in res['sizes'].items() if e['chain_over_fused_time'] < 1.0]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
