"""Micro-benchmark of the fused SwAV kernels (ops.swav_fwd + ops.swav_bwd: gca_swav_fwd / gca_swav_bwd) next to the same
arithmetic written as a chain of fp32 torch ops (two score matmuls, the published Sinkhorn loop on each, two log-softmaxes, the
swapped terms and their autograd backward down to z1, z2 and the prototypes), same device, same process, same inputs.

Sizes (N, D, K): the workload (64, 128, 3000) and two others, (256, 128, 3000) and (32, 128, 1000); unit-row inputs
(tests/swav_ref.py: unit_inputs), eps 0.05, T 0.1, 3 Sinkhorn rounds.  Timing: HIP events around `reps` back-to-back calls
after a warm-up of every side, the sides alternating over `rounds` rounds, median round reported with the spread.  `launches`
is the number of device kernels one forward + backward call issues, counted by torch.profiler over one call of each side.
`sinkhorn` puts the Sinkhorn passes alone side by side: the device time of swav_col_kernel + swav_row_kernel per forward call
(from torch.profiler's trace, a pass of its own after the event timings; the last row pass is fused into swav_codes_kernel
and is not in this figure) next to the event time of the torch loop on both views' scores.  No time here is a bar.  Needs a
GPU: there is no fallback.

  python tools/swav_micro.py [--out profiles/swav_micro.json] [--rounds 5]
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
SIZES = [(64, 128, 3000, 200), (256, 128, 3000, 100), (32, 128, 1000, 200)]        # N, D, K, reps
PARAMS = (0.05, 0.1, 3)


def device_events(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower()
            and 'memset' not in e.name.lower()]


def kernels_us(fn, reps, names):
    """Device time (us) per call of fn spent in kernels whose name contains one of `names`, mean over `reps` calls."""
    def many():
        for _ in range(reps):
            fn()
    ts = [e.device_time for e in device_events(many) if any(n in e.name for n in names)]
    if not ts or len(ts) % reps:
        raise RuntimeError('expected a multiple of %d launches of %s in the trace, found %d' % (reps, names, len(ts)))
    return sum(ts) / reps, len(ts) // reps


def get_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'swav_micro.json'))
    ap.add_argument('--rounds', type=int, default=5)
    return ap


def main(argv=None):
    a = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('swav_micro needs a GPU (a CPU run measures nothing)')
    import swav_ref as sr
    pkg = importlib.import_module('video-graph-ssl_amd')
    ops, dev = pkg.engine.ops, torch.device('cuda:0')
    res = {'tool': 'tools/swav_micro.py', 'device': torch.cuda.get_device_name(0), 'eps_T_iters': PARAMS, 'sizes': {},
           'timing': 'HIP events around back-to-back calls after warm-up, median of %d alternating rounds; kernel times from '
                     'torch.profiler\'s device trace in a separate pass' % a.rounds}
    for N, D, K, reps in SIZES:
        z1, z2, C = (torch.from_numpy(t).to(dev) for t in sr.unit_inputs(N, D, K))
        g1, g2, gc = (t.clone().requires_grad_(True) for t in (z1, z2, C))
        ops.WS.get(int(pkg._hip.lib.gca_swav_ws_bytes(N, D, K)), dev)       # (the arena grows outside the timed region)
        _, dS0 = ops.swav_fwd(z1, z2, C, *PARAMS)
        dC = torch.empty_like(C)
        S1, S2 = z1 @ C.t(), z2 @ C.t()

        def fused():
            parts, dS = ops.swav_fwd(z1, z2, C, *PARAMS)
            return parts[0], ops.swav_bwd(z1, z2, C, dS, dC, False) + (dC,)

        def chain():
            g1.grad = g2.grad = gc.grad = None
            loss = sr.torch_chain(g1, g2, gc, *PARAMS)[0]
            loss.backward()
            return loss, (g1.grad, g2.grad, gc.grad)

        def torch_sinkhorn():
            return sr.torch_sinkhorn(S1, PARAMS[0], PARAMS[2]), sr.torch_sinkhorn(S2, PARAMS[0], PARAMS[2])

        calls = {'fused': fused, 'torch_chain': chain, 'fused_fwd': lambda: ops.swav_fwd(z1, z2, C, *PARAMS),
                 'fused_bwd': lambda: ops.swav_bwd(z1, z2, C, dS0, dC, False), 'torch_sinkhorn': torch_sinkhorn}
        for fn in calls.values():                            # warm-up: code objects, the caching allocator's blocks
            fn()
            fn()
        torch.cuda.synchronize()
        (lf, gf), (lc, gch) = fused(), chain()
        agree = {'loss_rel_diff': abs(float(lf) - float(lc.detach())) / abs(float(lc.detach())),
                 'grad_rel_diff': max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(gf, gch))}
        launches = {side: len(device_events(calls[side])) for side in ('fused', 'torch_chain', 'torch_sinkhorn')}
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
        entry = {'N': N, 'D': D, 'K': K, 'reps': reps, 'fused_vs_chain': agree, 'saved_bytes': 8 * N * K}
        for side, ts in times.items():
            med = statistics.median(ts)
            entry[side] = {'ms_median': round(med, 5), 'ms_min': round(min(ts), 5), 'ms_max': round(max(ts), 5)}
            if side in launches:
                entry[side]['launches'] = launches[side]
        entry['chain_over_fused_time'] = round(entry['torch_chain']['ms_median'] / entry['fused']['ms_median'], 3)
        sk_us, sk_launches = kernels_us(calls['fused_fwd'], reps, ('swav_col_kernel', 'swav_row_kernel'))
        entry['sinkhorn'] = {'fused_passes_device_us': round(sk_us, 2), 'fused_passes_launches': sk_launches,
                             'torch_loop_ms_median': entry['torch_sinkhorn']['ms_median'],
                             'torch_loop_launches': launches['torch_sinkhorn']}
        key = '%dx%dx%d' % (N, D, K)
        res['sizes'][key] = entry
        print(json.dumps({key: entry}), flush=True)
        del z1, z2, C, g1, g2, gc, gf, gch, dS0, dC, S1, S2
        torch.cuda.empty_cache()
    res['fused_slower_than_chain_at'] = [k for k, e in res['sizes'].items() if e['chain_over_fused_time'] < 1.0]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
