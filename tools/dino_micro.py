"""Micro-benchmark of the fused DINO kernels (ops.dino_fwd + ops.dino_bwd: gca_dino_fwd / gca_swav_bwd) next to the same
arithmetic written as a chain of fp32 torch ops (four score matmuls, the centred teacher softmax, two log-softmaxes, the cross
terms, the entropy, the centre's EMA and the autograd backward down to zs1, zs2 and the student prototypes), same device, same
process, same inputs.

Sizes (N, D, K): the default workload (64, 128, 4096) and the largest head (64, 128, 65536); unit-row inputs
(tests/dino_ref.py: unit_inputs), Ts 0.1, Tt 0.04, cm 0.9.  Timing: HIP events around `reps` back-to-back calls after a warm-up
of every side, the sides alternating over `rounds` rounds, median round reported with the spread.  `launches` is the number of
device kernels one forward + backward call issues, counted by torch.profiler over one call of each side.  `row_kernel` puts
the two grids of the row launch side by side -- a 256-thread workgroup per row and direction (what gca_dino_fwd uses) and one
wave per row and direction (SwAV's grid, gca_dino_fwd_grid) -- as device time of dino_row_kernel per forward call, and
`kernels_us` lists every kernel of the fused pair (both from torch.profiler's trace, a pass of its own after the event
timings).  No time here is a bar.  Needs a GPU: there is no fallback.

  python tools/dino_micro.py [--out profiles/dino_micro.json] [--rounds 5]
"""
import argparse
import importlib
import json
import os
import re
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
SIZES = [(64, 128, 4096, 200), (64, 128, 65536, 40)]        # N, D, K, reps
PARAMS = (0.1, 0.04, 0.9)


def device_events(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower()
            and 'memset' not in e.name.lower()]


def kernel_times(fn, reps):
    """Device time (us) per call of fn by kernel, mean over `reps` calls -> {short kernel name: (us, launches per call)}."""
    def many():
        for _ in range(reps):
            fn()
    acc = {}
    for e in device_events(many):
        m = re.search(r'(\w+)\s*(?:<[^()]*>)?\s*\(', e.name.replace('(anonymous namespace)::', ''))
        name = m.group(1) if m else e.name
        t, n = acc.get(name, (0.0, 0))
        acc[name] = (t + e.device_time, n + 1)
    return {k: (round(t / reps, 2), n / reps) for k, (t, n) in acc.items()}


def get_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dino_micro.json'))
    ap.add_argument('--rounds', type=int, default=5)
    return ap


def main(argv=None):
    a = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('dino_micro needs a GPU (a CPU run measures nothing)')
    import dino_ref as dr
    pkg = importlib.import_module('video-graph-ssl_amd')
    ops, dev = pkg.engine.ops, torch.device('cuda:0')
    Ts, Tt, cm = PARAMS
    res = {'tool': 'tools/dino_micro.py', 'device': torch.cuda.get_device_name(0), 'Ts_Tt_cm': PARAMS, 'sizes': {},
           'timing': 'HIP events around back-to-back calls after warm-up, median of %d alternating rounds; kernel times from '
                     'torch.profiler\'s device trace in a separate pass' % a.rounds}
    for N, D, K, reps in SIZES:
        zs1, zs2, Cs, zt1, zt2, Ct, c0 = (torch.from_numpy(t).to(dev) for t in dr.unit_inputs(N, D, K))
        g1, g2, gc = (t.clone().requires_grad_(True) for t in (zs1, zs2, Cs))
        tt = torch.tensor([Tt], device=dev)
        center = c0.clone()
        ops.WS.get(max(int(pkg._hip.lib.gca_dino_ws_bytes(N, D, K)), int(pkg._hip.lib.gca_swav_ws_bytes(N, D, K))), dev)
        dC = torch.empty_like(Cs)

        def fwd(grid=None):
            return ops.dino_fwd(zs1, zs2, Cs, zt1, zt2, Ct, Ts, tt, cm, center, True, row_grid=grid)

        _, dS0 = fwd()

        def fused(grid=None):
            parts, dS = fwd(grid)
            return parts[0], ops.dino_bwd(zs1, zs2, Cs, dS, dC, False) + (dC,)

        def chain():
            g1.grad = g2.grad = gc.grad = None
            loss, _, _, _, new_c = dr.torch_chain(g1, g2, gc, zt1, zt2, Ct, center, Ts, Tt, cm)
            loss.backward()
            center.copy_(new_c)
            return loss, (g1.grad, g2.grad, gc.grad)

        calls = {'fused': fused, 'fused_wave_rows': lambda: fused(1), 'torch_chain': chain, 'fused_fwd': fwd,
                 'fused_fwd_wave_rows': lambda: fwd(1), 'fused_bwd': lambda: ops.dino_bwd(zs1, zs2, Cs, dS0, dC, False)}
        for fn in calls.values():                            # warm-up: code objects, the caching allocator's blocks
            fn()
            fn()
        torch.cuda.synchronize()
        center.copy_(c0)
        lf, gf = fused()
        gf = tuple(t.clone() for t in gf)
        center.copy_(c0)
        lc, gch = chain()
        agree = {'loss_rel_diff': abs(float(lf) - float(lc.detach())) / abs(float(lc.detach())),
                 'grad_rel_diff': max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(gf, gch))}
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
        entry = {'N': N, 'D': D, 'K': K, 'reps': reps, 'fused_vs_chain': agree, 'saved_bytes': 8 * N * K}
        for side, ts in times.items():
            med = statistics.median(ts)
            entry[side] = {'ms_median': round(med, 5), 'ms_min': round(min(ts), 5), 'ms_max': round(max(ts), 5)}
            if side in launches:
                entry[side]['launches'] = launches[side]
        entry['chain_over_fused_time'] = round(entry['torch_chain']['ms_median'] / entry['fused']['ms_median'], 3)
        kt = kernel_times(calls['fused'], reps)
        kw = kernel_times(calls['fused_fwd_wave_rows'], reps)
        entry['kernels_us'] = {k: v[0] for k, v in sorted(kt.items())}
        entry['row_kernel'] = {'workgroup_per_row_device_us': kt['dino_row_kernel'][0], 'wave_per_row_device_us': kw['dino_row_kernel'][0],
                               'workgroups': {'workgroup_per_row': 2 * N, 'wave_per_row': 2 * ((N + 3) // 4)}}
        key = '%dx%dx%d' % (N, D, K)
        res['sizes'][key] = entry
        print(json.dumps({key: entry}), flush=True)
        del zs1, zs2, Cs, zt1, zt2, Ct, g1, g2, gc, gf, gch, dS0, dC
        torch.cuda.empty_cache()
    res['fused_slower_than_chain_at'] = [k for k, e in res['sizes'].items() if e['chain_over_fused_time'] < 1.0]
    res['row_grid_in_use'] = 'workgroup_per_row'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
