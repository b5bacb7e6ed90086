"""Micro-benchmark of the fused arena updates: gca_adam_step + gca_adam_advance (Adam and AdamW) and gca_lars_step (LARS: norm
pass, trust ratios, update) next to gca_sgd_step, in one process, on an arena the size of the R(2+1)D-18 MoCo model's (the model is built on the host for its layout only).

Bytes moved per element: SGD reads p, g, buf and writes p, buf (20 B); Adam reads p, g, m, v and writes p, m, v (28 B); LARS
reads p and g once more for the norms on top of SGD's traffic (28 B); the chunk tables (8 - 12 B per 256 elements) and the
per-job partial sums are left out.  The expectation this is measured against: all are bandwidth-bound, so Adam time and LARS
time <= 7/5 x SGD time x 1.15 (the 15 % for Adam's divide, square root and advance launch; for LARS's two more launch
boundaries and its fp64 adds).

Timing: HIP events around `reps` back-to-back steps after a warm-up of every side, the sides alternating, rounds repeated until
each side has been timed for at least --window seconds; median round reported with the spread.  Needs a GPU.

  python tools/optim_micro.py [--out profiles/optim_micro.json] [--window 0.5]
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
BYTES_PER_ELEM = {'sgd': 20, 'adam': 28, 'adamw': 28, 'lars': 28}
BAR = 7.0 / 5.0 * 1.15


def arena_layout(pkg):
    """-> (offsets, sizes, total, tensors of more than one dimension?) of the R(2+1)D-18 MoCo model's parameter arena"""
    cfg = pkg.get_defaults()
    cfg.merge_from_list(['MODEL.BACKBONE', 'R2P1D18', 'MODEL.BACKBONE_TYPE', '3D', 'MODEL.DROPOUT', 0.0, 'MODEL.PRETRAINED', False,
                         'INPUT.VIDEO_LENGTH', 16, 'CONTRAST.MEM_TYPE', 'moco', 'CROSS.FEAT_DIM', 128])
    model, _ = pkg.lib.modeling.create_visual_model(cfg)
    a = pkg.engine.arena.arena_of(model)
    return a.offsets, a.sizes, a.total, [p.ndim > 1 for p in a.params]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optim_micro.json'))
    ap.add_argument('--window', type=float, default=0.5, help='seconds of timed steps per side, at least')
    ap.add_argument('--reps', type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('optim_micro needs a GPU (a CPU run measures nothing)')
    pkg = importlib.import_module('video-graph-ssl_amd')
    ops, dev = pkg.engine.ops, torch.device('cuda:0')
    offsets, sizes, n, adapt = arena_layout(pkg)
    gen = torch.Generator(device=dev).manual_seed(1)
    grad = torch.randn(n, device=dev, generator=gen).mul_(1e-2)
    p0 = torch.randn(n, device=dev, generator=gen).mul_(0.05)
    clr = torch.full((n // 256,), 1e-3, device=dev)
    cwd = torch.full((n // 256,), 5e-4, device=dev)
    state = {side: dict(p=p0.clone(), a=torch.zeros(n, device=dev)) for side in BYTES_PER_ELEM}
    for side in ('adam', 'adamw'):
        state[side].update(b=torch.zeros(n, device=dev), steps=torch.zeros(1, dtype=torch.int64, device=dev))
    plan = ops.LarsPlan(offsets, sizes, n, dev)         # the model's own tensors: 2-D and up take the trust ratio
    plan.adapt.copy_(torch.tensor([int(x) for x in adapt], dtype=torch.int32))

    def step(side):
        s = state[side]
        if side == 'sgd':
            ops.sgd_step(s['p'], grad, s['a'], clr, cwd, 1.0, 0.9, False)
        elif side == 'lars':
            ops.lars_step(s['p'], grad, s['a'], clr, cwd, plan, 0.9, False, 0.001, 1e-8)
        else:
            ops.adam_step(s['p'], grad, s['a'], s['b'], clr, cwd, 0.9, 0.999, 1e-8, side == 'adamw', s['steps'])

    for side in state:
        for _ in range(10):
            step(side)
    torch.cuda.synchronize()
    times = {side: [] for side in state}
    while min(sum(t) for t in times.values()) * a.reps * 1e-3 < a.window:
        for side in state:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                step(side)
            e1.record()
            e1.synchronize()
            times[side].append(e0.elapsed_time(e1) / a.reps)
    res = {'tool': 'tools/optim_micro.py', 'device': torch.cuda.get_device_name(0), 'arena_elems': n, 'reps': a.reps,
           'rounds': len(times['sgd']),
           'timing': 'HIP events around %d back-to-back steps after warm-up, alternating sides, at least %.2f s per side; '
                     'median round' % (a.reps, a.window), 'sides': {}}
    for side, ts in times.items():
        ms = statistics.median(ts)
        moved = BYTES_PER_ELEM[side] * n
        res['sides'][side] = {'ms_median': round(ms, 4), 'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4),
                              'bytes_moved': moved, 'GBps': round(moved / ms * 1e-6, 1)}
    sgd = res['sides']['sgd']['ms_median']
    res['bar_adam_over_sgd_time'] = round(BAR, 3)
    for side in ('adam', 'adamw', 'lars'):
        r = res['sides'][side]['ms_median'] / sgd
        res['sides'][side]['over_sgd_time'] = round(r, 3)
        res['sides'][side]['within_bar'] = bool(r <= BAR)
    res['lars'] = {'jobs': plan.n_jobs, 'tensors': plan.n_params, 'adapted': int(plan.adapt.sum()),
                   'job_chunks': int(pkg._hip.lib.gca_lars_job_chunks())}
    res['steps_counted'] = {side: int(state[side]['steps']) for side in ('adam', 'adamw')}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
