"""Micro-benchmark of gca_clip_augment at the reference geometry (b = 32, 2 views, T = 16, 128 x 171 -> 112 x 112), next to
gca_clip_prepare on the same output shape (what this stage cost before the augmentations moved to the device).

Three kinds of record: identity (crop + flip only), jitter only (all four colour ops, contrast included, so both launches
run), everything on (resized crop + jitter + blur k = 7; grayscale on every fourth record).  Timing: HIP events around
`reps` back-to-back calls of the C entry (tables already on the device), after a warm-up of every variant; the variants
alternate over `rounds` rounds and the median round is reported with the spread.  Needs a GPU: there is no fallback.

  python tools/augment_micro.py [--out profiles/augment_micro.json] [--reps 50] [--rounds 5]
"""
import argparse
import importlib
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'augment_micro.json'))
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--step-ms', type=float, default=21.0, help='iteration time the stage is compared with')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('augment_micro needs a GPU (a CPU run measures nothing)')
    pkg = importlib.import_module('video-graph-ssl_amd')
    inp, hip = pkg.engine.input, pkg._hip
    dev = torch.device('cuda:0')
    b, views, T, Hs, Ws, H, W = a.batch, 2, 16, 128, 171, 112, 112
    frames = torch.from_numpy(np.random.RandomState(0).randint(0, 256, size=(b, views, T, Hs, Ws, 3)).astype(np.uint8)).to(dev)
    m, d = inp.normalize_constants((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    out = torch.empty((b, 3 * views, T, H, W), dtype=torch.float32, device=dev)
    divtab = torch.from_numpy(inp.hsv_div_tables()).to(dev)
    ws = torch.empty(int(hip.lib.gca_clip_augment_ws_bytes(b, views, T)), dtype=torch.uint8, device=dev)
    rnd, nprnd = random.Random(1), np.random.RandomState(1)

    def records(kind):
        ps = []
        for n in range(b):
            row = []
            for v in range(views):
                p = inp.sample_augment(Hs, Ws, rnd, nprnd)
                if kind == 'identity':
                    p = inp.augment_identity(rnd.randint(0, Hs - H), rnd.randint(0, Ws - W), H, W, rnd.random() < 0.5)
                elif kind == 'jitter_only':
                    q = inp.augment_identity(rnd.randint(0, Hs - H), rnd.randint(0, Ws - W), H, W, rnd.random() < 0.5)
                    q.update(jitter=True, brightness=rnd.uniform(0.6, 1.4), contrast=rnd.uniform(0.6, 1.4),
                             saturation=rnd.uniform(0.6, 1.4), hue=rnd.uniform(-0.1, 0.1), perm=p['perm'])
                    p = q
                else:
                    p.update(jitter=True, brightness=rnd.uniform(0.6, 1.4), contrast=rnd.uniform(0.6, 1.4),
                             saturation=rnd.uniform(0.6, 1.4), hue=rnd.uniform(-0.1, 0.1), k=7, sigma=rnd.uniform(0.1, 2.0),
                             gray=(n * views + v) % 4 == 0)
                row.append(p)
            ps.append(row)
        return ps

    calls = {}
    prm = torch.zeros((b, views, 4), dtype=torch.int32)
    prm[..., 0], prm[..., 1], prm[..., 2] = 8, 29, torch.arange(b * views).view(b, views) % 2
    prm = prm.to(dev)
    calls['clip_prepare'] = lambda: hip.call('gca_clip_prepare', frames.data_ptr(), b, views, T, Hs, Ws, prm.data_ptr(),
                                             m.ctypes.data, d.ctypes.data, H, W, out.data_ptr(), 0, hip.stream())
    keep = []
    for kind in ('identity', 'jitter_only', 'everything_on'):
        rec, taps, luts = inp.pack_augment(records(kind), Hs, Ws, H, W)
        dt = tuple(torch.from_numpy(x).to(dev) for x in (rec, taps, luts))
        keep.append((rec, dt))
        calls['augment_' + kind] = (lambda rec=rec, dt=dt: hip.call(
            'gca_clip_augment', frames.data_ptr(), b, views, T, Hs, Ws, rec.ctypes.data, dt[0].data_ptr(), dt[1].data_ptr(),
            dt[2].data_ptr(), divtab.data_ptr(), m.ctypes.data, d.ctypes.data, H, W, out.data_ptr(), 0, ws.data_ptr(), hip.stream()))
    for fn in calls.values():                      # warm-up: code objects, every variant
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():                # alternate the variants inside a round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.reps)
    clips = b
    res = {'tool': 'tools/augment_micro.py', 'device': torch.cuda.get_device_name(0),
           'geometry': {'b': b, 'views': views, 'T': T, 'src': [Hs, Ws], 'out': [H, W], 'out_dtype': 'float32'},
           'timing': 'HIP events around %d back-to-back entry calls, median of %d alternating rounds' % (a.reps, a.rounds),
           'step_ms_compared_with': a.step_ms, 'variants': {}}
    for k, ts in times.items():
        med = statistics.median(ts)
        res['variants'][k] = {'ms_median': round(med, 4), 'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4),
                              'clips_per_s': round(clips / med * 1e3, 1), 'fraction_of_step': round(med / a.step_ms, 4)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
