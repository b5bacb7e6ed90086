"""Micro-benchmark of the fused ReSSL kernels, same device, same process, same inputs.

    fused_ressl     ops.ressl_fwd + ops.ressl_bwd: two passes over the queue, nothing of size K written
    torch_chain     the literal loss as fp32 torch ops with autograd: -(softmax(k Q^T / Tt) * log_softmax(q Q^T / Ts)).sum(1).mean()
                    and its backward to q
    moco_pair       ops.moco_logits_fwd (logits, log-sum-exps and the InfoNCE loss) + ops.moco_logits_bwd at the same shape:
                    MoCo's own fused pair, the yardstick for "a pass over the same queue" (it writes the (N, K + 1) logits)

Sizes: N = 64 rows, D = 128, K = 65536 and 98304 queue rows: unit rows, k a perturbed copy of q, Ts = 0.1, Tt = 0.04.  Timing: HIP
events around `reps` back-to-back calls after a warm-up of every side, the sides alternating over `rounds` rounds, median round
reported with the spread.  The queue (32 / 48 MB) is larger than the L2 but not than the 256 MB infinity cache, so back-to-back
calls may be served from it: the figures are warm-cache figures for every side alike.  The 2 K D 4 bytes the fused pair must
read are quoted against 8 TB/s, its 12 N K D FLOP (two score tiles in each pass, two P Q products in the second) against the
157.3 TF/s fp32-matrix peak.  No time here is a bar.  Needs a GPU: there is no fallback.  One process; run it under a time limit,
and start nothing on the device after it if it fails.

  python tools/ressl_micro.py [--out profiles/ressl_micro.json] [--rounds 5]
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
SIZES = [(64, 128, 65536, 50), (64, 128, 98304, 50)]        # N, D, K, reps
TS, TT = 0.1, 0.04
PEAK_TFLOPS, PEAK_TBS = 157.3, 8.0


def inputs(N, D, K, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    Q = F.normalize(torch.randn(K, D, device=dev, generator=gen))
    q = F.normalize(torch.randn(N, D, device=dev, generator=gen))
    k = F.normalize(q + torch.randn(N, D, device=dev, generator=gen) * (0.3 / D) ** 0.5)
    return q, k, Q


def get_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ressl_micro.json'))
    ap.add_argument('--rounds', type=int, default=5)
    return ap


def main(argv=None):
    a = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('ressl_micro needs a GPU (a CPU run measures nothing)')
    pkg = importlib.import_module('video-graph-ssl_amd')
    ops, lib, dev = pkg.engine.ops, pkg._hip.lib, torch.device('cuda:0')
    inv_Ts, inv_Tt = 1.0 / TS, 1.0 / TT
    res = {'tool': 'tools/ressl_micro.py', 'device': torch.cuda.get_device_name(0), 'Ts': TS, 'Tt': TT,
           'peak_tflops_fp32_matrix': PEAK_TFLOPS, 'peak_tb_per_s': PEAK_TBS, 'sizes': {},
           'timing': 'HIP events around back-to-back calls after warm-up, median of %d alternating rounds' % a.rounds}
    for N, D, K, reps in SIZES:
        q, k, Q = inputs(N, D, K, dev)
        qg = q.clone().requires_grad_(True)
        ops.WS.get(max(int(lib.gca_ressl_fwd_ws_bytes(N, D, K)), int(lib.gca_ressl_bwd_ws_bytes(N, D, K)),
                       int(lib.gca_infonce_ws_bytes(N, K))), dev)
        paths = {}
        for which in ('fwd', 'bwd'):
            waves, splits = C.c_int32(-1), C.c_int32(-1)
            rc = getattr(lib, 'gca_ressl_%s_path' % which)(N, D, K, 1, C.addressof(waves), C.addressof(splits))
            paths[which] = {'path': ('generic', 'fast')[rc], 'waves': waves.value, 'splits': splits.value}
        logits = torch.empty((N, K + 1), dtype=torch.float32, device=dev)
        _, lse0, _ = ops.ressl_fwd(q, k, Q, inv_Ts, inv_Tt)

        def fused():
            loss, row_lse, _ = ops.ressl_fwd(q, k, Q, inv_Ts, inv_Tt)
            return loss, ops.ressl_bwd(q, k, Q, row_lse, inv_Ts, inv_Tt)

        def chain():
            qg.grad = None
            loss = -(torch.softmax(k @ Q.t() / TT, dim=1) * torch.log_softmax(qg @ Q.t() / TS, dim=1)).sum(dim=1).mean()
            loss.backward()
            return loss.detach(), qg.grad

        def moco_pair():
            lg, lse, _, loss = ops.moco_logits_fwd(q, k, Q, inv_Ts, want_lse=True, want_loss=True, logits=logits)
            return loss, ops.moco_logits_bwd(k, Q, inv_Ts, logits=lg, lse=lse)

        calls = {'fused_ressl': fused, 'fused_fwd': lambda: ops.ressl_fwd(q, k, Q, inv_Ts, inv_Tt),
                 'fused_bwd': lambda: ops.ressl_bwd(q, k, Q, lse0, inv_Ts, inv_Tt), 'torch_chain': chain, 'moco_pair': moco_pair}
        for fn in calls.values():                            # warm-up: code objects, the caching allocator's blocks
            fn()
            fn()
        torch.cuda.synchronize()
        (lf, gf), (lc, gc) = fused(), chain()
        agree = {'loss_abs_diff': abs(float(lf[0]) - float(lc)), 'dq_rel_diff': float((gf - gc).abs().max() / gc.abs().max())}
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
        entry = {'N': N, 'D': D, 'K': K, 'reps': reps, 'paths': paths, 'agreement': agree}
        for side, ts in times.items():
            med = statistics.median(ts)
            entry[side] = {'ms_median': round(med, 5), 'ms_min': round(min(ts), 5), 'ms_max': round(max(ts), 5)}
        ms = entry['fused_ressl']['ms_median']
        tf, tbs = 12.0 * N * K * D / ms * 1e-9, 2 * 4.0 * K * D / ms * 1e-9
        entry['fused_ressl'].update(tflops=round(tf, 2), fraction_of_peak=round(tf / PEAK_TFLOPS, 4), tb_per_s=round(tbs, 3),
                                    fraction_of_bandwidth=round(tbs / PEAK_TBS, 4))
        entry['chain_over_fused_time'] = round(entry['torch_chain']['ms_median'] / ms, 3)
        entry['moco_pair_over_fused_time'] = round(entry['moco_pair']['ms_median'] / ms, 3)
        res['sizes']['%dx%dx%d' % (N, D, K)] = entry
        print(json.dumps({'%dx%dx%d' % (N, D, K): entry}), flush=True)
        del q, k, Q, qg, logits
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
