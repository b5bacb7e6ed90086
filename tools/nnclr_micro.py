"""Micro-benchmark of the fused NNCLR kernels, same device, same process, same inputs.

Search (ops.nnclr_search: gca_nnclr_search, both views in one pass over the support set, gather included) next to two
comparators, each run once PER VIEW as they must be:
    torch_search      argmax(z @ Q.T) + index_select, fp32 torch ops
    retrieval_topk    ops.retrieval_topk(z, Q, k=1) (the evaluation kernel: norm pass, per-slab lists, merge) + index_select
Backward (ops.nnclr_bwd after ops.mocov3_fwd on the gathered rows) next to torch autograd of the literal loss given the same
neighbours (tests/nnclr_ref.py's torch_chain without its search).

Sizes: N = 64 rows per view, D = 256, K = 65536 and 98304 support rows: unit rows, each z a perturbed copy (cos about 0.9) of a
support row, predictions near the projections, T = 0.1.  Timing: HIP events around `reps` back-to-back calls after a warm-up
of every side, the sides alternating over `rounds` rounds, median round reported with the spread.  The support set (64 / 96 MB)
is larger than the L2 but not than the 256 MB infinity cache, so back-to-back calls may be served from it: the figures are
warm-cache figures for every side alike.  The search's 4 N K D FLOP and the K D 4 bytes it must read are quoted against the
157.3 TF/s fp32-matrix peak and 8 TB/s.  No time here is a bar.  Needs a GPU: there is no fallback.  One process; run it under a
time limit, and start nothing on the device after it if it fails.

  python tools/nnclr_micro.py [--out profiles/nnclr_micro.json] [--rounds 5]
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
SIZES = [(64, 256, 65536, 50), (64, 256, 98304, 50)]        # N, D, K, reps
TEMPERATURE = 0.1
PEAK_TFLOPS, PEAK_TBS = 157.3, 8.0


def inputs(N, D, K, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    Q = F.normalize(torch.randn(K, D, device=dev, generator=gen))
    zs, ps = [], []
    for _ in range(2):
        des = torch.randint(0, K, (N,), device=dev, generator=gen)
        z = F.normalize(Q[des] + torch.randn(N, D, device=dev, generator=gen) * (0.23 / D) ** 0.5)
        zs.append(z)
        ps.append(F.normalize(z + torch.randn(N, D, device=dev, generator=gen) * (0.3 / D) ** 0.5))
    return zs[0], zs[1], ps[0], ps[1], Q


def get_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nnclr_micro.json'))
    ap.add_argument('--rounds', type=int, default=5)
    return ap


def main(argv=None):
    a = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('nnclr_micro needs a GPU (a CPU run measures nothing)')
    pkg = importlib.import_module('video-graph-ssl_amd')
    ops, lib, dev = pkg.engine.ops, pkg._hip.lib, torch.device('cuda:0')
    inv_T = 1.0 / TEMPERATURE
    res = {'tool': 'tools/nnclr_micro.py', 'device': torch.cuda.get_device_name(0), 'temperature': TEMPERATURE,
           'peak_tflops_fp32_matrix': PEAK_TFLOPS, 'peak_tb_per_s': PEAK_TBS, 'sizes': {},
           'timing': 'HIP events around back-to-back calls after warm-up, median of %d alternating rounds' % a.rounds}
    for N, D, K, reps in SIZES:
        z1, z2, p1, p2, Q = inputs(N, D, K, dev)
        pg1, pg2 = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
        ops.WS.get(max(int(lib.gca_nnclr_search_ws_bytes(N, D, K)), int(lib.gca_nnclr_bwd_ws_bytes(N, D)),
                       int(lib.gca_mocov3_ws_bytes(N, D)), int(lib.gca_retrieval_ws_bytes(N, K, D, 1, 0))), dev)
        waves, splits = C.c_int32(-1), C.c_int32(-1)
        path = lib.gca_nnclr_search_path(N, D, K, 1, C.addressof(waves), C.addressof(splits))
        idx0, _, nn1, nn2 = ops.nnclr_search(z1, z2, Q)
        _, lse0, _, _ = ops.mocov3_fwd(nn1, nn2, p1, p2, inv_T, w=ops.nnclr_weight())
        target = torch.arange(N, device=dev)

        def torch_search():
            i1, i2 = (z1 @ Q.t()).argmax(dim=1), (z2 @ Q.t()).argmax(dim=1)
            return i1, i2, Q.index_select(0, i1), Q.index_select(0, i2)

        def topk_search():
            i1, i2 = ops.retrieval_topk(z1, Q, 1)[0][:, 0].long(), ops.retrieval_topk(z2, Q, 1)[0][:, 0].long()
            return i1, i2, Q.index_select(0, i1), Q.index_select(0, i2)

        def chain_bwd():
            pg1.grad = pg2.grad = None
            loss = 0.5 * (F.cross_entropy(nn1 @ pg2.t() / TEMPERATURE, target) + F.cross_entropy(nn2 @ pg1.t() / TEMPERATURE, target))
            loss.backward()
            return pg1.grad, pg2.grad

        def fused_loss_bwd():
            _, lse, _, _ = ops.mocov3_fwd(nn1, nn2, p1, p2, inv_T, w=ops.nnclr_weight(), want_rank=True)
            return ops.nnclr_bwd(nn1, nn2, p1, p2, lse, inv_T)

        calls = {'fused_search': lambda: ops.nnclr_search(z1, z2, Q), 'torch_search': torch_search, 'retrieval_topk': topk_search,
                 'fused_bwd': lambda: ops.nnclr_bwd(nn1, nn2, p1, p2, lse0, inv_T), 'fused_loss_bwd': fused_loss_bwd,
                 'torch_chain_loss_bwd': chain_bwd}
        for fn in calls.values():                            # warm-up: code objects, the caching allocator's blocks
            fn()
            fn()
        torch.cuda.synchronize()
        t1, t2 = torch_search()[:2], topk_search()[:2]
        gf, gc = fused_loss_bwd(), chain_bwd()
        agree = {'idx_equal_torch': bool(torch.equal(idx0[0].long(), t1[0]) and torch.equal(idx0[1].long(), t1[1])),
                 'idx_equal_retrieval_topk': bool(torch.equal(idx0[0].long(), t2[0]) and torch.equal(idx0[1].long(), t2[1])),
                 'dp_rel_diff': max(float((a_ - b_).abs().max() / b_.abs().max()) for a_, b_ in zip(gf, gc))}
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
        entry = {'N': N, 'D': D, 'K': K, 'reps': reps, 'search_path': ('generic', 'fast')[path], 'waves': waves.value,
                 'splits': splits.value, 'agreement': agree}
        for side, ts in times.items():
            med = statistics.median(ts)
            entry[side] = {'ms_median': round(med, 5), 'ms_min': round(min(ts), 5), 'ms_max': round(max(ts), 5)}
        ms = entry['fused_search']['ms_median']
        tf, tbs = 4.0 * N * K * D / ms * 1e-9, 4.0 * K * D / ms * 1e-9
        entry['fused_search'].update(tflops=round(tf, 2), fraction_of_peak=round(tf / PEAK_TFLOPS, 4), tb_per_s=round(tbs, 3),
                                     fraction_of_bandwidth=round(tbs / PEAK_TBS, 4))
        entry['torch_search_over_fused_time'] = round(entry['torch_search']['ms_median'] / ms, 3)
        entry['retrieval_topk_over_fused_time'] = round(entry['retrieval_topk']['ms_median'] / ms, 3)
        entry['chain_over_fused_loss_bwd_time'] = round(entry['torch_chain_loss_bwd']['ms_median'] / entry['fused_loss_bwd']['ms_median'], 3)
        res['sizes']['%dx%dx%d' % (N, D, K)] = entry
        print(json.dumps({'%dx%dx%d' % (N, D, K): entry}), flush=True)
        del z1, z2, p1, p2, Q, pg1, pg2, nn1, nn2
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
