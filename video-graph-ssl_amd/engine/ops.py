"""Tensor-level wrappers over the C ABI (one function per kernel family), and the per-geometry conv plans.

torch is used for device memory and the current HIP stream only; every arithmetic
operation below runs in libgca_hip.so.  Geometry-dependent host data (gather tables,
workspace sizes, the pinned launch configuration) is cached per geometry in a ConvPlan.  A plan measures its launch
configuration once (ConvPlan.tune -> ConvPlan.search); the launch codes and the candidate lists it measures are host
arithmetic in engine/tune.py.
"""
import ctypes as C
import functools
import os

import torch

from .. import _hip as H
from .._hip import aptr, is_half, ptr, stream
from . import tune
from .tune import TUNE_HALO, TUNE_PW, TUNE_STEM, TUNE_VEC      # (flags of a forward / dgrad launch code; tests and tools force them)

F32 = torch.float32
F16 = torch.float16


def _t3(v):
    return (v, v, v) if isinstance(v, int) else tuple(int(a) for a in v)


# ----------------------------------------------------------------------------- workspace
class _Workspace:
    """One grow-only scratch buffer per device.  All kernels run stream-ordered on the current
    stream, so consecutive users never overlap in time.

    A captured hipGraph holds the RAW pointer of the buffer it was recorded with.  A buffer that was handed out
    during a capture is therefore never freed when a later (eager) caller needs more bytes: it is retired -- kept
    alive next to the new, larger one -- so every existing graph keeps replaying into memory it still owns.
    Growth is geometric, so the retired buffers sum to less than the live one."""

    def __init__(self):
        self.buf = {}
        self.captured = set()       # keys whose current buffer has been baked into a graph
        self.retired = []

    def get(self, nbytes, device):
        key = (device.type, device.index, WS_LANE[0])
        b = self.buf.get(key)
        capturing = torch.cuda.is_current_stream_capturing()
        if b is None or b.numel() < nbytes:
            if capturing:
                raise RuntimeError('workspace would grow during graph capture; run one eager step first')
            if b is not None and key in self.captured:
                self.retired.append(b)
                self.captured.discard(key)
            grown = 0 if b is None else b.numel() + b.numel() // 2
            b = torch.empty(max(int(nbytes), grown, 1 << 20), dtype=torch.uint8, device=device)
            self.buf[key] = b
        if capturing:
            self.captured.add(key)
        return b


# Scratch lane: work issued on a second stream next to the main one (the key encoder's forward inside the captured
# single-GPU step, engine/trainer.py) takes its scratch from its own buffer -- lanes never share split-K slabs.
WS_LANE = [0]
WS = _Workspace()


# ----------------------------------------------------------------------------- convolution
AUTOTUNE = os.environ.get('GCA_AUTOTUNE', '1') != '0'

# Measured launch configurations, keyed by (pass, geometry).  GCA_TUNE_CACHE=<file> persists them across runs
# (loaded at import, written at exit by rank 0): a restarted job, or a profiler pass that must see the same
# kernels as the run it explains, skips the measurement.
_TUNE_CACHE = {}
_TUNE_DIRTY = [False]
_TUNE_PATH = os.environ.get('GCA_TUNE_CACHE', '')


CONV_MATH = {'f32': 0, 'bf16x3': 1, 'bf16x6': 2}
ACT_F16 = [False]


def set_conv_math(mode):
    """Arithmetic of the conv kernels: 'f32' (fp32 MFMA), 'bf16x6' (fp32-grade split products) or 'bf16x3' (faster); see
    gca_set_conv_math in include/gca_hip.h.  Plans tuned under one mode re-tune under the other (cache keys differ),
    but a plan object keeps the configuration it was tuned with: set the mode before building the model.

    'fp16' is the fp16-STORAGE path (BASELINE configs[4]): every feature map between the input clip and the pooled
    features, and its gradient, lives in HBM as IEEE fp16; the convs run v_mfma_f32_32x32x16_f16 with fp32 accumulation;
    BatchNorm statistics, parameters (fp32 masters), their gradients, the head and the loss stay fp32."""
    ACT_F16[0] = mode == 'fp16'
    H.call('gca_set_conv_math', CONV_MATH['bf16x6' if mode == 'fp16' else mode])


def get_conv_math():
    return 'fp16' if ACT_F16[0] else ('f32', 'bf16x3', 'bf16x6')[H.lib.gca_get_conv_math()]


def cast_f16(x):
    """fp32 -> dense fp16 copy (the input clips of the fp16-storage path); x may be a channel slice of a wider batch."""
    rows, re = (1, x.numel()) if x.is_contiguous() else (x.shape[0], x[0].numel())
    if not x.is_contiguous() and not x[0].is_contiguous():
        raise RuntimeError('only channel slices of a contiguous (N, Ctot, ...) buffer are supported')
    y = torch.empty(x.shape, dtype=F16, device=x.device)
    H.call('gca_cast_f16', ptr(x), rows, re, re if x.is_contiguous() else x.stride(0), aptr(y), stream())
    return y


def load_tune_cache(path):
    import json
    with open(path) as f:
        for k, v in json.load(f).items():
            _TUNE_CACHE[k] = tuple(v)


def save_tune_cache(path):
    import json
    tmp = '%s.tmp.%d' % (path, os.getpid())
    with open(tmp, 'w') as f:
        json.dump({k: list(v) for k, v in sorted(_TUNE_CACHE.items())}, f, indent=0)
    os.replace(tmp, path)


if _TUNE_PATH:
    import atexit
    if os.path.exists(_TUNE_PATH):
        load_tune_cache(_TUNE_PATH)
    atexit.register(lambda: _TUNE_DIRTY[0] and os.environ.get('RANK', '0') == '0' and save_tune_cache(_TUNE_PATH))


def _time_ms(fn, reps=3):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


# Kernel families of the forward / dgrad pass: (name, flag of a launch code's bm that asks for it, bit of gca_conv_kernel_cfg's
# last word that reports it); neither set = the gather kernels
_KERNELS = (('halo', TUNE_HALO, 14), ('stem', TUNE_STEM, 16), ('pw', TUNE_PW, 17))


def _tune_kernel(code):
    """Kernel family a tune code asks for (as named by ConvPlan.kernel)."""
    return next((name for name, flag, _ in _KERNELS if code & flag), 'gather')


class ConvPlan:
    """Everything geometry-dependent about one conv: the ABI struct, device gather tables, and the launch
    configuration pinned by a one-off measurement (the role cudnn.benchmark plays in the reference)."""

    def __init__(self, N, Cin, D, Hh, W, K, k, s, p, device, x_batch_stride=0, act_f16=False):
        kd, kh, kw = _t3(k)
        sd, sh, sw = _t3(s)
        pd, ph, pw = _t3(p)
        OD, OH, OW = (D + 2 * pd - kd) // sd + 1, (Hh + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
        self.g = H.ConvGeom(N, Cin, D, Hh, W, K, kd, kh, kw, sd, sh, sw, pd, ph, pw, OD, OH, OW, x_batch_stride)
        self.g.act_f16 = int(bool(act_f16))
        self.act_dtype = F16 if act_f16 else F32
        self.gp = C.byref(self.g)
        self.in_shape = (N, Cin, D, Hh, W)
        self.out_shape = (N, K, OD, OH, OW)
        self.device = device
        self.taps = kd * kh * kw
        self._tables = {}
        self.tuned = [not AUTOTUNE] * 3
        if H.lib.gca_conv_fwd_stat_parts(self.gp) < 0:
            raise ValueError('unsupported conv geometry %r' % ((N, Cin, D, Hh, W, K, k, s, p),))
        self.pack_elems = [H.lib.gca_conv_pack_elems(self.gp, 0), H.lib.gca_conv_pack_elems(self.gp, 1)]
        self.refresh()

    def refresh(self):
        """Sizes that depend on the launch configuration."""
        self.parts = H.lib.gca_conv_fwd_stat_parts(self.gp)
        self.wgrad_ws = H.lib.gca_conv_wgrad_ws_bytes(self.gp)
        self.fwd_ws = H.lib.gca_conv_fwd_ws_bytes(self.gp)
        self.dgrad_ws = H.lib.gca_conv_dgrad_ws_bytes(self.gp) if self.g.x_batch_stride == 0 else 0
        # a strided dgrad runs its residue classes in one launch when their split-K slabs fit side by side (the sum over
        # classes; dgrad_ws is the maximum)
        self.dgrad_ws_merged = H.lib.gca_conv_dgrad_ws_bytes_merged(self.gp) if self.g.x_batch_stride == 0 else 0

    def table(self, which):
        t = self._tables.get(which)
        if t is None:
            rows = H.lib.gca_conv_table_rows(self.gp, which)
            host = torch.empty(rows * 2, dtype=torch.int32)
            H.call('gca_conv_table_build_host', self.gp, which, host.data_ptr())
            t = host.to(self.device)
            self._tables[which] = t
        return t

    def cfg(self, which):
        out = (C.c_int32 * 4)()
        if which == 2:
            H.call('gca_conv_wgrad_cfg', self.gp, out)
        else:
            H.call('gca_conv_kernel_cfg', self.gp, which, out)
        return tuple(out)

    # shape field (low byte of gca_conv_wgrad_cfg's last word) of the streaming wgrad kernels; 1..10 = the gather kernel's shapes
    WGRAD_KERNELS = {11: 'temporal32', 12: 'temporal64', 13: 'spatial', 14: 'stem'}
    WGRAD_SHAPES = tune.WGRAD_SHAPES

    def kernel(self, which):
        """Kernel family the forward (0) / dgrad (1) pass runs on under the configuration in force: 'gather', 'halo',
        'stem' or 'pw'; for the weight gradient (2): 'gather', 'temporal32', 'temporal64', 'spatial' or 'stem'."""
        kc = self.cfg(which)[3]
        if which == 2:
            return self.WGRAD_KERNELS.get(kc & 255, 'gather')
        return next((name for name, _, bit in _KERNELS if kc >> bit & 1), 'gather')

    def math(self, which):
        """Arithmetic the pass runs with (bits 12-13 of the configuration's last word): 0 f32, 1 bf16x3, 2 bf16x6, 3 fp16."""
        return self.cfg(which)[3] >> 12 & 3

    def pack_layout(self, which):
        """Packed-weight layout the pass reads under the configuration in force: 0 = k-major fp32 rows (gather kernels; the weight
        gradient reads none), else the LDS-halo layout, which also depends on the arithmetic (fp32 rows / 2 / 3 bf16 parts)."""
        return 0 if which == 2 else H.lib.gca_conv_pack_layout(self.gp, which)

    # ---- one-off launch tuning ------------------------------------------------------------
    def tune_key(self, which):
        """Tune-cache key of pass `which`: library version, arithmetic ('' f32, 'b' bf16x3, 'c' bf16x6, 'h' fp16 storage), pass, geometry."""
        g = self.g
        geom = (g.N, g.C, g.D, g.H, g.W, g.K, g.kd, g.kh, g.kw, g.sd, g.sh, g.sw, g.pd, g.ph, g.pw, g.x_batch_stride)
        return 'v%d%s:%d:%s' % (H.lib.gca_version(), 'h' if g.act_f16 else ('', 'b', 'c')[H.lib.gca_get_conv_math()], which,
                                ','.join(str(int(v)) for v in geom))

    def set_code(self, which, code):
        """Pin launch code `code` (tune.ConvCode / tune.WgradCode) for pass `which`."""
        for field, v in zip(code._fields, code):
            setattr(self.g, 'tune_%s_%s' % (tune.PASSES[which], field), v)
        self.refresh()

    def tune(self, which, run, repack=None):
        """Measure the candidate launch configurations of pass `which` (0 fwd, 1 dgrad, 2 wgrad) with `run`
        (a closure launching that pass on real operands) and pin the fastest.  `repack()` re-lays the packed weights
        out for the configuration in force (the LDS-halo kernels read another layout than the gather kernels);
        without it only configurations of the current layout are measured."""
        if self.tuned[which] or torch.cuda.is_current_stream_capturing():
            return

        def measure():
            try:
                return _time_ms(run)
            except RuntimeError:
                return None
        self.search(which, measure, repack)

    def _adopt(self, which, code, repack):
        """Pin the launch code of a tune-cache hit, if the packed weights at hand allow it; -> what happened."""
        layout = self.pack_layout(which)
        self.set_code(which, code)
        if H.lib.gca_conv_fwd_stat_parts(self.gp) < 0:
            return 'stale'                                     # not a valid launch code for this library (any more)
        if self.pack_layout(which) == layout:
            return 'as is'
        if repack is not None:
            repack()
            return 'repacked'
        # The measured configuration reads another packed layout and this caller cannot re-pack (no raw weights: the plain
        # HipConv3d.forward path).  It runs on the heuristic shape of the layout at hand, and BOTH the cache entry and the
        # plan's "untuned" state are left alone: the next caller that can re-pack adopts the entry.
        return 'cannot repack'

    def search(self, which, measure, repack=None):
        """tune() behind its device: `measure()` times the pass under the configuration in force (None = cannot run)."""
        self.tuned[which] = True
        key, heuristic = self.tune_key(which), tune.CODES[which]()
        packed_as = self.pack_layout(which)
        hit = _TUNE_CACHE.get(key)
        if hit is not None:
            adopted = self._adopt(which, tune.CODES[which](*hit), repack)
            if adopted in ('stale', 'cannot repack'):
                self.set_code(which, heuristic)
            self.tuned[which] = adopted != 'cannot repack'
            if adopted != 'stale':
                return
        g, math = self.g, H.lib.gca_get_conv_math()
        timed = []
        for round_ in (1, 2):               # every candidate, then two-phase forms of the two fastest
            codes = tune.candidates(which, g, math) if round_ == 1 else [c for _, base in sorted(timed)[:2]
                                                                          for c in tune.two_phase(which, g, base)]
            for code in codes:
                self.set_code(which, code)
                # where the library cannot run what a code asks for (tile shape not built for this tap count, halo / stem
                # kernel not runnable here) it falls back to another kernel: nothing new to measure
                asked = self.cfg(2)[3] & 255 == code.tile if which == 2 else self.kernel(which) == _tune_kernel(code.bm)
                if not asked:
                    continue
                if self.pack_layout(which) != packed_as:
                    if repack is None:
                        continue
                    repack()
                    packed_as = self.pack_layout(which)
                t = measure()
                if t is not None:
                    timed.append((t, code))
        if timed:
            _TUNE_CACHE[key] = tuple(min(timed)[1])
            _TUNE_DIRTY[0] = True
        self.set_code(which, min(timed)[1] if timed else heuristic)
        if repack is not None and self.pack_layout(which) != packed_as:
            repack()


@functools.lru_cache(maxsize=None)
def _conv_plan(N, Cin, D, Hh, W, K, k, s, p, dev_type, dev_index, xbs, math):
    return ConvPlan(N, Cin, D, Hh, W, K, k, s, p, torch.device(dev_type, dev_index), xbs, act_f16=math == 3)


def conv_plan(x_shape, K, k, s, p, device, x_batch_stride=0, act_f16=False):
    N, Cin, D, Hh, W = x_shape
    # one plan (= one set of tuned launch configurations) per geometry AND arithmetic mode (3 = fp16 storage)
    return _conv_plan(N, Cin, D, Hh, W, K, _t3(k), _t3(s), _t3(p), device.type, device.index, int(x_batch_stride),
                      3 if act_f16 else H.lib.gca_get_conv_math())


def conv_pack(plan, which, w, out=None):
    n = plan.pack_elems[which]
    if out is None or out.numel() != n:
        out = torch.zeros(n, dtype=F32, device=w.device)      # (room for either layout of the class; the unused part stays 0)
    H.call('gca_conv_pack', plan.gp, which, ptr(w), ptr(out), stream())
    return out


def _act(plan, t):
    """Pointer of an activation operand of a conv, checked against the storage type the plan was built for."""
    if t.dtype is not plan.act_dtype:
        raise TypeError('conv plan built for %s activations, got %s' % (plan.act_dtype, t.dtype))
    return aptr(t)


def _conv_fwd_launch(plan, x, wpack, bias, y, ss, sq):
    ws = WS.get(plan.fwd_ws, x.device) if plan.fwd_ws else None
    H.call('gca_conv_fwd', plan.gp, _act(plan, x), ptr(wpack), ptr(plan.table(0)), ptr(bias), _act(plan, y), ptr(ss), ptr(sq),
           ptr(ws), stream())


def _repacker(plan, which, w_raw, wpack):
    if w_raw is None:
        return None
    return lambda: H.call('gca_conv_pack', plan.gp, which, ptr(w_raw), ptr(wpack), stream())


def _stat_pair(plan, device):
    """Uninitialised (sum, sum of squares) BatchNorm partials of a forward under the launch shape in force: [K][plan.parts] each."""
    return tuple(torch.empty((plan.g.K, plan.parts), dtype=F32, device=device) for _ in range(2))


def conv_fwd(plan, x, wpack, bias=None, stats=False, w_raw=None):
    """-> y [, (stat_sum, stat_sq)]  with stat layout [K][plan.parts].  w_raw: the unpacked weights behind `wpack`; lets
    the one-off launch tuning try configurations that read another packed layout (it re-packs into `wpack`)."""
    y = torch.empty(plan.out_shape, dtype=plan.act_dtype, device=x.device)
    if not plan.tuned[0]:
        plan.tune(0, lambda: _conv_fwd_launch(plan, x, wpack, bias, y, None, None), _repacker(plan, 0, w_raw, wpack))
    ss, sq = _stat_pair(plan, x.device) if stats else (None, None)
    _conv_fwd_launch(plan, x, wpack, bias, y, ss, sq)
    return (y, (ss, sq)) if stats else y


def conv_xf_ok(plan):
    """True when, under the launch shapes pinned in `plan`, the conv can consume relu(y*scale+shift) of its PRODUCER on the
    fly (forward on an LDS-halo kernel, weight gradient on a streaming kernel): gca_conv_xf_ok."""
    return plan.tuned[0] and plan.tuned[2] and plan.g.x_batch_stride == 0 and bool(H.lib.gca_conv_xf_ok(plan.gp))


def conv_fwd_xf(plan, y_in, scale, shift, wpack, stats=False):
    """conv_fwd on z = relu(y_in * scale[c] + shift[c]) without materialising z (scale / shift: padded rows of bn_finalize)."""
    y = torch.empty(plan.out_shape, dtype=F32, device=y_in.device)
    ss, sq = _stat_pair(plan, y_in.device) if stats else (None, None)
    ws = WS.get(plan.fwd_ws, y_in.device) if plan.fwd_ws else None
    H.call('gca_conv_fwd_xf', plan.gp, ptr(y_in), ptr(scale), ptr(shift), ptr(wpack), ptr(plan.table(0)), None, ptr(y), ptr(ss),
           ptr(sq), ptr(ws), stream())
    return (y, (ss, sq)) if stats else y


def set_dgrad_merge(on):
    """Strided dgrads as one launch over all stride-residue classes (default; GCA_DGRAD_MERGE=0 in the environment turns it
    off) or one launch per class.  Same bits either way (A/B runs, tests).  -> the previous setting."""
    return bool(H.lib.gca_set_dgrad_merge(int(bool(on))))


def _conv_dgrad_launch(plan, dy, wpack_t, dx, accumulate, ws_bytes=None):
    """ws_bytes: scratch handed to the library (default: room for the merged launch of a strided dgrad; with only
    plan.dgrad_ws the library launches the classes one after another)."""
    need = max(plan.dgrad_ws, plan.dgrad_ws_merged) if ws_bytes is None else ws_bytes
    ws = WS.get(need, dy.device) if need else None
    H.call('gca_conv_dgrad_ws', plan.gp, _act(plan, dy), ptr(wpack_t), ptr(plan.table(1)), _act(plan, dx), int(accumulate), ptr(ws),
           need, stream())


def conv_dgrad(plan, dy, wpack_t, dx=None, accumulate=False, w_raw=None):
    if dx is None:
        dx = torch.empty(plan.in_shape, dtype=plan.act_dtype, device=dy.device)
        accumulate = False
    if not plan.tuned[1]:
        scratch = torch.empty(plan.in_shape, dtype=plan.act_dtype, device=dy.device)
        plan.tune(1, lambda: _conv_dgrad_launch(plan, dy, wpack_t, scratch, False), _repacker(plan, 1, w_raw, wpack_t))
    _conv_dgrad_launch(plan, dy, wpack_t, dx, accumulate)
    return dx


def _conv_wgrad_launch(plan, x, dy, dw, accumulate):
    ws = WS.get(plan.wgrad_ws, x.device)
    H.call('gca_conv_wgrad', plan.gp, _act(plan, x), _act(plan, dy), ptr(plan.table(2)), ptr(dw), int(accumulate), ptr(ws), stream())


class DeferredReduce(object):
    """Collects the split-K reductions of the weight gradients of one backward pass (stage) and runs them as ONE launch
    (gca_splitk_reduce_batched) instead of one 8-12 us launch per layer.  Each (gradient tensor, plan) pair owns a
    persistent slab buffer (the partial sums must survive until the flush); the job table of a given set of layers is
    built and uploaded once -- during the eager warm-up steps -- and replayed from then on, hipGraph capture included.
    Results are bit-identical to the per-layer reductions (same fold order)."""

    def __init__(self):
        self.slabs = {}          # (dw data_ptr, plan id) -> uint8 slab buffer
        self.tables = {}         # tuple of job signatures -> (device table, njobs, blocks)
        self.pending = []        # [(slab, dw, n, splits, accumulate)]
        self.launches = 0

    def slab_for(self, dw, plan):
        key = (dw.data_ptr(), id(plan))
        b = self.slabs.get(key)
        if b is None or b.numel() < plan.wgrad_ws:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('weight-gradient slab would be allocated during graph capture; run one eager step first')
            b = self.slabs[key] = torch.empty(max(int(plan.wgrad_ws), 16), dtype=torch.uint8, device=dw.device)
        return b

    def add(self, plan, x, dy, dw, accumulate, xf=None, dzf=None):
        """dzf = (y, consts, relu): `dy` is dz, the gradient behind the conv's own BatchNorm (conv_wgrad_dzf)."""
        if any(j[1].data_ptr() == dw.data_ptr() for j in self.pending):
            self.flush()                                   # a weight used twice (SimSiam's two views): keep the += order, no race
        slab = self.slab_for(dw, plan)
        splits = C.c_int32(0)
        if dzf is not None:
            H.call('gca_conv_wgrad_dzf_partial', plan.gp, _act(plan, x), _act(plan, dy), _act(plan, dzf[0]), ptr(dzf[1]),
                   int(dzf[2]), ptr(plan.table(2)), slab.data_ptr(), C.addressof(splits), stream())
        else:
            H.call('gca_conv_wgrad_partial', plan.gp, _act(plan, x), ptr(xf[0]) if xf else None, ptr(xf[1]) if xf else None,
                   _act(plan, dy), ptr(plan.table(2)), slab.data_ptr(), C.addressof(splits), stream())
        self.pending.append((slab, dw, dw.numel(), int(splits.value), int(bool(accumulate))))

    def flush(self):
        if not self.pending:
            return
        jobs, self.pending = self.pending, []
        sig = tuple((j[0].data_ptr(), j[1].data_ptr(), j[2], j[3], j[4]) for j in jobs)
        t = self.tables.get(sig)
        if t is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('reduce-job table would be built during graph capture; run one eager step first')
            arr = (H.ReduceJob * len(jobs))()
            for r, (slab, dw, n, splits, acc) in zip(arr, jobs):
                r.slabs, r.dw, r.n, r.splits, r.accumulate = slab.data_ptr(), dw.data_ptr(), n, splits, acc
            blocks = H.lib.gca_reduce_jobs_finalize_host(C.addressof(arr), len(jobs))
            if blocks <= 0:
                raise RuntimeError('gca_reduce_jobs_finalize_host: %d' % blocks)
            dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(jobs[0][1].device)
            t = self.tables[sig] = (dev, len(jobs), int(blocks))
        H.call('gca_splitk_reduce_batched', t[0].data_ptr(), t[1], t[2], stream())
        self.launches += 1


# The collector of the backward pass that is running (set by the trainers around Tape.backward), or None: every
# conv_wgrad then reduces its own slabs at once.
DEFER = [None]


def conv_wgrad(plan, x, dy, dw, accumulate=True, xf=None):
    """xf = (scale, shift): `x` is the producer's PRE-activation tensor, the gradient is taken against
    relu(x * scale[c] + shift[c]) (gca_conv_wgrad_xf; only where conv_xf_ok(plan))."""
    if not plan.tuned[2]:
        if xf is not None:
            raise RuntimeError('conv_wgrad(xf=...) needs a tuned plan (conv_xf_ok)')
        scratch = torch.empty_like(dw)
        plan.tune(2, lambda: _conv_wgrad_launch(plan, x, dy, scratch, False))
    d = DEFER[0]
    if d is not None and dw.is_contiguous():
        d.add(plan, x, dy, dw, accumulate, xf)
        return dw
    if xf is not None:
        ws = WS.get(plan.wgrad_ws, x.device)
        H.call('gca_conv_wgrad_xf', plan.gp, _act(plan, x), ptr(xf[0]), ptr(xf[1]), _act(plan, dy), ptr(plan.table(2)), ptr(dw),
               int(accumulate), ptr(ws), stream())
        return dw
    _conv_wgrad_launch(plan, x, dy, dw, accumulate)
    return dw


# GCA_STEM_DZF=0: the first layer's BatchNorm backward writes dy and its weight gradient reads it back (A/B runs)
STEM_DZF = os.environ.get('GCA_STEM_DZF', '1') != '0'


def conv_dzf_ok(plan):
    """True when, under the launch shape pinned in `plan`, the weight gradient runs on the stem kernel, which can form dy from
    (dz, y, BatchNorm-backward constants) in registers: gca_conv_dzf_ok."""
    return plan.tuned[2] and bool(H.lib.gca_conv_dzf_ok(plan.gp))


def conv_wgrad_dzf(plan, x, dz, y, consts, relu, dw, accumulate=True):
    """conv_wgrad against dy = BatchNorm backward of (dz, y) with the constants of bn_bwd_sums, never materialised
    (gca_conv_wgrad_dzf; only where conv_dzf_ok(plan)).  relu: 0 or 2, as given to bn_bwd_sums."""
    if not plan.tuned[2]:
        raise RuntimeError('conv_wgrad_dzf needs a tuned plan (conv_dzf_ok)')
    d = DEFER[0]
    if d is not None and dw.is_contiguous():
        d.add(plan, x, dz, dw, accumulate, dzf=(y, consts, relu))
        return dw
    ws = WS.get(plan.wgrad_ws, x.device)
    H.call('gca_conv_wgrad_dzf', plan.gp, _act(plan, x), _act(plan, dz), _act(plan, y), ptr(consts), int(relu), ptr(plan.table(2)),
           ptr(dw), int(accumulate), ptr(ws), stream())
    return dw


def bias_grad(dy, N, K, SP, db, accumulate=True):
    H.call('gca_bias_grad', ptr(dy), N, K, SP, ptr(db), int(accumulate), stream())


# ----------------------------------------------------------------------------- batch norm
def bn_stats(x, N, Cc, SP):
    P = H.lib.gca_bn_stats_parts(N, Cc, SP)
    ss = torch.empty((Cc, P), dtype=F32, device=x.device)
    sq = torch.empty((Cc, P), dtype=F32, device=x.device)
    H.call('gca_bn_stats', aptr(x), N, Cc, SP, ptr(ss), ptr(sq), None, is_half(x), stream())
    return ss, sq


def bn_finalize(ss, sq, count, gamma, beta, eps, momentum, rmean, rvar, nbt):
    """-> (save_mean, save_invstd, scale, shift); running stats updated in place."""
    Cc, P = ss.shape
    # rows padded to a multiple of 16 + 16 floats: a consumer that applies (scale, shift) while it stages its input
    # (conv_fwd_xf) reads whole 16-channel chunks
    Cp = -(-Cc // 16) * 16 + 16
    out = torch.empty((4, Cp), dtype=F32, device=ss.device)      # (the pad is never used as a number: consumers select on c < C)
    H.call('gca_bn_finalize', ptr(ss), ptr(sq), P, Cc, float(count), ptr(gamma), ptr(beta), float(eps),
           float(momentum), ptr(rmean), ptr(rvar), ptr(nbt), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]),
           stream())
    return out[0][:Cc], out[1][:Cc], out[2][:Cc], out[3][:Cc]


def bn_train_fwd(ss, sq, count, gamma, beta, eps, momentum, rmean, rvar, nbt, x, residual, relu, N, Cc, SP, out=None):
    """bn_finalize + bn_apply behind one call (one launch for small N*SP).
    -> (z, save_mean, save_invstd, scale, shift); running stats updated in place."""
    P = ss.shape[1]
    st = torch.empty((4, Cc), dtype=F32, device=ss.device)
    z = torch.empty_like(x) if out is None else out
    H.call('gca_bn_train_fwd', ptr(ss), ptr(sq), P, Cc, float(count), ptr(gamma), ptr(beta), float(eps), float(momentum),
           ptr(rmean), ptr(rvar), ptr(nbt), ptr(st[0]), ptr(st[1]), ptr(st[2]), ptr(st[3]), aptr(x), aptr(residual),
           int(relu), N, SP, aptr(z), _slice_stride(z, Cc, SP), is_half(x, residual, z), stream())
    return z, st[0], st[1], st[2], st[3]


# GCA_FUSE_SPLITK_BN=0: a split-K conv in front of a small BatchNorm finishes its slabs in its own launch (A/B runs)
FUSE_SPLITK_BN = os.environ.get('GCA_FUSE_SPLITK_BN', '1') != '0'


def conv_bn_small_fwd(plan, x, wpack, count, gamma, beta, eps, momentum, rmean, rvar, nbt, residual, relu, out=None):
    """conv forward whose pinned launch shape splits the reduction + training-mode BatchNorm of a small map, in two launches:
    the conv leaves its slabs in the scratch lane (gca_conv_fwd_slabs), the BatchNorm kernel folds them, writes y and z
    (gca_bn_train_fwd_slabs).  -> (y, z, save_mean, save_invstd, scale, shift)"""
    N, K, OD, OH, OW = plan.out_shape
    SP = OD * OH * OW
    ws = WS.get(plan.fwd_ws, x.device)
    splits = C.c_int32(0)
    H.call('gca_conv_fwd_slabs', plan.gp, ptr(x), ptr(wpack), ptr(plan.table(0)), ptr(ws), C.addressof(splits), stream())
    y = torch.empty(plan.out_shape, dtype=F32, device=x.device)
    z = torch.empty_like(y) if out is None else out
    st = torch.empty((4, K), dtype=F32, device=x.device)
    H.call('gca_bn_train_fwd_slabs', ptr(ws), int(splits.value), float(count), ptr(gamma), ptr(beta), float(eps), float(momentum),
           ptr(rmean), ptr(rvar), ptr(nbt), ptr(st[0]), ptr(st[1]), ptr(st[2]), ptr(st[3]), ptr(y), ptr(residual), int(relu),
           N, K, SP, ptr(z), _slice_stride(z, K, SP), stream())
    return y, z, st[0], st[1], st[2], st[3]


def bn_fold_eval(gamma, beta, rmean, rvar, eps):
    Cc = rmean.numel()
    out = torch.empty((2, Cc), dtype=F32, device=rmean.device)
    H.call('gca_bn_fold_eval', ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), float(eps), Cc, ptr(out[0]), ptr(out[1]),
           stream())
    return out[0], out[1]


def _slice_stride(t, Cc, SP):
    """0 for a contiguous (N,C,...) tensor, else the batch stride of a channel-slice view."""
    if t.is_contiguous():
        return 0
    if t.dim() < 2 or t[0].is_contiguous() is False:
        raise RuntimeError('only channel slices of a contiguous (N, Ctot, ...) buffer are supported')
    return t.stride(0)


def bn_apply(x, scale, shift, residual, relu, N, Cc, SP, out=None):
    z = torch.empty_like(x) if out is None else out
    H.call('gca_bn_apply', aptr(x), ptr(scale), ptr(shift), aptr(residual), int(relu), N, Cc, SP, aptr(z),
           _slice_stride(z, Cc, SP), is_half(x, residual, z), stream())
    return z


def bn_bwd(dz, z, x, gamma, mean, invstd, relu, N, Cc, SP, dgamma, dbeta, dres=None, dres_accumulate=False,
           scale=None, shift=None):
    """relu: False/0 none, True/1 mask from z, 2 mask recomputed from x with the forward's (scale, shift)."""
    dx = torch.empty_like(x)
    ws = WS.get(H.lib.gca_bn_bwd_ws_bytes(N, Cc, SP), x.device)
    H.call('gca_bn_bwd', aptr(dz), aptr(z) if int(relu) == 1 else None, aptr(x), ptr(gamma), ptr(mean), ptr(invstd), int(relu),
           N, Cc, SP, aptr(dx), ptr(dgamma), ptr(dbeta), aptr(dres), int(dres_accumulate), _slice_stride(dz, Cc, SP),
           ptr(scale), ptr(shift), ptr(ws), is_half(dz, z if int(relu) == 1 else None, x, dres), stream())
    return dx


def bn_bwd_sums(dz, x, gamma, mean, invstd, relu, N, Cc, SP, dgamma, dbeta, scale=None, shift=None):
    """bn_bwd without its apply pass (relu 0 or 2): dgamma / dbeta accumulated as bn_bwd does, and -> the constant array
    [7][16 * ceil(C / 16) + 16] from which conv_wgrad_dzf forms dx where it reads it."""
    consts = torch.empty(H.lib.gca_bn_bwd_consts_elems(Cc), dtype=F32, device=x.device)
    ws = WS.get(H.lib.gca_bn_bwd_ws_bytes(N, Cc, SP), x.device)
    H.call('gca_bn_bwd_sums', aptr(dz), aptr(x), ptr(gamma), ptr(mean), ptr(invstd), int(relu), N, Cc, SP, ptr(dgamma), ptr(dbeta),
           _slice_stride(dz, Cc, SP), ptr(scale), ptr(shift), ptr(consts), ptr(ws), is_half(dz, x), stream())
    return consts


# ----------------------------------------------------------------------------- pooling
class PoolPlan:
    def __init__(self, x_shape, k, s, p):
        N, Cc, D, Hh, W = x_shape
        kd, kh, kw = _t3(k)
        sd, sh, sw = _t3(s)
        pd, ph, pw = _t3(p)
        OD, OH, OW = (D + 2 * pd - kd) // sd + 1, (Hh + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
        self.g = H.PoolGeom(N, Cc, D, Hh, W, kd, kh, kw, sd, sh, sw, pd, ph, pw, OD, OH, OW)
        self.gp = C.byref(self.g)
        self.in_shape, self.out_shape = tuple(x_shape), (N, Cc, OD, OH, OW)


@functools.lru_cache(maxsize=None)
def pool_plan(x_shape, k, s, p):
    return PoolPlan(x_shape, k, s, p)


def maxpool_fwd(plan, x, want_argmax=True, scale=None, shift=None):
    """scale/shift: pool relu(x*scale[c]+shift[c]) (the BatchNorm+ReLU in front of the pool) without materialising it."""
    y = torch.empty(plan.out_shape, dtype=x.dtype, device=x.device)
    am = torch.empty(plan.out_shape, dtype=torch.int32, device=x.device) if want_argmax else None
    H.call('gca_maxpool3d_fwd', plan.gp, aptr(x), aptr(y), ptr(am), ptr(scale), ptr(shift), is_half(x), stream())
    return y, am


def maxpool_bwd(plan, dy, argmax, dx=None, accumulate=False):
    if dx is None:
        dx = torch.empty(plan.in_shape, dtype=dy.dtype, device=dy.device)
        accumulate = False
    H.call('gca_maxpool3d_bwd', plan.gp, aptr(dy), ptr(argmax), aptr(dx), int(accumulate), is_half(dy, dx), stream())
    return dx


def avgpool_fwd(plan, x):
    """nn.AvgPool3d(kernel_size=k) (stride k, no padding) on fp32 maps."""
    y = torch.empty(plan.out_shape, dtype=F32, device=x.device)
    H.call('gca_avgpool3d_fwd', plan.gp, ptr(x), ptr(y), stream())
    return y


def avgpool_bwd(plan, dy, dx=None, accumulate=False):
    if dx is None:
        dx = torch.empty(plan.in_shape, dtype=F32, device=dy.device)
        accumulate = False
    H.call('gca_avgpool3d_bwd', plan.gp, ptr(dy), ptr(dx), int(accumulate), stream())
    return dx


def wavgpool_fwd(x, wt, norm):
    N, Cc, D, Hh, W = x.shape
    y = torch.empty((N, Cc), dtype=F32, device=x.device)
    H.call('gca_wavgpool_fwd', aptr(x), ptr(wt), float(norm), N * Cc, D, Hh * W, ptr(y), is_half(x), stream())
    return y


def wavgpool_bwd(dy, wt, norm, x_shape, dtype=F32):
    N, Cc, D, Hh, W = x_shape
    dx = torch.empty(x_shape, dtype=dtype, device=dy.device)
    H.call('gca_wavgpool_bwd', ptr(dy), ptr(wt), float(norm), N * Cc, D, Hh * W, aptr(dx), is_half(dx), stream())
    return dx


# ----------------------------------------------------------------------------- head pieces
def relu_fwd(x):
    y = torch.empty_like(x)
    H.call('gca_relu_fwd', ptr(x), x.numel(), ptr(y), stream())
    return y


def relu_bwd(dy, y):
    dx = torch.empty_like(dy)
    H.call('gca_relu_bwd', ptr(dy), ptr(y), dy.numel(), ptr(dx), stream())
    return dx


def l2norm_fwd(x, eps=1e-12):
    rows, dim = x.shape
    y = torch.empty_like(x)
    inv = torch.empty(rows, dtype=F32, device=x.device)
    H.call('gca_l2norm_fwd', ptr(x), rows, dim, float(eps), ptr(y), ptr(inv), stream())
    return y, inv


def l2norm_bwd(dy, y, inv):
    rows, dim = y.shape
    dx = torch.empty_like(y)
    H.call('gca_l2norm_bwd', ptr(dy), ptr(y), ptr(inv), rows, dim, ptr(dx), stream())
    return dx


def negcos(p, z, scale, loss_buf, accumulate):
    """loss_buf: (1 + rows) floats; returns dp."""
    rows, dim = p.shape
    dp = torch.empty_like(p)
    H.call('gca_negcos_fwd_bwd', ptr(p), ptr(z), rows, dim, float(scale), ptr(loss_buf), int(accumulate), ptr(dp),
           stream())
    return dp


# ----------------------------------------------------------------------------- MoCo / InfoNCE
_NCE_SYNC = {}


def _nce_sync(device):
    """The zero-initialised ticket counter of the single-launch InfoNCE forward.  Every call leaves it at zero (the last
    workgroup re-arms it; the GCA_NCE_DEBUG early exits either draw no ticket at all or re-arm it too), and calls on ONE
    stream are ordered, so a counter may be shared exactly by the calls that already share a scratch buffer: one per
    (device, scratch lane).  Work issued on a second stream must run under its own lane (ops.WS_LANE, as the trainers' key
    encoder does) -- that rule already holds for every workspace user (the partials of this kernel live in WS.get), and with
    it two concurrent RGBMoCo.forward calls never interleave their tickets."""
    key = (device.type, device.index, WS_LANE[0])
    c = _NCE_SYNC.get(key)
    if c is None:
        c = _NCE_SYNC[key] = torch.zeros(16, dtype=torch.int32, device=device)
    return c


def moco_logits_fwd(q, k, queue, inv_T, want_lse=False, want_rank=False, want_loss=False, logits=None):
    """-> (logits, lse, rank) [+ (loss,) when want_loss: the InfoNCE loss of these logits, fused into the same launch
    (b <= 32) -- the separate nce_loss_fwd call is then unnecessary].  logits: optional (b, K+1) output buffer."""
    b, D = q.shape
    K = queue.shape[0]
    want_lse = want_lse or want_loss
    if logits is None:
        logits = torch.empty((b, K + 1), dtype=F32, device=q.device)
    lse = torch.empty(b, dtype=F32, device=q.device) if want_lse else None
    rank = torch.empty(b, dtype=torch.int32, device=q.device) if want_rank else None
    loss = torch.empty(1, dtype=F32, device=q.device) if want_loss else None
    ws = WS.get(H.lib.gca_infonce_ws_bytes(b, K), q.device)
    H.call('gca_moco_logits_fwd', ptr(q), ptr(k), ptr(queue), b, K, D, float(inv_T), ptr(logits), ptr(lse), ptr(rank),
           ptr(loss), ptr(ws), ptr(_nce_sync(q.device)), stream())
    return (logits, lse, rank, loss) if want_loss else (logits, lse, rank)


def nce_loss_fwd(logits, lse=None):
    b, ncol = logits.shape
    loss = torch.empty(1, dtype=F32, device=logits.device)
    lse_out = None
    if lse is None:
        lse_out = torch.empty(b, dtype=F32, device=logits.device)
    H.call('gca_nce_softmax_loss_fwd', ptr(logits), b, ncol, ptr(lse), ptr(lse_out), ptr(loss), stream())
    return loss, (lse if lse is not None else lse_out)


def nce_loss_bwd(logits, lse, gscale_dev=None, gscale_host=1.0):
    b, ncol = logits.shape
    dl = torch.empty_like(logits)
    H.call('gca_nce_softmax_loss_bwd', ptr(logits), ptr(lse), b, ncol, ptr(gscale_dev), float(gscale_host), ptr(dl),
           stream())
    return dl


def moco_logits_bwd(k, queue, inv_T, dlogits=None, logits=None, lse=None, gscale_dev=None, gscale_host=1.0,
                    ov_start=0, ov_rows=None, ov_start_dev=None):
    b, D = k.shape
    K = queue.shape[0]
    dq = torch.empty((b, D), dtype=F32, device=k.device)
    ws = WS.get(H.lib.gca_infonce_ws_bytes(b, K), k.device)
    ov_n = 0 if ov_rows is None else ov_rows.shape[0]
    H.call('gca_moco_logits_bwd', ptr(dlogits), ptr(logits), ptr(lse), ptr(gscale_dev), float(gscale_host), ptr(k),
           ptr(queue), b, K, D, float(inv_T), int(ov_start), ptr(ov_start_dev), int(ov_n), ptr(ov_rows), ptr(dq),
           ptr(ws), stream())
    return dq


def queue_enqueue(queue, keys, ptr_index, save=False, ptr_dev=None):
    K, D = queue.shape
    n = keys.shape[0]
    saved = torch.empty((n, D), dtype=F32, device=queue.device) if save else None
    H.call('gca_queue_enqueue', ptr(queue), K, D, ptr(keys), n, int(ptr_index), ptr(ptr_dev), ptr(saved), stream())
    return saved


def queue_advance(ptr_dev, n, K):
    H.call('gca_queue_advance', ptr(ptr_dev), int(n), int(K), stream())


# ----------------------------------------------------------------------------- retrieval
RETRIEVAL_METRICS = {'cosine': 0, 'euclidean': 1}


def retrieval_topk(q, g, k, metric='cosine', q_label=None, g_label=None, slabs=0):
    """Nearest gallery rows of every query without the (nq, ng) distance matrix (tools/video_retrieval.py:174-197):
    q (nq, D), g (ng, D) fp32 on the device -> (idx (nq, k) int32, dist (nq, k) fp32, first_hit (nq) int32 or None).
    Ascending by (distance, gallery index); idx = -1 / dist = +inf past the end of a gallery shorter than k.  With int64
    labels on both sides, first_hit is the 1-based rank of the first row of the query's class, k + 1 if none.  `slabs`
    forces the number of gallery slabs (0 = fill the device); the result does not depend on it.  tests/retrieval_ref.py
    states the arithmetic.  ValueError for arguments the kernel entry refuses."""
    if metric not in RETRIEVAL_METRICS:
        raise ValueError('retrieval_topk: metric must be one of %s (got %r)' % (sorted(RETRIEVAL_METRICS), metric))
    if q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1]:
        raise ValueError('retrieval_topk: q (nq, D) and g (ng, D) must share D (got %s, %s)' % (tuple(q.shape), tuple(g.shape)))
    for lab, n in ((q_label, q.shape[0]), (g_label, g.shape[0])):
        if lab is not None and (lab.dtype is not torch.int64 or lab.dim() != 1 or lab.shape[0] != n):
            raise ValueError('retrieval_topk: labels are int64 vectors, one entry per row')
    if (q_label is None) != (g_label is None):
        raise ValueError('retrieval_topk: labels on both sides or on neither')
    nq, D = q.shape
    ng, k, slabs = g.shape[0], int(k), int(slabs)
    if not -2 ** 31 <= k < 2 ** 31 or not -2 ** 31 <= slabs < 2 ** 31:
        raise ValueError('retrieval_topk: k / slabs out of range')
    nbytes = H.lib.gca_retrieval_ws_bytes(nq, ng, D, k, slabs)
    if nbytes < 0:
        raise ValueError('retrieval_topk: invalid arguments (nq=%d, ng=%d, D=%d, k=%d, slabs=%d)' % (nq, ng, D, k, slabs))
    q, g = q.contiguous(), g.contiguous()
    ql = None if q_label is None else q_label.contiguous()
    gl = None if g_label is None else g_label.contiguous()
    dev = q.device
    labelled = ql is not None
    if nq == 0 or ng == 0:         # nothing to search and nothing launched: every slot is tail
        return (torch.full((nq, k), -1, dtype=torch.int32, device=dev), torch.full((nq, k), float('inf'), dtype=F32, device=dev),
                torch.full((nq,), k + 1, dtype=torch.int32, device=dev) if labelled else None)
    idx = torch.empty((nq, k), dtype=torch.int32, device=dev)
    dist = torch.empty((nq, k), dtype=F32, device=dev)
    hit = torch.empty((nq,), dtype=torch.int32, device=dev) if labelled else None
    ws = WS.get(nbytes, dev)
    rc = H.lib.gca_retrieval_topk(ptr(q), ptr(g), nq, ng, D, k, RETRIEVAL_METRICS[metric], ptr(ql), ptr(gl), slabs, ptr(idx),
                                  ptr(dist), ptr(hit), ptr(ws), nbytes, stream())
    if rc == -1:
        raise ValueError('retrieval_topk: gca_retrieval_topk refused its arguments (labels on one side only?)')
    H.check(rc, 'gca_retrieval_topk')
    return idx, dist, hit


KNN_WEIGHTINGS = {'uniform': 0, 'exp': 1}


def knn_vote(idx, dist, g_label, num_class, kvote=None, q_label=None, self_base=-1, weighting='exp', T=0.07, want_scores=False):
    """Weighted k-NN vote on retrieval_topk's lists (gca_knn_vote; tests/knn_ref.py states the arithmetic): idx (nq, k) int32,
    dist (nq, k) fp32, g_label (ng) int64 -> (pred (nq) int32, rank (nq) int32 or None, scores (nq, num_class) fp32 or None).
    The first `kvote` (default k) valid slots of a row vote, each with weight 1 ('uniform') or exp(-dist / T) ('exp'); pred
    is the class with the largest weight sum (ties: the lower class), -1 for a row without voters.  With q_label (nq) int64,
    rank counts the other classes that come before the query's own (top-k' is correct iff rank < k').  self_base >= 0
    drops slot idx == self_base + row (leave-one-out on a slice of the gallery).  ValueError for arguments the kernel entry
    refuses; labels are not range-checked here (out-of-range gallery labels do not vote)."""
    if weighting not in KNN_WEIGHTINGS:
        raise ValueError('knn_vote: weighting must be one of %s (got %r)' % (sorted(KNN_WEIGHTINGS), weighting))
    if idx.dim() != 2 or tuple(dist.shape) != tuple(idx.shape) or idx.dtype is not torch.int32 or dist.dtype is not F32:
        raise ValueError('knn_vote: idx (nq, k) int32 and dist (nq, k) fp32 expected (got %s %s, %s %s)'
                         % (tuple(idx.shape), idx.dtype, tuple(dist.shape), dist.dtype))
    if g_label.dtype is not torch.int64 or g_label.dim() != 1:
        raise ValueError('knn_vote: g_label is an int64 vector')
    nq, k = idx.shape
    if q_label is not None and (q_label.dtype is not torch.int64 or tuple(q_label.shape) != (nq,)):
        raise ValueError('knn_vote: q_label is an int64 vector, one label per query')
    ng, Cc, self_base = g_label.shape[0], int(num_class), int(self_base)
    kvote = k if kvote is None else int(kvote)
    if not 1 <= k <= 64 or not 1 <= kvote <= k:
        raise ValueError('knn_vote: 1 <= kvote <= k <= 64 required (k=%d, kvote=%d)' % (k, kvote))
    if Cc < 1 or Cc >= 2 ** 63 or ng >= 2 ** 31 or nq >= 2 ** 31 or not -2 ** 63 <= self_base < 2 ** 63:
        raise ValueError('knn_vote: invalid sizes (nq=%d, ng=%d, num_class=%d)' % (nq, ng, Cc))
    if want_scores and nq * Cc >= 2 ** 31:
        raise ValueError('knn_vote: a (%d, %d) score block has 2^31 elements or more' % (nq, Cc))
    T = float(T)
    inv_T = 1.0 / T if T > 0 else float('nan')
    if not (T > 0 and inv_T < 3.0e38):
        raise ValueError('knn_vote: the temperature must be positive, 1 / T finite in fp32 (got %r)' % T)
    idx, dist, g_label = idx.contiguous(), dist.contiguous(), g_label.contiguous()
    ql = None if q_label is None else q_label.contiguous()
    pi, pd, pg, pq = ptr(idx), ptr(dist), ptr(g_label), ptr(ql)          # (RuntimeError for host tensors)
    dev = idx.device
    pred = torch.empty((nq,), dtype=torch.int32, device=dev)
    rank = torch.empty((nq,), dtype=torch.int32, device=dev) if ql is not None else None
    scores = torch.empty((nq, Cc), dtype=F32, device=dev) if want_scores else None
    rc = H.lib.gca_knn_vote(pi, pd, nq, k, kvote, pg, ng, pq, self_base, Cc, KNN_WEIGHTINGS[weighting], inv_T, ptr(scores),
                            ptr(pred), ptr(rank), stream())
    if rc == -1:
        raise ValueError('knn_vote: gca_knn_vote refused its arguments')
    H.check(rc, 'gca_knn_vote')
    return pred, rank, scores


# ----------------------------------------------------------------------------- NT-Xent (SimCLR)
def _ntxent_args(z, inv_T, what):
    """Host-side refusals of gca_ntxent_fwd / _bwd (before any device is touched) -> (N, D, inv_T)."""
    if z.dim() != 2 or z.dtype is not F32:
        raise ValueError('%s: z is a (N, D) fp32 matrix (got %s %s)' % (what, tuple(z.shape), z.dtype))
    N, D = z.shape
    if N < 2 or N % 2 or N > 65536 or D < 1 or N * D >= 2 ** 31:
        raise ValueError('%s: N must be even, 2 <= N <= 65536, D >= 1, N * D < 2^31 (got N=%d, D=%d)' % (what, N, D))
    inv_T = float(inv_T)
    if not 0.0 < inv_T < 3.0e38:
        raise ValueError('%s: 1 / T must be positive and finite in fp32 (got %r)' % (what, inv_T))
    return N, D, inv_T


def ntxent_fwd(z, inv_T, want_rank=False):
    """NT-Xent forward (gca_ntxent_fwd; tests/ntxent_ref.py states the arithmetic): z (N, D) fp32 with rows 0..N/2-1 view 1 and
    N/2..N-1 view 2 -> (loss (1,), lse (N,), rank (N,) int32 or None), all on the device.  rank[i] counts the negatives of
    row i that score at least its positive (top-k hit iff rank < k).  ValueError for arguments the kernel entry refuses."""
    N, D, inv_T = _ntxent_args(z, inv_T, 'ntxent_fwd')
    z = z.contiguous()
    pz = ptr(z)                                                         # (RuntimeError for host tensors)
    dev = z.device
    loss = torch.empty(1, dtype=F32, device=dev)
    lse = torch.empty(N, dtype=F32, device=dev)
    rank = torch.empty(N, dtype=torch.int32, device=dev) if want_rank else None
    ws = WS.get(H.lib.gca_ntxent_ws_bytes(N, D), dev)
    H.call('gca_ntxent_fwd', pz, N, D, inv_T, ptr(lse), None, ptr(rank), ptr(loss), ptr(ws), stream())
    return loss, lse, rank


def ntxent_bwd(z, lse, inv_T, gscale_dev=None, gscale_host=1.0):
    """d loss / d z of ntxent_fwd from its row log-sum-exps, times gscale_host * (*gscale_dev if given) -> dz (N, D)."""
    N, D, inv_T = _ntxent_args(z, inv_T, 'ntxent_bwd')
    if lse.dtype is not F32 or tuple(lse.shape) != (N,):
        raise ValueError('ntxent_bwd: lse is the (N,) fp32 vector of ntxent_fwd (got %s %s)' % (tuple(lse.shape), lse.dtype))
    z, lse = z.contiguous(), lse.contiguous()
    pz, pl = ptr(z), ptr(lse)
    dz = torch.empty((N, D), dtype=F32, device=z.device)
    ws = WS.get(H.lib.gca_ntxent_ws_bytes(N, D), z.device)
    H.call('gca_ntxent_bwd', pz, pl, N, D, inv_T, ptr(gscale_dev), float(gscale_host), ptr(dz), ptr(ws), stream())
    return dz


# ----------------------------------------------------------------------------- Barlow Twins
def _barlow_args(z1, z2, lambd, eps, what):
    """Host-side refusals of gca_barlow_fwd / _bwd (before any device is touched) -> (N, D, lambda, eps)."""
    for z in (z1, z2):
        if z.dim() != 2 or z.dtype is not F32:
            raise ValueError('%s: z1 and z2 are (N, D) fp32 matrices (got %s %s)' % (what, tuple(z.shape), z.dtype))
    if z1.shape != z2.shape:
        raise ValueError('%s: the two views differ in shape (%s, %s)' % (what, tuple(z1.shape), tuple(z2.shape)))
    N, D = z1.shape
    if N < 2 or N > 65536 or D < 1 or D > 8192 or N * D >= 2 ** 31:
        raise ValueError('%s: 2 <= N <= 65536, 1 <= D <= 8192, N * D < 2^31 (got N=%d, D=%d)' % (what, N, D))
    lambd, eps = float(lambd), float(eps)
    if not 0.0 <= lambd < 3.0e38:
        raise ValueError('%s: lambda must be non-negative and finite in fp32 (got %r)' % (what, lambd))
    if not 0.0 <= eps < 3.0e38:
        raise ValueError('%s: eps must be non-negative and finite in fp32 (got %r)' % (what, eps))
    return N, D, lambd, eps


def barlow_fwd(z1, z2, lambd, eps=1e-5):
    """Barlow Twins forward (gca_barlow_fwd; tests/barlow_ref.py states the arithmetic): the (N, D) fp32 projector outputs of
    the two views -> (loss3 = [loss, on, off], stats (4, D) = mean_1, rstd_1, mean_2, rstd_2, cmat (D, D), rsum (2, D)), all on
    the device; stats, cmat and rsum are what barlow_bwd needs.  ValueError for arguments the kernel entry refuses."""
    N, D, lambd, eps = _barlow_args(z1, z2, lambd, eps, 'barlow_fwd')
    z1, z2 = z1.contiguous(), z2.contiguous()
    p1, p2 = ptr(z1), ptr(z2)                                           # (RuntimeError for host tensors)
    dev = z1.device
    loss3 = torch.empty(3, dtype=F32, device=dev)
    stats = torch.empty((4, D), dtype=F32, device=dev)
    cmat = torch.empty((D, D), dtype=F32, device=dev)
    rsum = torch.empty((2, D), dtype=F32, device=dev)
    ws = WS.get(H.lib.gca_barlow_ws_bytes(N, D), dev)
    H.call('gca_barlow_fwd', p1, p2, N, D, lambd, eps, ptr(stats), ptr(cmat), ptr(rsum), ptr(loss3), ptr(ws), stream())
    return loss3, stats, cmat, rsum


def barlow_bwd(z1, z2, stats, cmat, rsum, lambd, gscale_dev=None, gscale_host=1.0):
    """d loss / d (z1, z2) of barlow_fwd from its saved state, times gscale_host * (*gscale_dev if given) -> (dz1, dz2)."""
    N, D, lambd, _ = _barlow_args(z1, z2, lambd, 0.0, 'barlow_bwd')
    gscale_host = float(gscale_host)
    if not -3.0e38 < gscale_host < 3.0e38:
        raise ValueError('barlow_bwd: gscale_host must be finite in fp32 (got %r)' % gscale_host)
    for t, shape, name in ((stats, (4, D), 'stats'), (cmat, (D, D), 'cmat'), (rsum, (2, D), 'rsum')):
        if t.dtype is not F32 or tuple(t.shape) != shape:
            raise ValueError('barlow_bwd: %s is the %s fp32 tensor of barlow_fwd (got %s %s)' % (name, shape, tuple(t.shape), t.dtype))
    z1, z2, stats, cmat, rsum = (t.contiguous() for t in (z1, z2, stats, cmat, rsum))
    p1, p2 = ptr(z1), ptr(z2)
    dz1 = torch.empty((N, D), dtype=F32, device=z1.device)
    dz2 = torch.empty((N, D), dtype=F32, device=z1.device)
    ws = WS.get(H.lib.gca_barlow_ws_bytes(N, D), z1.device)
    H.call('gca_barlow_bwd', p1, p2, ptr(stats), ptr(cmat), ptr(rsum), N, D, lambd, ptr(gscale_dev), gscale_host, ptr(dz1),
           ptr(dz2), ptr(ws), stream())
    return dz1, dz2


# ----------------------------------------------------------------------------- VICReg
def _vicreg_args(z1, z2, sim, std, cov, eps, what):
    """Host-side refusals of gca_vicreg_fwd / _bwd (before any device is touched) -> (N, D, sim, std, cov, eps)."""
    for z in (z1, z2):
        if z.dim() != 2 or z.dtype is not F32:
            raise ValueError('%s: z1 and z2 are (N, D) fp32 matrices (got %s %s)' % (what, tuple(z.shape), z.dtype))
    if z1.shape != z2.shape:
        raise ValueError('%s: the two views differ in shape (%s, %s)' % (what, tuple(z1.shape), tuple(z2.shape)))
    N, D = z1.shape
    if N < 2 or N > 65536 or D < 1 or D > 8192 or N * D >= 2 ** 31:
        raise ValueError('%s: 2 <= N <= 65536, 1 <= D <= 8192, N * D < 2^31 (got N=%d, D=%d)' % (what, N, D))
    vals = []
    for name, v in (('sim', sim), ('std', std), ('cov', cov), ('eps', eps)):
        v = float(v)
        if not 0.0 <= v < 3.0e38:
            raise ValueError('%s: %s must be non-negative and finite in fp32 (got %r)' % (what, name, v))
        vals.append(v)
    return (N, D) + tuple(vals)


def vicreg_fwd(z1, z2, sim, std, cov, eps=1e-4):
    """VICReg forward (gca_vicreg_fwd; tests/vicreg_ref.py states the arithmetic): the (N, D) fp32 projector outputs of the two
    views -> (loss4 = [loss, inv, varl, covl] with the parts unweighted, stats (4, D) = mean_1, sd_1, mean_2, sd_2, covm
    (2, D, D), 8 D^2 bytes), all on the device; stats and covm are what vicreg_bwd needs.  ValueError for arguments the kernel
    entry refuses."""
    N, D, sim, std, cov, eps = _vicreg_args(z1, z2, sim, std, cov, eps, 'vicreg_fwd')
    z1, z2 = z1.contiguous(), z2.contiguous()
    p1, p2 = ptr(z1), ptr(z2)                                           # (RuntimeError for host tensors)
    dev = z1.device
    loss4 = torch.empty(4, dtype=F32, device=dev)
    stats = torch.empty((4, D), dtype=F32, device=dev)
    covm = torch.empty((2, D, D), dtype=F32, device=dev)
    ws = WS.get(H.lib.gca_vicreg_ws_bytes(N, D), dev)
    H.call('gca_vicreg_fwd', p1, p2, N, D, sim, std, cov, eps, ptr(stats), ptr(covm), ptr(loss4), ptr(ws), stream())
    return loss4, stats, covm


def vicreg_bwd(z1, z2, stats, covm, sim, std, cov, gscale_dev=None, gscale_host=1.0):
    """d loss / d (z1, z2) of vicreg_fwd from its saved state, times gscale_host * (*gscale_dev if given) -> (dz1, dz2)."""
    N, D, sim, std, cov, _ = _vicreg_args(z1, z2, sim, std, cov, 0.0, 'vicreg_bwd')
    gscale_host = float(gscale_host)
    if not -3.0e38 < gscale_host < 3.0e38:
        raise ValueError('vicreg_bwd: gscale_host must be finite in fp32 (got %r)' % gscale_host)
    for t, shape, name in ((stats, (4, D), 'stats'), (covm, (2, D, D), 'covm')):
        if t.dtype is not F32 or tuple(t.shape) != shape:
            raise ValueError('vicreg_bwd: %s is the %s fp32 tensor of vicreg_fwd (got %s %s)' % (name, shape, tuple(t.shape), t.dtype))
    z1, z2, stats, covm = (t.contiguous() for t in (z1, z2, stats, covm))
    p1, p2 = ptr(z1), ptr(z2)
    dz1 = torch.empty((N, D), dtype=F32, device=z1.device)
    dz2 = torch.empty((N, D), dtype=F32, device=z1.device)
    ws = WS.get(H.lib.gca_vicreg_ws_bytes(N, D), z1.device)
    H.call('gca_vicreg_bwd', p1, p2, ptr(stats), ptr(covm), N, D, sim, std, cov, ptr(gscale_dev), gscale_host, ptr(dz1), ptr(dz2),
           ptr(ws), stream())
    return dz1, dz2


# ----------------------------------------------------------------------------- SwAV
def rows_normalize_(C):
    """C[k,:] /= ||C[k,:]|| in place (gca_rows_normalize): C (K, D) fp32 contiguous on the device, 1 <= K <= 65536,
    1 <= D <= 8192; an all-zero row is left as it is.  -> C."""
    if C.dim() != 2 or C.dtype is not F32 or not C.is_contiguous():
        raise ValueError('rows_normalize_: C is a contiguous (K, D) fp32 matrix (got %s %s)' % (tuple(C.shape), C.dtype))
    K, D = C.shape
    if not (1 <= K <= 65536 and 1 <= D <= 8192):
        raise ValueError('rows_normalize_: 1 <= K <= 65536, 1 <= D <= 8192 (got K=%d, D=%d)' % (K, D))
    H.call('gca_rows_normalize', ptr(C), K, D, stream())
    return C


def _swav_args(z1, z2, C, what):
    """Host-side refusals of gca_swav_fwd / _bwd on the shapes (before any device is touched) -> (N, D, K)."""
    for z in (z1, z2):
        if z.dim() != 2 or z.dtype is not F32:
            raise ValueError('%s: z1 and z2 are (N, D) fp32 matrices (got %s %s)' % (what, tuple(z.shape), z.dtype))
    if z1.shape != z2.shape:
        raise ValueError('%s: the two views differ in shape (%s, %s)' % (what, tuple(z1.shape), tuple(z2.shape)))
    N, D = z1.shape
    if C.dim() != 2 or C.dtype is not F32 or C.shape[1] != D:
        raise ValueError('%s: the prototypes C are a (K, D) fp32 matrix with D = %d (got %s %s)' % (what, D, tuple(C.shape), C.dtype))
    K = C.shape[0]
    if not (2 <= N <= 8192 and 2 <= K <= 65536 and 1 <= D <= 8192):
        raise ValueError('%s: 2 <= N <= 8192, 2 <= K <= 65536, 1 <= D <= 8192 (got N=%d, K=%d, D=%d)' % (what, N, K, D))
    return N, D, K


def swav_params(what, eps, T, iters):
    """-> (eps, T, iters) as gca_swav_fwd accepts them; ValueError otherwise (0.025 <= eps <= 1, T > 0 with T and 1 / T finite
    in fp32, 1 <= iters <= 16)."""
    import ctypes
    eps, T = float(eps), float(T)
    if isinstance(iters, bool) or int(iters) != iters:
        raise ValueError('%s: iters is an integer (got %r)' % (what, iters))
    iters = int(iters)
    if not ctypes.c_float(0.025).value <= ctypes.c_float(eps).value <= 1.0:
        raise ValueError('%s: eps must lie in [0.025, 1] (got %r)' % (what, eps))
    if not 1.2e-38 < T < 3.0e38:
        raise ValueError('%s: T must be positive, T and 1 / T finite in fp32 (got %r)' % (what, T))
    if not 1 <= iters <= 16:
        raise ValueError('%s: iters must lie in [1, 16] (got %r)' % (what, iters))
    return eps, T, iters


def swav_fwd(z1, z2, C, eps, T, iters, want_codes=False):
    """SwAV forward (gca_swav_fwd; tests/swav_ref.py states the arithmetic): the (N, D) fp32 unit-row features of the two views
    and the (K, D) unit-row prototypes -> (parts = [loss, l12, l21], dS (2, N, K)[, codes (2, N, K)]), all on the device.  dS,
    8 N K bytes, is d loss / d (S_1, S_2) and all that swav_bwd needs.  ValueError for arguments the kernel entry refuses."""
    N, D, K = _swav_args(z1, z2, C, 'swav_fwd')
    eps, T, iters = swav_params('swav_fwd', eps, T, iters)
    z1, z2, C = z1.contiguous(), z2.contiguous(), C.contiguous()
    p1, p2, pc = ptr(z1), ptr(z2), ptr(C)                               # (RuntimeError for host tensors)
    dev = z1.device
    parts = torch.empty(3, dtype=F32, device=dev)
    dS = torch.empty((2, N, K), dtype=F32, device=dev)
    codes = torch.empty((2, N, K), dtype=F32, device=dev) if want_codes else None
    ws = WS.get(H.lib.gca_swav_ws_bytes(N, D, K), dev)
    H.call('gca_swav_fwd', p1, p2, pc, N, D, K, eps, T, iters, ptr(parts), ptr(dS), ptr(codes), ptr(ws), stream())
    return (parts, dS, codes) if want_codes else (parts, dS)


def swav_bwd(z1, z2, C, dS, dC, accumulate, gscale_dev=None, gscale_host=1.0):
    """d loss / d (z1, z2) of swav_fwd from its saved dS, times gscale_host * (*gscale_dev if given) -> (dz1, dz2); the
    prototypes' gradient, scaled alike, goes into dC (K, D) (added to it with `accumulate`)."""
    N, D, K = _swav_args(z1, z2, C, 'swav_bwd')
    gscale_host = float(gscale_host)
    if not -3.0e38 < gscale_host < 3.0e38:
        raise ValueError('swav_bwd: gscale_host must be finite in fp32 (got %r)' % gscale_host)
    if dS.dtype is not F32 or tuple(dS.shape) != (2, N, K):
        raise ValueError('swav_bwd: dS is the (2, %d, %d) fp32 tensor of swav_fwd (got %s %s)' % (N, K, tuple(dS.shape), dS.dtype))
    if dC.dtype is not F32 or tuple(dC.shape) != (K, D) or not dC.is_contiguous():
        raise ValueError('swav_bwd: dC is a contiguous (%d, %d) fp32 matrix (got %s %s)' % (K, D, tuple(dC.shape), dC.dtype))
    z1, z2, C, dS = (t.contiguous() for t in (z1, z2, C, dS))
    p1, p2, pc = ptr(z1), ptr(z2), ptr(C)
    dz1 = torch.empty((N, D), dtype=F32, device=z1.device)
    dz2 = torch.empty((N, D), dtype=F32, device=z1.device)
    ws = WS.get(H.lib.gca_swav_ws_bytes(N, D, K), z1.device)
    H.call('gca_swav_bwd', p1, p2, pc, ptr(dS), N, D, K, ptr(gscale_dev), gscale_host, ptr(dz1), ptr(dz2), ptr(dC),
           int(bool(accumulate)), ptr(ws), stream())
    return dz1, dz2


# ----------------------------------------------------------------------------- DINO
def dino_temperature(what, T, name='Tt'):
    """-> T as the kernels accept a temperature: positive, T and 1 / T finite in fp32; ValueError otherwise."""
    T = float(T)
    if not 1.2e-38 < T < 3.0e38:
        raise ValueError('%s: %s must be positive, %s and 1 / %s finite in fp32 (got %r)' % (what, name, name, name, T))
    return T


def dino_params(what, Ts, Tt, cm):
    """-> (Ts, Tt, cm) as gca_dino_fwd accepts them; ValueError otherwise (both temperatures positive with T and 1 / T finite
    in fp32, the centre momentum cm in [0, 1))."""
    import ctypes
    Ts, Tt, cm = dino_temperature(what, Ts, 'Ts'), dino_temperature(what, Tt, 'Tt'), float(cm)
    if not 0.0 <= ctypes.c_float(cm).value < 1.0:
        raise ValueError('%s: cm must lie in [0, 1) (got %r)' % (what, cm))
    return Ts, Tt, cm


def _dino_args(zs1, zs2, Cs, zt1, zt2, Ct, center, what):
    """Host-side refusals of gca_dino_fwd on the shapes (before any device is touched) -> (N, D, K)."""
    N, D, K = _swav_args(zs1, zs2, Cs, what)
    if _swav_args(zt1, zt2, Ct, what) != (N, D, K):
        raise ValueError('%s: the teacher operands must have the student shapes (%d, %d), (%d, %d) (got %s, %s)'
                         % (what, N, D, K, D, tuple(zt1.shape), tuple(Ct.shape)))
    if center.dtype is not F32 or tuple(center.shape) != (K,) or not center.is_contiguous():
        raise ValueError('%s: the centre is a contiguous (%d,) fp32 vector (got %s %s)' % (what, K, tuple(center.shape), center.dtype))
    return N, D, K


def dino_fwd(zs1, zs2, Cs, zt1, zt2, Ct, Ts, tt_dev, cm, center, update_center, want_probs=False, row_grid=None):
    """DINO forward (gca_dino_fwd; tests/dino_ref.py states the arithmetic): the (N, D) fp32 unit-row features of the two views
    from the student and from the teacher, the (K, D) unit-row prototypes of each, the student temperature Ts and centre
    momentum cm (host floats), the teacher temperature tt_dev (ONE fp32 on the device, checked by whoever writes it) and the
    (K,) centre, which is updated in place after the loss has used it when `update_center` -> (parts = [loss, l12, l21, ent],
    dS (2, N, K)[, probs (2, N, K)]), all on the device.  dS, 8 N K bytes, is d loss / d (Ss_1, Ss_2) and all that dino_bwd
    needs.  row_grid: None, or 0 / 1 for gca_dino_fwd_grid's workgroup / wave per row (the micro-benchmark's switch).
    ValueError for arguments the kernel entry refuses."""
    if row_grid not in (None, 0, 1):
        raise ValueError('dino_fwd: row_grid is None, 0 (workgroup per row) or 1 (wave per row) (got %r)' % (row_grid,))
    N, D, K = _dino_args(zs1, zs2, Cs, zt1, zt2, Ct, center, 'dino_fwd')
    Ts, _, cm = dino_params('dino_fwd', Ts, 1.0, cm)
    if tt_dev.dtype is not F32 or tt_dev.numel() != 1:
        raise ValueError('dino_fwd: tt_dev is one fp32 on the device (got %s %s)' % (tuple(tt_dev.shape), tt_dev.dtype))
    zs1, zs2, Cs, zt1, zt2, Ct = (t.contiguous() for t in (zs1, zs2, Cs, zt1, zt2, Ct))
    ps = [ptr(t) for t in (zs1, zs2, Cs, zt1, zt2, Ct)]                 # (RuntimeError for host tensors)
    dev = zs1.device
    parts = torch.empty(4, dtype=F32, device=dev)
    dS = torch.empty((2, N, K), dtype=F32, device=dev)
    probs = torch.empty((2, N, K), dtype=F32, device=dev) if want_probs else None
    ws = WS.get(H.lib.gca_dino_ws_bytes(N, D, K), dev)
    tail = (ptr(ws), stream())
    H.call('gca_dino_fwd' if row_grid is None else 'gca_dino_fwd_grid', *ps, N, D, K, Ts, ptr(tt_dev), cm, ptr(center),
           int(bool(update_center)), ptr(parts), ptr(dS), ptr(probs), *(tail if row_grid is None else (int(row_grid),) + tail))
    return (parts, dS, probs) if want_probs else (parts, dS)


def dino_bwd(zs1, zs2, Cs, dS, dC, accumulate, gscale_dev=None, gscale_host=1.0):
    """d loss / d (zs1, zs2) of dino_fwd from its saved dS, times gscale_host * (*gscale_dev if given) -> (dz1, dz2); the student
    prototypes' gradient, scaled alike, goes into dC (K, D) (added to it with `accumulate`).  The products are SwAV's:
    gca_swav_bwd never looks at how dS was made."""
    N, D, K = _swav_args(zs1, zs2, Cs, 'dino_bwd')
    gscale_host = float(gscale_host)
    if not -3.0e38 < gscale_host < 3.0e38:
        raise ValueError('dino_bwd: gscale_host must be finite in fp32 (got %r)' % gscale_host)
    if dS.dtype is not F32 or tuple(dS.shape) != (2, N, K):
        raise ValueError('dino_bwd: dS is the (2, %d, %d) fp32 tensor of dino_fwd (got %s %s)' % (N, K, tuple(dS.shape), dS.dtype))
    if dC.dtype is not F32 or tuple(dC.shape) != (K, D) or not dC.is_contiguous():
        raise ValueError('dino_bwd: dC is a contiguous (%d, %d) fp32 matrix (got %s %s)' % (K, D, tuple(dC.shape), dC.dtype))
    zs1, zs2, Cs, dS = (t.contiguous() for t in (zs1, zs2, Cs, dS))
    p1, p2, pc = ptr(zs1), ptr(zs2), ptr(Cs)
    dz1 = torch.empty((N, D), dtype=F32, device=zs1.device)
    dz2 = torch.empty((N, D), dtype=F32, device=zs1.device)
    ws = WS.get(H.lib.gca_swav_ws_bytes(N, D, K), zs1.device)
    H.call('gca_swav_bwd', p1, p2, pc, ptr(dS), N, D, K, ptr(gscale_dev), gscale_host, ptr(dz1), ptr(dz2), ptr(dC),
           int(bool(accumulate)), ptr(ws), stream())
    return dz1, dz2


# ----------------------------------------------------------------------------- MoCo v3
def mocov3_weight(inv_T):
    """The loss weight 2 T of Algorithm 1 as the host rounds it to fp32."""
    return float(torch.tensor(2.0 / float(inv_T), dtype=F32).item())


def _mocov3_args(q1, q2, k1, k2, inv_T, w, what):
    """Host-side refusals of gca_mocov3_fwd / _bwd (before any device is touched) -> (N, D, inv_T, w)."""
    for t in (q1, q2, k1, k2):
        if t.dim() != 2 or t.dtype is not F32 or t.shape != q1.shape:
            raise ValueError('%s: q1, q2, k1, k2 are (N, D) fp32 matrices of one shape (got %s)'
                             % (what, ', '.join('%s %s' % (tuple(u.shape), u.dtype) for u in (q1, q2, k1, k2))))
    N, D = q1.shape
    if N < 1 or N > 65536 or D < 1 or N * D >= 2 ** 31:
        raise ValueError('%s: 1 <= N <= 65536, D >= 1, N * D < 2^31 (got N=%d, D=%d)' % (what, N, D))
    inv_T = float(inv_T)
    if not 0.0 < inv_T < 3.0e38:
        raise ValueError('%s: 1 / T must be positive and finite in fp32 (got %r)' % (what, inv_T))
    w = mocov3_weight(inv_T) if w is None else float(w)
    if not 0.0 < w < 3.0e38:
        raise ValueError('%s: the loss weight must be positive and finite in fp32 (got %r)' % (what, w))
    return N, D, inv_T, w


def mocov3_fwd(q1, q2, k1, k2, inv_T, want_rank=False, w=None, want_pos=False):
    """MoCo v3's symmetrised InfoNCE forward (gca_mocov3_fwd; tests/mocov3_ref.py states the arithmetic): the (N, D) fp32 student
    rows q1, q2 and teacher rows k1, k2 of the two views -> (loss (3,): w (l_0 + l_1), l_0, l_1; lse (2 N,); rank (2, N) int32
    or None; pos_logit (2 N,) or None), all on the device; direction 0 is q1 against k2, direction 1 q2 against k1.  rank[d, i]
    counts the other columns that score at least row i's positive (top-k hit iff rank < k).  w defaults to 2 T rounded to fp32.
    ValueError for arguments the kernel entry refuses."""
    N, D, inv_T, w = _mocov3_args(q1, q2, k1, k2, inv_T, w, 'mocov3_fwd')
    q1, q2, k1, k2 = (t.contiguous() for t in (q1, q2, k1, k2))
    ps = [ptr(t) for t in (q1, q2, k1, k2)]                             # (RuntimeError for host tensors)
    dev = q1.device
    loss = torch.empty(3, dtype=F32, device=dev)
    lse = torch.empty(2 * N, dtype=F32, device=dev)
    rank = torch.empty((2, N), dtype=torch.int32, device=dev) if want_rank else None
    pos = torch.empty(2 * N, dtype=F32, device=dev) if want_pos else None
    ws = WS.get(H.lib.gca_mocov3_ws_bytes(N, D), dev)
    H.call('gca_mocov3_fwd', *ps, N, D, inv_T, w, ptr(lse), ptr(pos), ptr(rank), ptr(loss), ptr(ws), stream())
    return loss, lse, rank, pos


def mocov3_bwd(q1, q2, k1, k2, lse, inv_T, gscale_dev=None, gscale_host=1.0, w=None):
    """d loss / d (q1, q2) of mocov3_fwd from its row log-sum-exps, times gscale_host * (*gscale_dev if given) -> (dq1, dq2).
    Nothing flows to k1, k2."""
    N, D, inv_T, w = _mocov3_args(q1, q2, k1, k2, inv_T, w, 'mocov3_bwd')
    gscale_host = float(gscale_host)
    if not -3.0e38 < gscale_host < 3.0e38:
        raise ValueError('mocov3_bwd: gscale_host must be finite in fp32 (got %r)' % gscale_host)
    if lse.dtype is not F32 or tuple(lse.shape) != (2 * N,):
        raise ValueError('mocov3_bwd: lse is the (2 N,) fp32 vector of mocov3_fwd (got %s %s)' % (tuple(lse.shape), lse.dtype))
    q1, q2, k1, k2, lse = (t.contiguous() for t in (q1, q2, k1, k2, lse))
    ps = [ptr(t) for t in (q1, q2, k1, k2, lse)]
    dq1 = torch.empty((N, D), dtype=F32, device=q1.device)
    dq2 = torch.empty((N, D), dtype=F32, device=q1.device)
    ws = WS.get(H.lib.gca_mocov3_ws_bytes(N, D), q1.device)
    H.call('gca_mocov3_bwd', *ps, N, D, inv_T, w, ptr(gscale_dev), gscale_host, ptr(dq1), ptr(dq2), ptr(ws), stream())
    return dq1, dq2


# ----------------------------------------------------------------------------- NNCLR
def nnclr_weight():
    """The loss weight 1/2 of NNCLR's two directions (exact in fp32)."""
    return 0.5


def nnclr_search(z1, z2, queue):
    """Nearest support-set row of every row of both views, with the gather (gca_nnclr_search; tests/nnclr_ref.py states the
    arithmetic): z1, z2 (N, D), queue (K, D) fp32 on the device -> (idx (2, N) int32, sim (2, N) fp32, nn1 (N, D), nn2 (N, D)).
    idx[v, i] is the smallest j that attains max_j z_v[i] . queue[j] (NaN scores count as -inf; always in [0, K)), sim the
    score, nn_v[i] = queue[idx[v, i]] bit for bit.  One pass over the queue for both views, no host sync.  ValueError for
    arguments the kernel entry refuses."""
    if z1.dim() != 2 or z2.shape != z1.shape or queue.dim() != 2 or queue.shape[1] != z1.shape[1]:
        raise ValueError('nnclr_search: z1, z2 (N, D) of one shape and queue (K, D) expected (got %s, %s, %s)'
                         % (tuple(z1.shape), tuple(z2.shape), tuple(queue.shape)))
    if any(t.dtype is not F32 for t in (z1, z2, queue)):
        raise ValueError('nnclr_search: fp32 tensors expected (got %s)' % ', '.join(str(t.dtype) for t in (z1, z2, queue)))
    (N, D), K = z1.shape, queue.shape[0]
    nbytes = H.lib.gca_nnclr_search_ws_bytes(N, D, K)
    if nbytes < 0:
        raise ValueError('nnclr_search: 1 <= N <= 65536, D >= 1, 1 <= K < 2^31, N * D and K * D < 2^31 (got N=%d, D=%d, K=%d)'
                         % (N, D, K))
    z1, z2, queue = z1.contiguous(), z2.contiguous(), queue.contiguous()
    ps = [ptr(t) for t in (z1, z2, queue)]                              # (RuntimeError for host tensors)
    dev = z1.device
    idx = torch.empty((2, N), dtype=torch.int32, device=dev)
    sim = torch.empty((2, N), dtype=F32, device=dev)
    nn1 = torch.empty((N, D), dtype=F32, device=dev)
    nn2 = torch.empty((N, D), dtype=F32, device=dev)
    ws = WS.get(nbytes, dev)
    H.call('gca_nnclr_search', *ps, N, D, K, ptr(idx), ptr(sim), ptr(nn1), ptr(nn2), ptr(ws), ws.numel(), stream())
    return idx, sim, nn1, nn2


def nnclr_bwd(nn1, nn2, p1, p2, lse, inv_T, gscale_dev=None, gscale_host=1.0, w=None):
    """d loss / d (p1, p2) of mocov3_fwd(nn1, nn2, p1, p2, inv_T, w=1/2) from its row log-sum-exps (gca_nnclr_bwd: the softmax
    runs over the predictions, so the gradient goes to the column operand), times gscale_host * (*gscale_dev if given)
    -> (dp1, dp2).  Nothing flows to nn1, nn2.  w defaults to nnclr_weight()."""
    N, D, inv_T, w = _mocov3_args(nn1, nn2, p1, p2, inv_T, nnclr_weight() if w is None else w, 'nnclr_bwd')
    gscale_host = float(gscale_host)
    if not -3.0e38 < gscale_host < 3.0e38:
        raise ValueError('nnclr_bwd: gscale_host must be finite in fp32 (got %r)' % gscale_host)
    if lse.dtype is not F32 or tuple(lse.shape) != (2 * N,):
        raise ValueError('nnclr_bwd: lse is the (2 N,) fp32 vector of mocov3_fwd (got %s %s)' % (tuple(lse.shape), lse.dtype))
    nn1, nn2, p1, p2, lse = (t.contiguous() for t in (nn1, nn2, p1, p2, lse))
    ps = [ptr(t) for t in (nn1, nn2, p1, p2, lse)]
    dp1 = torch.empty((N, D), dtype=F32, device=p1.device)
    dp2 = torch.empty((N, D), dtype=F32, device=p1.device)
    ws = WS.get(H.lib.gca_nnclr_bwd_ws_bytes(N, D), p1.device)
    H.call('gca_nnclr_bwd', *ps, N, D, inv_T, w, ptr(gscale_dev), gscale_host, ptr(dp1), ptr(dp2), ptr(ws), stream())
    return dp1, dp2


# ----------------------------------------------------------------------------- ReSSL
def _ressl_args(q, k, queue, inv_Ts, inv_Tt, what):
    """Host-side refusals of gca_ressl_fwd / _bwd (before any device is touched) -> (N, D, K, inv_Ts, inv_Tt)."""
    if q.dim() != 2 or k.shape != q.shape or queue.dim() != 2 or queue.shape[1] != q.shape[1]:
        raise ValueError('%s: q, k (N, D) of one shape and queue (K, D) expected (got %s, %s, %s)'
                         % (what, tuple(q.shape), tuple(k.shape), tuple(queue.shape)))
    if any(t.dtype is not F32 for t in (q, k, queue)):
        raise ValueError('%s: fp32 tensors expected (got %s)' % (what, ', '.join(str(t.dtype) for t in (q, k, queue))))
    (N, D), K = q.shape, queue.shape[0]
    if N < 1 or N > 65536 or D < 1 or K < 1 or K >= 2 ** 31 or N * D >= 2 ** 31 or K * D >= 2 ** 31:
        raise ValueError('%s: 1 <= N <= 65536, D >= 1, 1 <= K < 2^31, N * D and K * D < 2^31 (got N=%d, D=%d, K=%d)'
                         % (what, N, D, K))
    inv_Ts, inv_Tt = float(inv_Ts), float(inv_Tt)
    for name, v in (('1 / Ts', inv_Ts), ('1 / Tt', inv_Tt)):
        if not 0.0 < v < 3.0e38:
            raise ValueError('%s: %s must be positive and finite in fp32 (got %r)' % (what, name, v))
    return N, D, K, inv_Ts, inv_Tt


def ressl_fwd(q, k, queue, inv_Ts, inv_Tt):
    """ReSSL's relational loss (gca_ressl_fwd; tests/ressl_ref.py states the arithmetic): student rows q and teacher rows k,
    (N, D) fp32, against the (K, D) queue -> (loss (2,): mean_i loss_i and the teacher's mean entropy; row_lse (2 N,): the
    log-sum-exps of q Q^T / Ts, then of k Q^T / Tt; row_loss (N,)), all on the device.  loss_i = -sum_j softmax(t_i)_j
    log softmax(s_i)_j.  One pass over the queue, nothing of size K written.  ValueError for arguments the kernel entry refuses."""
    N, D, K, inv_Ts, inv_Tt = _ressl_args(q, k, queue, inv_Ts, inv_Tt, 'ressl_fwd')
    q, k, queue = q.contiguous(), k.contiguous(), queue.contiguous()
    ps = [ptr(t) for t in (q, k, queue)]                                # (RuntimeError for host tensors)
    dev = q.device
    loss = torch.empty(2, dtype=F32, device=dev)
    row_lse = torch.empty(2 * N, dtype=F32, device=dev)
    row_loss = torch.empty(N, dtype=F32, device=dev)
    ws = WS.get(H.lib.gca_ressl_fwd_ws_bytes(N, D, K), dev)
    H.call('gca_ressl_fwd', *ps, N, D, K, inv_Ts, inv_Tt, ptr(row_lse), ptr(row_loss), ptr(loss), ptr(ws), ws.numel(), stream())
    return loss, row_lse, row_loss


def ressl_bwd(q, k, queue, row_lse, inv_Ts, inv_Tt, gscale_dev=None, gscale_host=1.0):
    """d loss / d q of ressl_fwd from its row log-sum-exps, times gscale_host * (*gscale_dev if given) -> dq (N, D):
    g / (N Ts) (softmax(s) - softmax(t)) Q.  `queue` must still be the queue ressl_fwd saw.  Nothing flows to k."""
    N, D, K, inv_Ts, inv_Tt = _ressl_args(q, k, queue, inv_Ts, inv_Tt, 'ressl_bwd')
    gscale_host = float(gscale_host)
    if not -3.0e38 < gscale_host < 3.0e38:
        raise ValueError('ressl_bwd: gscale_host must be finite in fp32 (got %r)' % gscale_host)
    if row_lse.dtype is not F32 or tuple(row_lse.shape) != (2 * N,):
        raise ValueError('ressl_bwd: row_lse is the (2 N,) fp32 vector of ressl_fwd (got %s %s)'
                         % (tuple(row_lse.shape), row_lse.dtype))
    q, k, queue, row_lse = q.contiguous(), k.contiguous(), queue.contiguous(), row_lse.contiguous()
    ps = [ptr(t) for t in (q, k, queue, row_lse)]
    dq = torch.empty((N, D), dtype=F32, device=q.device)
    ws = WS.get(H.lib.gca_ressl_bwd_ws_bytes(N, D, K), q.device)
    H.call('gca_ressl_bwd', *ps, N, D, K, inv_Ts, inv_Tt, ptr(gscale_dev), gscale_host, ptr(dq), ptr(ws), ws.numel(), stream())
    return dq


# ----------------------------------------------------------------------------- class head
def _classifier_args(x, w, bias, target, what):
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1]:
        raise ValueError('%s: x (b, F) and w (C, F) must share F (got %s, %s)' % (what, tuple(x.shape), tuple(w.shape)))
    if bias is not None and tuple(bias.shape) != (w.shape[0],):
        raise ValueError('%s: bias must be (C,)' % what)
    if target is not None and (target.dtype is not torch.int64 or tuple(target.shape) != (x.shape[0],)):
        raise ValueError('%s: target is an int64 vector, one label per row' % what)
    b, Fd = x.shape
    nbytes = H.lib.gca_classifier_ws_bytes(b, Fd, w.shape[0])
    if nbytes < 0:
        raise ValueError('%s: invalid sizes (b=%d, F=%d, C=%d)' % (what, b, Fd, w.shape[0]))
    return b, Fd, w.shape[0], nbytes


def classifier_fwd(x, w, bias=None, target=None, want_lse=False, want_rank=True, want_loss=True):
    """Linear class head fused with softmax cross-entropy (gca_classifier_fwd; tests/classify_ref.py states the arithmetic).
    x (b, F), w (C, F), bias (C) or None, fp32 on the device.  Without `target`: -> logits (b, C), or (logits, row_lse) with
    want_lse (the eval path).  With int64 `target` (b,): -> (logits, row_lse, rank_ge | None, loss (1,) | None).  The labels
    are NOT range-checked here (that needs their host copy: engine.layers.f_classifier's callers do it)."""
    b, Fd, Cc, nbytes = _classifier_args(x, w, bias, target, 'classifier_fwd')
    x, w = x.contiguous(), w.contiguous()
    dev = x.device
    logits = torch.empty((b, Cc), dtype=F32, device=dev)
    train = target is not None
    lse = torch.empty(b, dtype=F32, device=dev) if (train or want_lse) else None
    rank = torch.empty(b, dtype=torch.int32, device=dev) if (train and want_rank) else None
    loss = torch.empty(1, dtype=F32, device=dev) if (train and want_loss) else None
    ws = WS.get(nbytes, dev)
    H.call('gca_classifier_fwd', ptr(x), ptr(w), ptr(bias), ptr(target), b, Fd, Cc, ptr(logits), ptr(lse), ptr(rank), ptr(loss),
           ptr(ws), nbytes, stream())
    if train:
        return logits, lse, rank, loss
    return (logits, lse) if want_lse else logits


def cross_entropy_fwd(logits, target):
    """Row statistics and mean cross-entropy of existing (b, C) logits: gca_classifier_fwd without its product (x = w =
    NULL).  -> (row_lse (b,), rank_ge (b,), loss (1,))."""
    if logits.dim() != 2 or target.dtype is not torch.int64 or tuple(target.shape) != (logits.shape[0],):
        raise ValueError('cross_entropy_fwd: (b, C) logits and int64 labels (b,)')
    b, Cc = logits.shape
    nbytes = H.lib.gca_classifier_ws_bytes(b, 1, Cc)
    if nbytes < 0 or b == 0:
        raise ValueError('cross_entropy_fwd: invalid sizes (b=%d, C=%d)' % (b, Cc))
    logits = logits.contiguous()
    dev = logits.device
    lse, rank = torch.empty(b, dtype=F32, device=dev), torch.empty(b, dtype=torch.int32, device=dev)
    loss = torch.empty(1, dtype=F32, device=dev)
    ws = WS.get(nbytes, dev)
    H.call('gca_classifier_fwd', None, None, None, ptr(target), b, 1, Cc, ptr(logits), ptr(lse), ptr(rank), ptr(loss), ptr(ws),
           nbytes, stream())
    return lse, rank, loss


def classifier_bwd(x, w, logits, lse, target, dw, dbias=None, accumulate=True, dx=None, dx_accumulate=False, gscale_dev=None,
                   gscale_host=1.0):
    """d loss / d (w, bias, x) of classifier_fwd's mean cross-entropy times gscale_host * (*gscale_dev), the softmax gradient
    formed on the fly (gca_classifier_bwd).  dw (C, F) and dbias (C) are written, or added to with `accumulate`; dx (b, F)
    likewise with `dx_accumulate`, and dx=None skips that product altogether."""
    b, Fd, Cc, nbytes = _classifier_args(x, w, dbias, target, 'classifier_bwd')
    if tuple(logits.shape) != (b, Cc) or tuple(lse.shape) != (b,) or tuple(dw.shape) != (Cc, Fd) or target is None:
        raise ValueError('classifier_bwd: logits (b, C), row_lse (b,), target (b,) and dw (C, F) are required')
    if dx is not None and tuple(dx.shape) != (b, Fd):
        raise ValueError('classifier_bwd: dx must be (b, F)')
    for t in (logits, lse, dw, dbias, dx):
        if t is not None and not t.is_contiguous():
            raise ValueError('classifier_bwd: buffers must be contiguous')
    x, w = x.contiguous(), w.contiguous()
    ws = WS.get(nbytes, x.device)
    H.call('gca_classifier_bwd', ptr(x), ptr(w), ptr(logits), ptr(lse), ptr(target), ptr(gscale_dev), float(gscale_host), b, Fd, Cc,
           ptr(dw), ptr(dbias), int(bool(accumulate)), ptr(dx), int(bool(dx_accumulate)), ptr(ws), nbytes, stream())


# ----------------------------------------------------------------------------- graph block
def graph_adj_fwd(gq, gk, u, max_hop, alpha, temperature):
    B, Ci, T = gq.shape[0], gq.shape[1], gq.shape[2]
    HW = gq.shape[3] * gq.shape[4]
    out = torch.empty((3, B, T, T), dtype=F32, device=gq.device)
    ws = WS.get(H.lib.gca_graph_gram_ws_bytes(B, Ci, T, HW), gq.device)
    H.call('gca_graph_adj_fwd', ptr(gq), ptr(gk), B, Ci, T, HW, int(max_hop), float(alpha), float(temperature), ptr(u),
           ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(ws), stream())
    return out[0], out[1], out[2]          # sim, adj_pre, adj


def graph_adj_bwd(dadj, gq, gk, sim, pre, adj, max_hop, alpha, temperature):
    B, Ci, T = gq.shape[0], gq.shape[1], gq.shape[2]
    HW = gq.shape[3] * gq.shape[4]
    dgq, dgk = torch.empty_like(gq), torch.empty_like(gk)
    H.call('gca_graph_adj_bwd', ptr(dadj), ptr(gq), ptr(gk), ptr(sim), ptr(pre), ptr(adj), B, Ci, T, HW, int(max_hop),
           float(alpha), float(temperature), ptr(dgq), ptr(dgk), stream())
    return dgq, dgk


def graph_gcn_fwd(adj, s, out=None):
    B, Cc, T = s.shape[0], s.shape[1], s.shape[2]
    if out is None:
        out = torch.empty_like(s)
    H.call('gca_graph_gcn_fwd', ptr(adj), ptr(s), B, Cc, T, s.shape[3] * s.shape[4], ptr(out), stream())
    return out


def graph_gcn_bwd(adj, s, dout, want_dadj=True):
    B, Cc, T = s.shape[0], s.shape[1], s.shape[2]
    ds = torch.empty_like(s)
    dadj = torch.empty((B, T, T), dtype=F32, device=s.device) if want_dadj else None
    ws = WS.get(H.lib.gca_graph_gcn_bwd_ws_bytes(B, Cc, T, s.shape[3] * s.shape[4]), s.device) if want_dadj else None
    H.call('gca_graph_gcn_bwd', ptr(adj), ptr(s), ptr(dout), B, Cc, T, s.shape[3] * s.shape[4], ptr(ds), ptr(dadj),
           ptr(ws), stream())
    return ds, dadj


# ----------------------------------------------------------------------------- flat-arena updates
def ema_update(p_ema, p, m):
    H.call('gca_ema_update', ptr(p_ema), ptr(p), p.numel(), float(m), stream())


def ema_update_dev(p_ema, p, m_dev):
    """ema_update with the momentum read from `m_dev`, ONE fp32 on the device (gca_ema_update_dev): a captured step follows
    a momentum schedule.  p_ema and p are contiguous fp32 of one size, any length >= 1."""
    if p_ema.dtype is not F32 or p.dtype is not F32 or p_ema.numel() != p.numel() or p.numel() < 1:
        raise ValueError('ema_update_dev: p_ema and p are fp32 tensors of one size >= 1 (got %s %s, %s %s)'
                         % (tuple(p_ema.shape), p_ema.dtype, tuple(p.shape), p.dtype))
    if not (p_ema.is_contiguous() and p.is_contiguous()):
        raise ValueError('ema_update_dev: p_ema and p must be contiguous')
    if m_dev.dtype is not F32 or m_dev.numel() != 1:
        raise ValueError('ema_update_dev: m_dev is one fp32 on the device (got %s %s)' % (tuple(m_dev.shape), m_dev.dtype))
    H.call('gca_ema_update_dev', ptr(p_ema), ptr(p), p.numel(), ptr(m_dev), stream())


def sgd_step(p, g, buf, chunk_lr, chunk_wd, lr_scale, momentum, nesterov, grad_clip=None):
    """grad_clip: the (norm, coef) pair of grad_clip_coef -- gradients are scaled by coef inside the update."""
    H.call('gca_sgd_step', ptr(p), ptr(g), ptr(buf), p.numel(), ptr(chunk_lr), ptr(chunk_wd), float(lr_scale),
           float(momentum), int(nesterov), 0, ptr(grad_clip), stream())


def adam_step(p, g, exp_avg, exp_avg_sq, chunk_lr, chunk_wd, beta1, beta2, eps, decoupled, state, grad_clip=None):
    """One Adam (decoupled False) / AdamW (True) step over the arena, then the step count `state` (one int64 on the device,
    steps taken so far) is advanced by a launch of its own; a set skip flag in `grad_clip` leaves all of it untouched."""
    if state.dtype is not torch.int64 or state.numel() != 1:
        raise TypeError('the Adam step count is one int64 on the device')
    H.call('gca_adam_step', ptr(p), ptr(g), ptr(exp_avg), ptr(exp_avg_sq), p.numel(), ptr(chunk_lr), ptr(chunk_wd),
           float(beta1), float(beta2), float(eps), int(bool(decoupled)), ptr(grad_clip), ptr(state), stream())
    H.call('gca_adam_advance', ptr(state), ptr(grad_clip), stream())


def lars_job_tables(offsets, sizes, total, job_chunks=None):
    """Host arithmetic of the LARS norm pass: cut every tensor of an arena (element offsets / sizes, each padded to whole
    256-element chunks, `total` elements in all) into jobs of at most `job_chunks` chunks that never cross a tensor.
    -> (jobs int32 (n_jobs, 3): tensor, first chunk, chunk count;  params int32 (n_params, 4): first job, job count, first
    chunk, chunk count), as gca_lars_step reads them."""
    J = int(job_chunks or H.lib.gca_lars_job_chunks())
    jobs, params = [], []
    for i, (o, s) in enumerate(zip(offsets, sizes)):
        if o % 256 or s <= 0:
            raise ValueError('tensor %d: offset %d, %d elements -- not an arena layout' % (i, o, s))
        c0, nc = o // 256, (s + 255) // 256
        if (c0 + nc) * 256 > total or (params and c0 < params[-1][2] + params[-1][3]):
            raise ValueError('tensor %d lies outside the arena or over its predecessor' % i)
        params.append((len(jobs), (nc + J - 1) // J, c0, nc))
        jobs.extend((i, c, min(J, c0 + nc - c)) for c in range(c0, c0 + nc, J))
    return torch.tensor(jobs, dtype=torch.int32).reshape(-1, 3), torch.tensor(params, dtype=torch.int32).reshape(-1, 4)


class LarsPlan:
    """Everything gca_lars_step needs beyond the SGD operands, allocated once per arena (nothing is sized or uploaded at step
    time, so the step can be captured): the job tables, the fp64 partial sums, and the results -- `norms` (n_params, 2) fp64
    (|w|, |g|), `trust` (n_params,) fp32 and its per-chunk copy.  `adapt` (n_params,) int32 is the caller's to fill."""

    def __init__(self, offsets, sizes, total, device):
        jobs, params = lars_job_tables(offsets, sizes, total)
        self.total, self.n_jobs, self.n_params = int(total), jobs.shape[0], params.shape[0]
        self.jobs, self.params = jobs.to(device), params.to(device)
        self.adapt = torch.zeros(self.n_params, dtype=torch.int32, device=device)
        self.partials = torch.zeros(self.n_jobs, 2, dtype=torch.float64, device=device)
        self.norms = torch.zeros(self.n_params, 2, dtype=torch.float64, device=device)
        self.trust = torch.ones(self.n_params, dtype=F32, device=device)
        self.chunk_trust = torch.ones(self.total // 256, dtype=F32, device=device)


def _f64ptr(t, like):
    """Device pointer of one of a LarsPlan's fp64 records (ptr() is for the fp32 / integer operands)."""
    if t.dtype is not torch.float64 or t.device != like.device or not t.is_contiguous():
        raise TypeError('a contiguous fp64 tensor on %s expected' % like.device)
    return t.data_ptr()


def lars_step(p, g, buf, chunk_lr, chunk_wd, plan, momentum, nesterov, trust_coef, eps, grad_clip=None):
    """One LARS step over the arena (three launches: per-job sums of squares, per-tensor trust ratio, update); `plan` is the
    arena's LarsPlan, whose norms / trust it overwrites.  A set skip flag in `grad_clip` leaves all of it untouched."""
    n = p.numel()
    if plan.total != n or g.numel() != n or buf.numel() != n or chunk_lr.numel() != n // 256 or chunk_wd.numel() != n // 256:
        raise ValueError('operands and LarsPlan describe arenas of different sizes')
    H.call('gca_lars_step', ptr(p), ptr(g), ptr(buf), n, ptr(chunk_lr), ptr(chunk_wd), ptr(plan.jobs), plan.n_jobs,
           ptr(plan.params), ptr(plan.adapt), plan.n_params, _f64ptr(plan.partials, p), _f64ptr(plan.norms, p), ptr(plan.trust),
           ptr(plan.chunk_trust), float(momentum), int(bool(nesterov)), float(trust_coef), float(eps), ptr(grad_clip), stream())


def grad_clip_coef(g, max_norm, out=None):
    """clip_grad_norm_ over the flat gradient arena -> device tensor (total_norm, clip coefficient, 0, 0)."""
    if out is None:
        out = torch.empty(4, dtype=F32, device=g.device)
    ws = WS.get(H.lib.gca_grad_clip_ws_bytes(), g.device)
    H.call('gca_grad_clip_coef', ptr(g), g.numel(), float(max_norm), ptr(out), ptr(ws), stream())
    return out


# Dynamic loss scaling of the fp16-storage path (apex amp's LossScaler defaults: x2 after 2000 clean steps, x0.5 and a
# skipped optimizer step on inf / nan, scale capped at 2^24), kept on the device: see gca_grad_unscale_clip.
LOSS_SCALE_GROWTH, LOSS_SCALE_BACKOFF, LOSS_SCALE_INTERVAL, LOSS_SCALE_MAX = 2.0, 0.5, 2000, 2.0 ** 24
# The (scale, clean steps, skipped steps, steps) state of the trainer that is running its step, or None for fp32 storage:
# loss-gradient seeds inside the models (SimSiam's negative cosine) multiply by its first element.
LOSS_SCALE_STATE = [None]


def loss_scale_state(initial, device):
    return torch.tensor([float(initial), 0.0, 0.0, 0.0], dtype=F32, device=device)


def grad_unscale_clip(g, state, max_norm=None, out=None):
    """Un-scale (by the device-resident loss scale in `state`), overflow-check and clip the flat gradient arena without
    touching it: -> device tensor (norm of g / S, factor for the SGD kernel, skip flag, S); `state` is advanced."""
    if out is None:
        out = torch.empty(4, dtype=F32, device=g.device)
    ws = WS.get(H.lib.gca_grad_clip_ws_bytes(), g.device)
    H.call('gca_grad_unscale_clip', ptr(g), g.numel(), float(max_norm or 0.0), ptr(state), LOSS_SCALE_GROWTH,
           LOSS_SCALE_BACKOFF, int(LOSS_SCALE_INTERVAL), LOSS_SCALE_MAX, ptr(out), ptr(ws), stream())
    return out


def scale_dev_(y, a_dev, a_host=1.0):
    """y *= a_dev[0] * a_host (a device-resident factor: the loss scale)."""
    H.call('gca_scale_dev', ptr(y), y.numel(), ptr(a_dev), float(a_host), stream())


def fill(t, v):
    H.call('gca_fill', ptr(t), t.numel(), float(v), stream())


def axpy(y, x, a=1.0):
    if is_half(y, x):
        H.call('gca_axpy_f16', aptr(y), aptr(x), y.numel(), float(a), stream())
    else:
        H.call('gca_axpy', ptr(y), ptr(x), y.numel(), float(a), stream())


def scale_(y, a):
    H.call('gca_scale', ptr(y), y.numel(), float(a), stream())


def gather_rows(src, idx):
    """dst[r] = src[idx[r]] over dim 0.  src may be a batch-strided view (each row itself contiguous)."""
    rows = idx.numel()
    re = src[0].numel()
    if not src[0].is_contiguous() or idx.dtype != torch.long:
        raise ValueError('gather_rows: rows must be contiguous, idx int64')
    dst = torch.empty((rows,) + tuple(src.shape[1:]), dtype=F32, device=src.device)
    H.call('gca_gather_rows', ptr(src), ptr(idx), rows, re, src.stride(0) if src.shape[0] > 1 else re, ptr(dst), stream())
    return dst
