"""Pre-training step drivers (MoCo, SimSiam, SimCLR, Barlow Twins, VICReg, SwAV, DINO, MoCo v3 and NNCLR) on the HIP engine.

Restates the iteration of tools/train_video_contrast_dis.py:395-454 (_train_moco) and :479-523
(_train_simsiam) without its host syncs (3x .item() per iteration, :429-431) and defects
(SURVEY.md fact 7).  One iteration =

    key encoder fwd (no grad, BN in train mode)      ShuffleBN exchange / negatives all-gather (N>1)
    query encoder fwd                                InfoNCE: logits GEMM + LSE + loss + top-k rank
    enqueue keys -> queue                            dq -> encoder backward (tape)
    gradient all-reduce (N>1) -> fused SGD           fused EMA of the key encoder

Everything between the collectives is a fixed kernel sequence, so it is captured into hipGraphs
(one for N=1; three segments around the collectives for N>1) and replayed per step.
"""
import atexit
import math
import os
import weakref

import torch

from . import layers as L
from . import ops
from .arena import arena_of
from .input import ActionInputStage, StagedBatch
from .layers import BatchedPacker
from .tape import Tape, Var
from .. import parallel as par
from ..lib.memory import create_contrast, create_criterion
from ..lib.evaluation.metric import accuracy_from_rank
from ..lib.evaluation.retrieval import encoder_state_dict
from ..lib.modeling import create_video_model, create_visual_model
from ..lib.solver import make_lr_scheduler, make_optimizer
from ..lib.solver.build import check_optimizer_name, clip_value_of
from ..lib.utils import creat_criterion


def set_key_encoder_mode(model_ema):
    """eval() but every BatchNorm stays in train mode (tools/...dis.py:383-389)."""
    model_ema.eval()
    for m in model_ema.modules():
        if m.__class__.__name__.find('BatchNorm') != -1:
            m.train()


# Every live _Graphed, weakly: captured hipGraphs must be destroyed while the HIP runtime is still up.  A graph that is
# only released by interpreter shutdown (a trainer held at module scope, the INTEGRATION.md usage) is torn down after the
# runtime and aborts the process, so the package itself resets whatever is still alive from an atexit hook -- registered at
# import, i.e. after torch's own hooks, and atexit runs last-registered first.
_LIVE_GRAPHS = weakref.WeakSet()


def release_all_graphs():
    """Destroy every captured hipGraph of this process (idempotent).  Runs at interpreter exit; callable by hand."""
    live = list(_LIVE_GRAPHS)
    for g in live:
        g.release()
    if live and torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError:
            pass


atexit.register(release_all_graphs)


class _Graphed(object):
    """Capture-once / replay wrapper for a no-argument closure working on static buffers."""

    def __init__(self, fn, enabled, pool=None):
        self.fn, self.enabled, self.graph, self.warm, self.pool = fn, enabled, None, 0, pool
        _LIVE_GRAPHS.add(self)

    def release(self):
        """Drop the captured graph (the next run() re-captures after its eager warm-up)."""
        g, self.graph, self.warm = self.graph, None, 0
        if g is not None:
            torch.cuda.synchronize()
            g.reset()

    def run(self):
        if not self.enabled:
            return self.fn()
        if self.graph is None:
            if self.warm < 2:               # eager warm-up: builds plans/tables/workspaces, warms allocator
                self.warm += 1
                return self.fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            # with a process group alive, its watchdog thread polls events while we capture: only THIS thread's
            # calls must be checked against the capture (the default "global" mode would fail the capture)
            mode = 'thread_local' if torch.distributed.is_available() and torch.distributed.is_initialized() else 'global'
            with torch.cuda.graph(g, pool=self.pool, capture_error_mode=mode):    # records the launches, does not execute them
                self.fn()
            self.graph = g
        self.graph.replay()


def _check_unsupported(cfg):
    """Options the reference's trainer honours and this one does not must fail loudly, not train differently."""
    apex = getattr(cfg, 'APEX', None)
    if apex is not None and bool(getattr(apex, 'FLAG', False)):
        raise NotImplementedError('APEX.FLAG (apex amp, tools/train_video_contrast_dis.py:134-141) is not available: '
                                  'select the reduced-precision conv path with engine.ops.set_conv_math instead')


# GCA_FORK_KEY=0: key and query encoders on one stream inside the captured step as well (A/B runs)
FORK_KEY_ENCODER = os.environ.get('GCA_FORK_KEY', '1') != '0'
# gradient all-reduce bucket: 8 M fp32 = 32 MB (four buckets for R(2+1)D-18 + head); 0 = one all-reduce after the backward pass
BUCKET_ELEMS = int(os.environ.get('GCA_BUCKET_ELEMS', 8 << 20))


class _ShapeOnly(object):
    """Stand-in for the fp32 batch a StagedBatch will become (shape / device bookkeeping of _ensure_static)."""

    def __init__(self, shape, device):
        self.shape, self.device, self.dtype = torch.Size(shape), device, torch.float32


# GCA_DEFER_REDUCE=0: every weight gradient reduces its split-K slabs in its own launch (A/B runs)
DEFER_REDUCE = os.environ.get('GCA_DEFER_REDUCE', '1') != '0'


class _TrainerBase(object):
    def _backward(self, tape, upto):
        """Tape.backward with the weight-gradient split-K reductions of the stage collected into one launch."""
        if not DEFER_REDUCE:
            return tape.backward(upto)
        if getattr(self, '_deferred', None) is None:
            self._deferred = ops.DeferredReduce()
        if ops.DEFER[0] is not None:
            raise RuntimeError('another backward pass is collecting weight-gradient reductions')
        ops.DEFER[0] = self._deferred
        try:
            tape.backward(upto)
        finally:
            ops.DEFER[0] = None
            # a pass that raised part-way leaves queued (slab, dw, +=) jobs behind: the next step must not fold them in
            self._deferred.pending.clear()

    def _buckets_from_log(self, arena, log):
        """log: (backward closure index, parameter) pairs of one eager backward pass (engine.layers.GRAD_LOG).  Cuts the
        arena into buckets that a reverse sweep of the tape completes one after the other (parallel.plan_buckets)."""
        first = {}
        for idx, prm in log:
            if idx >= 0:
                first[id(prm)] = min(first.get(id(prm), idx), idx)
        fc = [first.get(id(prm)) for prm in arena.params]
        return par.plan_buckets(fc, arena.offsets, arena.sizes, arena.total, int(getattr(self, 'bucket_elems', BUCKET_ELEMS)))

    def close(self):
        """Release the captured hipGraphs now (they are re-captured if train_step is called again)."""
        for g in (self._segments or []):
            g.release()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _loss_scale():
    """INITIAL loss scale of the fp16-storage path (a power of two: scaling and un-scaling are exact in fp32; the
    activation gradients, stored fp16, stay clear of the subnormal range).  From there the scale is dynamic, as apex amp's
    is in the reference (tools/train_video_contrast_dis.py:134-141,413-418): a step whose gradients hold an inf / nan is
    skipped and halves it, 2000 clean steps double it -- all decided on the device (ops.grad_unscale_clip).  None for
    fp32 storage."""
    if not ops.ACT_F16[0]:
        return None
    s = float(os.environ.get('GCA_LOSS_SCALE', '1024'))
    if s <= 0 or math.frexp(s)[0] != 0.5:
        raise ValueError('GCA_LOSS_SCALE must be a positive power of two, got %r' % s)
    return s


class MoCoTrainer(_TrainerBase):
    def __init__(self, cfg, device, ctx=None, use_graph=True, seed=None):
        _check_unsupported(cfg)
        self.cfg, self.device = cfg, torch.device(device)
        self.clip = clip_value_of(cfg)
        self.ctx = ctx or par.DistCtx()
        ls = _loss_scale()
        # fp16 storage: (scale, clean steps in a row, skipped steps, steps) on the device; None for fp32 storage
        self.scale_state = None if ls is None else ops.loss_scale_state(ls, torch.device(device))
        self.loss_scale = 1.0 if ls is None else ls           # the INITIAL scale (the live one is scale_state[0], on the device)
        if seed is not None:
            torch.manual_seed(seed)
        self.model, self.model_ema = create_visual_model(cfg)
        self.model.to(self.device)
        self.model_ema.to(self.device)
        self.arena_q, self.arena_k = arena_of(self.model), arena_of(self.model_ema)
        if self.arena_q.total != self.arena_k.total:
            raise RuntimeError('query / key encoders must share one parameter layout')
        par.broadcast_(self.arena_q.flat, self.ctx)
        self.arena_k.flat.copy_(self.arena_q.flat)                       # _momentum_update(m=0), :146
        self.contrast = create_contrast(cfg, 0).to(self.device)
        par.broadcast_(self.contrast.memory, self.ctx)                    # _broadcast_memory, :121
        self.criterion = create_criterion(cfg, 0)
        self.optimizer = make_optimizer(cfg, self.model)
        self.scheduler = make_lr_scheduler(cfg, self.optimizer)
        self.model.train()
        set_key_encoder_mode(self.model_ema)
        self.alpha = float(cfg.CONTRAST.ALPHA)
        self.inv_T = 1.0 / float(cfg.CONTRAST.NCE_T)
        self.K = int(cfg.CONTRAST.NCE_K)
        self.ptr_dev = torch.zeros(1, dtype=torch.long, device=self.device)
        self.use_graph = bool(use_graph)
        self.step_count = 0
        self.perm_seed = int(getattr(cfg.MODEL, 'SEED', 1))
        self._static = None
        self._segments = None
        self._packers = None        # built after the first (eager) step, when every layer has its plan
        self._buckets = None        # N > 1: [(closure index, lo, hi)] gradient buckets in completion order
        self._tape = None
        self._planned = False
        self._plans = None          # N > 1: look-ahead ShuffleBN exchange plans (parallel.ExchangePlans)
        self._reducer = par.BucketReducer(self.arena_q.grad, self.ctx)
        self._side = None           # second stream of the captured step (key encoder forward)
        self._fwd = None            # N > 1: (tape, query feature) between the forward segment and the rest
        self.out = {}

    # -------------------------------------------------------------------------------- buffers
    def _ensure_static(self, images):
        b = images.shape[0]
        if self._static is None or self._static['images'].shape != images.shape:
            W = self.ctx.world
            D = int(self.cfg.CROSS.FEAT_DIM)
            self._static = dict(
                images=torch.empty(tuple(images.shape), dtype=torch.float32, device=self.device),
                key_in=torch.empty((b,) + (3,) + tuple(images.shape[2:]), dtype=torch.float32, device=self.device)
                if self.ctx.active else None,
                k_shuf=torch.empty((b, D), dtype=torch.float32, device=self.device),
                k=torch.empty((b, D), dtype=torch.float32, device=self.device),
                all_k=torch.empty((b * W, D), dtype=torch.float32, device=self.device),
                enq_idx=torch.empty(b, dtype=torch.long, device=self.device))
            self._segments = None
            self._packers = None
        return self._static

    def _pack(self, which):
        """Refresh the packed weights of a whole encoder in one launch (layers skip their own packing)."""
        if self._packers is not None:
            self._packers[which].run()

    def _unpack(self, which):
        if self._packers is not None:
            self._packers[which].release()

    # -------------------------------------------------------------------------------- phases
    def _phase_key(self):
        """k (shuffled order on N>1) = key_encoder(key_in); no tape, BN train mode."""
        s = self._static
        x2 = s['key_in'] if self.ctx.active else torch.chunk(s['images'], 2, dim=1)[1]
        self._pack('k')
        kv = self.model_ema.fwd(Tape(False), Var(x2))
        self._unpack('k')
        s['k_shuf'].copy_(kv.t)

    def _phase_query_fwd(self):
        """Query encoder forward (needs nothing from the key encoder)."""
        s = self._static
        self.optimizer.zero_grad()
        self._pack('q')
        tape = Tape(True)
        qv = self.model.fwd(tape, Var(torch.chunk(s['images'], 2, dim=1)[0]))
        return tape, qv

    def _phase_query_rest(self, tape, qv, upto=0):
        """InfoNCE, enqueue, dq and the backward pass down to tape index `upto` (0 = all of it; N > 1 runs the rest in stages,
        one per gradient bucket: _phase_backward_stage)."""
        s = self._static
        mem = self.contrast.memory
        logits, lse, rank, loss = ops.moco_logits_fwd(qv.t, s['k'], mem, self.inv_T, want_lse=True, want_rank=True,
                                                      want_loss=True)
        saved = ops.queue_enqueue(mem, s['all_k'], 0, save=True, ptr_dev=self.ptr_dev)
        # DDP averages gradients: fold 1/world into the loss-gradient scale
        qv.grad = ops.moco_logits_bwd(s['k'], mem, self.inv_T, logits=logits, lse=lse,
                                      gscale_dev=self.scale_state, gscale_host=1.0 / self.ctx.world, ov_rows=saved,
                                      ov_start_dev=self.ptr_dev)
        ops.queue_advance(self.ptr_dev, s['all_k'].shape[0], self.K)
        self.out = dict(loss=loss, logits=logits, rank=rank, q=qv.t)
        self._backward(tape, upto)
        self._tape = tape if upto > 0 else None
        if upto == 0:
            self._unpack('q')

    def _phase_backward_stage(self, upto, last):
        self._backward(self._tape, upto)
        if last:
            self._tape = None
            self._unpack('q')

    def _phase_update(self):
        clip = None
        if self.scale_state is not None:
            # fp16 storage: the gradients were computed x S.  One pass over the arena yields the un-scaled norm, the factor
            # (clip coefficient / S) the SGD kernel applies on the fly and the overflow verdict: inf / nan anywhere -> the
            # optimizer step is skipped (parameters and momentum untouched) and S is halved, as amp does.  The EMA below
            # still runs: the reference's _momentum_update is its own call, which amp does not patch (:440).
            clip = ops.grad_unscale_clip(self.arena_q.grad, self.scale_state, self.clip)
            self.out['grad_norm'] = clip
            self.out['loss_scale'] = self.scale_state
        elif self.clip is not None:                                           # :420-423, after the gradient all-reduce
            clip = self.optimizer.clip_grad_norm(self.clip)
            self.out['grad_norm'] = clip
        self.optimizer.step(grad_clip=clip)
        ops.ema_update(self.arena_k.flat, self.arena_q.flat, self.alpha)      # :440

    def _key_and_query_fwd(self):
        """Key encoder forward and query encoder forward (they share nothing until InfoNCE).  Inside a captured hipGraph the
        key encoder runs on a SECOND stream next to the query encoder: the latency-bound kernels of the deep, small layers
        of one fill the CUs the other leaves idle (measured +5 % on the whole step at N = 1).  Eager runs keep one stream (the
        launch tuner times kernels there) but already use the key lane's own scratch buffer, so nothing grows during the
        capture.  -> (tape, query feature Var)"""
        fork = FORK_KEY_ENCODER and torch.cuda.is_current_stream_capturing()
        ops.WS_LANE[0] = 1
        try:
            if fork:
                cur = torch.cuda.current_stream()
                if self._side is None:
                    self._side = torch.cuda.Stream(device=self.device)
                self._side.wait_stream(cur)
                with torch.cuda.stream(self._side):
                    self._phase_key()
            else:
                self._phase_key()
        finally:
            ops.WS_LANE[0] = 0
        tape, qv = self._phase_query_fwd()
        if fork:
            cur.wait_stream(self._side)
        return tape, qv

    def _single_gpu_all(self):
        s = self._static
        tape, qv = self._key_and_query_fwd()
        # N=1: BN batch statistics are permutation invariant, so the clips are NOT physically shuffled;
        # only the enqueue order (all_k = k in shuffled order, :222) is reproduced.
        s['k'].copy_(s['k_shuf'])
        s['all_k'].copy_(ops.gather_rows(s['k_shuf'], s['enq_idx']))
        self._phase_query_rest(tape, qv, 0)
        self._phase_update()

    def _phase_fwd_pair(self):
        """N > 1, first segment: both encoder forwards; the tape lives on until the next segment (after the key gather)."""
        self._fwd = self._key_and_query_fwd()

    def _phase_rest(self, upto):
        (tape, qv), self._fwd = self._fwd, None
        self._phase_query_rest(tape, qv, upto)

    # -------------------------------------------------------------------------------- step
    def train_step(self, images, shuffle_ids=None):
        """images: (b, 6, T, H, W) fp32 on the device, or a StagedBatch of engine.input.DeviceInputStage (uint8 frames on
        their way to the device: the crop / flip / normalise / layout pass then writes the static batch directly).
        Returns dict(loss, logits, rank, q) of device tensors (no host sync).  shuffle_ids: optional host int64 permutation
        of the node batch."""
        staged = images if isinstance(images, StagedBatch) else None
        if staged is not None:
            images = _ShapeOnly(staged.stage.out_shape(), self.device)
        elif images.device != self.device or images.dtype != torch.float32:
            raise RuntimeError('train_step needs fp32 clips already resident on %s (or a StagedBatch)' % self.device)
        s = self._ensure_static(images)
        b, W = images.shape[0], self.ctx.world
        user_ids = shuffle_ids
        if shuffle_ids is None and not self.ctx.active:
            shuffle_ids = par.shared_permutation(b * W, self.perm_seed, self.step_count)
        if staged is not None:
            staged.stage.prepare(staged, s['images'])
        else:
            s['images'].copy_(images)
        self.optimizer._sync_tables()
        if not self.ctx.active:
            s['enq_idx'].copy_(shuffle_ids)
            if self._segments is None:
                self._segments = [_Graphed(self._single_gpu_all, self.use_graph)]
            self._segments[0].run()
        else:
            if self._plans is None or self._plans.b != b:
                self._plans = par.ExchangePlans(b, self.ctx, self.perm_seed, self.device)
            plan = self._plans.get(self.step_count, user_ids)
            if self._segments is None:
                # One graph segment per stage: key forward || query forward (two streams) | InfoNCE + backward down to the first bucket
                # boundary | one backward stage per further gradient bucket | update.  The all-reduce of a bucket is
                # issued behind the segment that completes it and runs on RCCL's stream while the next stage computes
                # (DDP's overlap, tools/train_video_contrast_dis.py:143,419, with a few 32 MB buckets).  Activations
                # allocated while one segment is captured are read by the next: the segments share one graph memory pool.
                pool = torch.cuda.graph_pool_handle() if self.use_graph else None
                if self._buckets is None:
                    self._buckets = [(0, 0, self.arena_q.total)]         # first step: un-staged; planned below
                bk = self._buckets
                last = len(bk) - 1
                segs = [_Graphed(self._phase_fwd_pair, self.use_graph, pool),
                        _Graphed(lambda u=(0 if last == 0 else bk[0][0]): self._phase_rest(u), self.use_graph, pool)]
                for i in range(1, len(bk)):
                    segs.append(_Graphed(lambda u=(0 if i == last else bk[i][0]), l=(i == last): self._phase_backward_stage(u, l),
                                         self.use_graph, pool))
                segs.append(_Graphed(self._phase_update, self.use_graph, pool))
                self._segments = segs
            x2 = torch.chunk(s['images'], 2, dim=1)[1]
            s['key_in'].copy_(par.shuffle_exchange_planned(x2, plan, self.ctx, ops.gather_rows))
            self._segments[0].run()
            s['all_k'].copy_(par.gather_keys(s['k_shuf'], self.ctx))
            s['k'].copy_(ops.gather_rows(s['all_k'], plan['unshuffle_idx']))
            bk = self._buckets
            be = int(getattr(self, 'bucket_elems', BUCKET_ELEMS))
            planning = len(bk) == 1 and not self._planned and 0 < be < self.arena_q.total
            log = None
            if planning:
                if L.GRAD_LOG is not None:
                    raise RuntimeError('another trainer is planning its gradient buckets (engine.layers.GRAD_LOG is live)')
                L.GRAD_LOG = log = []
            try:
                for i, (_, lo, hi) in enumerate(bk):
                    self._segments[1 + i].run()
                    self._reducer.launch(lo, hi)
            finally:
                if planning:
                    L.GRAD_LOG = None        # whatever happened in the step, the log never outlives it
            self._reducer.wait()
            self._segments[-1].run()
            if user_ids is None:
                self._plans.prefetch(self.step_count + 1)        # host index work of the NEXT step, while this one runs
            if planning:
                # the first step ran un-staged with the gradient log on: cut the arena into buckets by the closure that
                # completes each and rebuild the segments, so that every later step overlaps all-reduce and backward
                self._buckets = self._buckets_from_log(self.arena_q, log)
                self._planned = True             # only once the buckets exist: a step that raised is planned again
                for g in self._segments:
                    g.release()
                self._segments = None
        if self._packers is None:
            self._packers = dict(k=BatchedPacker(self.model_ema, (0,)), q=BatchedPacker(self.model, (0, 1)))
        self.contrast.index = (self.contrast.index + b * W) % self.K      # host mirror of ptr_dev
        self.step_count += 1
        return self.out

    def state_dict(self, epoch=0):
        """Checkpoint dict with the reference's keys (tools/...dis.py:274-286) + the queue pointer."""
        return {'epoch': epoch, 'state_dict': self.model.state_dict(), 'optimizer': self.optimizer.state_dict(),
                'contrast': self.contrast.state_dict(), 'model_ema': self.model_ema.state_dict(),
                'queue_index': int(self.contrast.index), 'step_count': int(self.step_count),
                **({} if self.scale_state is None else {'loss_scale_state': self.scale_state.detach().cpu().clone()})}

    def load_state_dict(self, sd):
        """Resume from state_dict() -- or from a reference checkpoint, which lacks `queue_index` / `step_count`
        (the reference restarts the queue pointer at 0 on resume; so do we for such a file)."""
        self.model.load_state_dict(sd['state_dict'])
        self.model_ema.load_state_dict(sd['model_ema'])
        self.optimizer.load_state_dict(sd['optimizer'])
        self.contrast.load_state_dict(sd['contrast'])
        self.contrast.index = int(sd.get('queue_index', 0)) % self.K
        self.ptr_dev.fill_(self.contrast.index)
        self.step_count = int(sd.get('step_count', 0))
        if self.scale_state is not None and sd.get('loss_scale_state') is not None:
            self.scale_state.copy_(sd['loss_scale_state'])
        return int(sd.get('epoch', 0))


class ReSSLTrainer(MoCoTrainer):
    """ReSSL pre-training (CONTRAST.MEM_TYPE 'ressl'; queue of CONTRAST.NCE_K rows of width CROSS.FEAT_DIM, student / teacher
    temperatures CONTRAST.RESSL_TS / RESSL_TT, teacher momentum CONTRAST.ALPHA): MoCoTrainer's step with the relational loss in
    InfoNCE's place.  The model and its momentum teacher are MoCo's, the queue is the `memory` of lib.memory.ressl.ReSSLLoss.
    After both encoder forwards:

        ressl_fwd(q, k, PRE-enqueue queue)      ressl_bwd -> q.grad (x loss scale / world)
        all_k enqueued at the device pointer, pointer advanced      tape backward

    The gradient is taken before the enqueue, so no overwritten rows are saved.  Key encoder on the second stream, packers,
    graph capture, the EMA, checkpoints and the StagedBatch input are inherited.  `out` carries `loss` and `ent` (the teacher's
    mean entropy over the queue: the collapse monitor), `row_loss` (b,) and the query features `q`.  One GPU only: the
    inherited multi-GPU path is untested with this loss."""

    def __init__(self, cfg, device, ctx=None, use_graph=True, seed=None):
        if cfg.CONTRAST.MEM_TYPE != 'ressl':
            raise ValueError('ReSSLTrainer needs CONTRAST.MEM_TYPE == ressl (got %r)' % (cfg.CONTRAST.MEM_TYPE,))
        if ctx is not None and ctx.active:
            raise NotImplementedError('ReSSLTrainer runs on one GPU: the inherited multi-GPU step is untested with this loss')
        super().__init__(cfg, device, ctx, use_graph, seed)
        self.inv_Ts, self.inv_Tt = 1.0 / self.contrast.Ts, 1.0 / self.contrast.Tt

    def _phase_query_rest(self, tape, qv, upto=0):
        s = self._static
        mem = self.contrast.memory
        loss, row_lse, row_loss = ops.ressl_fwd(qv.t, s['k'], mem, self.inv_Ts, self.inv_Tt)
        qv.grad = ops.ressl_bwd(qv.t, s['k'], mem, row_lse, self.inv_Ts, self.inv_Tt, gscale_dev=self.scale_state,
                                gscale_host=1.0 / self.ctx.world)
        ops.queue_enqueue(mem, s['all_k'], 0, ptr_dev=self.ptr_dev)
        ops.queue_advance(self.ptr_dev, s['all_k'].shape[0], self.K)
        self.out = dict(loss=loss[:1], ent=loss[1:], row_loss=row_loss, q=qv.t)
        self._backward(tape, upto)
        self._tape = tape if upto > 0 else None
        if upto == 0:
            self._unpack('q')


class _TwoViewTrainer(_TrainerBase):
    """One encoder, both views of a (b, 6, T, H, W) batch through it with gradients, a loss formed inside the model
    (``model.fwd`` returns the loss Var): the step that SimSiamTrainer and SimCLRTrainer share.  A subclass checks its
    configuration (_check_cfg / _check_model) and says what a step reports (_outputs)."""

    def __init__(self, cfg, device, ctx=None, use_graph=True, seed=None):
        _check_unsupported(cfg)
        self.cfg, self.device = cfg, torch.device(device)
        self.clip = clip_value_of(cfg)
        self.ctx = ctx or par.DistCtx()
        self._check_cfg(cfg)
        ls = _loss_scale()
        self.scale_state = None if ls is None else ops.loss_scale_state(ls, torch.device(device))
        if seed is not None:
            torch.manual_seed(seed)
        self.model, ema = create_visual_model(cfg)
        self._check_model(ema)
        self.model.to(self.device)
        self.arena = arena_of(self.model)
        par.broadcast_(self.arena.flat, self.ctx)
        self.optimizer = make_optimizer(cfg, self.model)
        self.scheduler = make_lr_scheduler(cfg, self.optimizer)
        self.model.train()
        self.use_graph = bool(use_graph)
        self._static, self._segments, self._packer, self.out = None, None, None, {}
        self._buckets, self._planned, self._tape = None, False, None     # N > 1: gradient buckets (see MoCoTrainer)
        self._reducer = par.BucketReducer(self.arena.grad, self.ctx)

    def _check_cfg(self, cfg):
        pass

    def _check_model(self, ema):
        pass

    def _outputs(self, lv):
        return dict(loss=lv.t)

    def _loss(self, tape):
        """The loss Var of the static batch, its backward recorded on `tape`."""
        return self.model.fwd(tape, Var(self._static))

    def _fwd_bwd(self, upto=0):
        """Forward, loss and the backward pass down to tape index `upto` (0 = all of it; N > 1 runs the rest in stages)."""
        self.optimizer.zero_grad()
        if self._packer is not None:
            self._packer.run()
        tape = Tape(True)
        lv = self._loss(tape)
        self.out = self._outputs(lv)
        ops.LOSS_SCALE_STATE[0] = self.scale_state            # fp16 storage: the model's loss-gradient seed is scaled by S
        try:
            self._backward(tape, upto)
        finally:
            ops.LOSS_SCALE_STATE[0] = None
        self._tape = tape if upto > 0 else None
        if upto == 0 and self._packer is not None:
            self._packer.release()

    def _bwd_stage(self, upto, last):
        ops.LOSS_SCALE_STATE[0] = self.scale_state
        try:
            self._backward(self._tape, upto)
        finally:
            ops.LOSS_SCALE_STATE[0] = None
        if last:
            self._tape = None
            if self._packer is not None:
                self._packer.release()

    def _update(self):
        if self.ctx.active:
            ops.scale_(self.arena.grad, 1.0 / self.ctx.world)      # DDP's mean (the loss gradient is seeded inside the model)
        clip = None
        if self.scale_state is not None:                       # fp16 storage: un-scale + overflow check + clip, see MoCoTrainer
            clip = ops.grad_unscale_clip(self.arena.grad, self.scale_state, self.clip)
            self.out['grad_norm'] = clip
            self.out['loss_scale'] = self.scale_state
        elif self.clip is not None:                            # tools/train_video_contrast_dis.py:497-500
            clip = self.optimizer.clip_grad_norm(self.clip)
            self.out['grad_norm'] = clip
        self.optimizer.step(grad_clip=clip)

    def train_step(self, images):
        """images: (b, 6, T, H, W) fp32 on the device, or a StagedBatch (engine.input.DeviceInputStage)."""
        staged = images if isinstance(images, StagedBatch) else None
        shape = torch.Size(staged.stage.out_shape()) if staged is not None else images.shape
        if self._static is None or self._static.shape != shape:
            self._static = torch.empty(tuple(shape), dtype=torch.float32, device=self.device)
            self._packer = None
            self._segments = None
        if staged is not None:
            staged.stage.prepare(staged, self._static)
        else:
            self._static.copy_(images)
        self.optimizer._sync_tables()
        if not self.ctx.active:
            if self._segments is None:
                self._segments = [_Graphed(self._fwd_bwd, self.use_graph), _Graphed(self._update, self.use_graph)]
            self._segments[0].run()
            self._segments[1].run()
        else:
            # staged backward, one graph segment per gradient bucket, all-reduce of a bucket overlapped with the stages
            # below it (as MoCoTrainer.train_step); the first step runs un-staged with the gradient log on and plans the buckets
            if self._segments is None:
                pool = torch.cuda.graph_pool_handle() if self.use_graph else None
                if self._buckets is None:
                    self._buckets = [(0, 0, self.arena.total)]
                bk = self._buckets
                last = len(bk) - 1
                segs = [_Graphed(lambda u=(0 if last == 0 else bk[0][0]): self._fwd_bwd(u), self.use_graph, pool)]
                for i in range(1, len(bk)):
                    segs.append(_Graphed(lambda u=(0 if i == last else bk[i][0]), l=(i == last): self._bwd_stage(u, l),
                                         self.use_graph, pool))
                segs.append(_Graphed(self._update, self.use_graph, pool))
                self._segments = segs
            bk = self._buckets
            be = int(getattr(self, 'bucket_elems', BUCKET_ELEMS))
            planning = len(bk) == 1 and not self._planned and 0 < be < self.arena.total
            log = None
            if planning:
                if L.GRAD_LOG is not None:
                    raise RuntimeError('another trainer is planning its gradient buckets (engine.layers.GRAD_LOG is live)')
                L.GRAD_LOG = log = []
            try:
                for i, (_, lo, hi) in enumerate(bk):
                    self._segments[i].run()
                    self._reducer.launch(lo, hi)
            finally:
                if planning:
                    L.GRAD_LOG = None
            self._reducer.wait()
            self._segments[-1].run()
            if planning:
                self._buckets = self._buckets_from_log(self.arena, log)
                self._planned = True
                for g in self._segments:
                    g.release()
                self._segments = None
        if self._packer is None:
            self._packer = BatchedPacker(self.model, (0, 1))
        return self.out

    def state_dict(self, epoch=0):
        """Checkpoint dict with the reference's keys (tools/...dis.py:274-286; neither SimSiam nor SimCLR has a memory, so
        `contrast` is None as the reference writes it).  ActionTrainer.load_pretrained and lib.evaluation.load_encoder read its
        `state_dict`."""
        return {'epoch': epoch, 'state_dict': self.model.state_dict(), 'optimizer': self.optimizer.state_dict(), 'contrast': None,
                **({} if self.scale_state is None else {'loss_scale_state': self.scale_state.detach().cpu().clone()})}

    def load_state_dict(self, sd):
        """Resume from state_dict() (bit-exact: parameters, BatchNorm buffers, optimizer state, learning rates) or from a
        reference checkpoint -> the epoch."""
        self.model.load_state_dict(sd['state_dict'])
        self.optimizer.load_state_dict(sd['optimizer'])
        if self.scale_state is not None and sd.get('loss_scale_state') is not None:
            self.scale_state.copy_(sd['loss_scale_state'])
        return int(sd.get('epoch', 0))


class SimSiamTrainer(_TwoViewTrainer):
    """tools/train_video_contrast_dis.py:479-523 (_train_simsiam): CONTRAST.MEM_TYPE 'simsiam'."""

    def _check_model(self, ema):
        if ema is not None:
            raise ValueError('SimSiamTrainer needs CONTRAST.MEM_TYPE == simsiam')


class SimCLRTrainer(_TwoViewTrainer):
    """In-batch contrastive pre-training (NT-Xent; CONTRAST.MEM_TYPE 'simclr', temperature CONTRAST.NCE_T): SimSiamTrainer's
    step with lib.modeling.graph_wrappers.SimCLR as the model.  `out` carries `loss` and `rank` (per row of the 2b views, the
    negatives that score at least the positive: a top-k hit iff rank < k).  One GPU only: global negatives need an all-gather
    of the features and an exchange of their gradients."""

    def _check_cfg(self, cfg):
        if cfg.CONTRAST.MEM_TYPE != 'simclr':
            raise ValueError('SimCLRTrainer needs CONTRAST.MEM_TYPE == simclr (got %r)' % (cfg.CONTRAST.MEM_TYPE,))
        if self.ctx.active:
            raise NotImplementedError('SimCLRTrainer runs on one GPU: NT-Xent over the global batch needs a feature all-gather '
                                      'and a gradient exchange between the ranks')

    def _outputs(self, lv):
        return dict(loss=lv.t, rank=self.model.model.rank)


class BarlowTwinsTrainer(_TwoViewTrainer):
    """Barlow Twins pre-training (CONTRAST.MEM_TYPE 'barlow', off-diagonal weight CONTRAST.BT_LAMBDA): SimSiamTrainer's step
    with lib.modeling.graph_wrappers.BarlowTwins as the model.  `out` carries `loss` and its two sums `on_diag`, `off_diag`
    (device scalars).  One GPU only: the column statistics and the cross-correlation over the global batch need all-reduces."""

    def _check_cfg(self, cfg):
        if cfg.CONTRAST.MEM_TYPE != 'barlow':
            raise ValueError('BarlowTwinsTrainer needs CONTRAST.MEM_TYPE == barlow (got %r)' % (cfg.CONTRAST.MEM_TYPE,))
        if self.ctx.active:
            raise NotImplementedError('BarlowTwinsTrainer runs on one GPU: column statistics and the cross-correlation over the '
                                      'global batch need all-reduces between the ranks')

    def _outputs(self, lv):
        return dict(loss=lv.t, on_diag=self.model.model.on_diag, off_diag=self.model.model.off_diag)


class VICRegTrainer(_TwoViewTrainer):
    """VICReg pre-training (CONTRAST.MEM_TYPE 'vicreg', weights CONTRAST.VIC_SIM / VIC_STD / VIC_COV): SimSiamTrainer's step with
    lib.modeling.graph_wrappers.VICReg as the model.  `out` carries `loss` and its three unweighted parts `inv`, `var`, `cov`
    (device scalars).  One GPU only: the column statistics and the covariances over the global batch need a feature
    all-gather between the ranks."""

    def _check_cfg(self, cfg):
        if cfg.CONTRAST.MEM_TYPE != 'vicreg':
            raise ValueError('VICRegTrainer needs CONTRAST.MEM_TYPE == vicreg (got %r)' % (cfg.CONTRAST.MEM_TYPE,))
        if self.ctx.active:
            raise NotImplementedError('VICRegTrainer runs on one GPU: column statistics and covariances over the global batch '
                                      'need a feature all-gather between the ranks')

    def _outputs(self, lv):
        m = self.model.model
        return dict(loss=lv.t, inv=m.inv, var=m.var, cov=m.cov)


class SwAVTrainer(_TwoViewTrainer):
    """SwAV pre-training (CONTRAST.MEM_TYPE 'swav'; CONTRAST.SWAV_K prototypes, Sinkhorn SWAV_EPS / SWAV_ITERS, temperature
    SWAV_T): SimSiamTrainer's step with lib.modeling.graph_wrappers.SwAV as the model.  `out` carries `loss` and its two swapped
    terms `l12`, `l21` (device scalars).  One GPU only: the Sinkhorn sums over the global batch need all-reduces between the
    ranks inside every iteration."""

    def _check_cfg(self, cfg):
        if cfg.CONTRAST.MEM_TYPE != 'swav':
            raise ValueError('SwAVTrainer needs CONTRAST.MEM_TYPE == swav (got %r)' % (cfg.CONTRAST.MEM_TYPE,))
        if self.ctx.active:
            raise NotImplementedError('SwAVTrainer runs on one GPU: the Sinkhorn sums over the global batch need all-reduces '
                                      'between the ranks inside every iteration')

    def _outputs(self, lv):
        m = self.model.model
        return dict(loss=lv.t, l12=m.l12, l21=m.l21)


class DINOTrainer(_TwoViewTrainer):
    """DINO pre-training (CONTRAST.MEM_TYPE 'dino'; CONTRAST.DINO_K prototypes, student / teacher temperatures DINO_TS / DINO_TT,
    centre momentum DINO_CM, teacher momentum CONTRAST.ALPHA): self-distillation from a momentum teacher.  The student is
    _TwoViewTrainer's model (lib.modeling.graph_wrappers.DINO: both views through it with gradients); the teacher is a second
    wrapper of the same layout that sees both views without a tape (BatchNorm in train mode, as MoCo's key encoder) and follows
    the student as an EMA over the whole parameter arena, prototypes included.  One step:

        teacher forward, both views (no tape)            student forward, both views (tape)
        both prototype matrices renormalised             dino_fwd: loss, dS, centre update       dino_bwd -> tape backward
        optimizer step                                   EMA of the teacher (momentum read from the device)

    The teacher temperature and the teacher momentum live in one device float each, read by the kernels, so the captured
    step follows their schedules (lib.solver.dino_teacher_temp / cosine_momentum) through set_schedule without re-capture.
    `out` carries `loss`, `l12`, `l21` and `ent` (the mean teacher entropy: log K or 0 when collapsed) as device scalars.
    One GPU only: the centre's column mean over the global batch needs an all-reduce between the ranks."""

    def __init__(self, cfg, device, ctx=None, use_graph=True, seed=None):
        super().__init__(cfg, device, ctx, use_graph, seed)
        self.model_ema.to(self.device)
        self.arena_t = arena_of(self.model_ema)
        if self.arena_t.total != self.arena.total:
            raise RuntimeError('student and teacher must share one parameter layout')
        self.arena_t.flat.copy_(self.arena.flat)                          # the teacher starts as the student
        set_key_encoder_mode(self.model_ema)
        self.contrast = create_contrast(cfg, 0).to(self.device)
        self.teacher_temp, self.momentum = self.contrast.Tt, float(cfg.CONTRAST.ALPHA)
        self.tt_dev = self.contrast.tt_dev(self.device)
        self.m_dev = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.set_schedule(self.teacher_temp, self.momentum)
        self._packer_t, self._packer_t_of = None, None                     # the teacher's BatchedPacker, and the student's it was built next to

    def _check_cfg(self, cfg):
        if cfg.CONTRAST.MEM_TYPE != 'dino':
            raise ValueError('DINOTrainer needs CONTRAST.MEM_TYPE == dino (got %r)' % (cfg.CONTRAST.MEM_TYPE,))
        if self.ctx.active:
            raise NotImplementedError("DINOTrainer runs on one GPU: the centre's column mean over the global batch needs an "
                                      'all-reduce between the ranks')

    def _check_model(self, ema):
        if ema is None:
            raise ValueError('DINOTrainer needs the EMA twin that create_visual_model returns for CONTRAST.MEM_TYPE == dino')
        self.model_ema = ema                                              # the teacher; set up once the base class is done

    def set_schedule(self, teacher_temp=None, momentum=None):
        """Write the teacher temperature and / or the teacher momentum of the following steps into their device scalars
        (outside the captured graph, which reads them).  ValueError for a temperature that is not positive with T and 1 / T
        finite in fp32, or a momentum outside [0, 1]."""
        if teacher_temp is not None:
            teacher_temp = ops.dino_temperature('DINOTrainer.set_schedule', teacher_temp, 'teacher_temp')
        if momentum is not None:
            momentum = float(momentum)
            if not 0.0 <= momentum <= 1.0:
                raise ValueError('DINOTrainer.set_schedule: momentum must lie in [0, 1] (got %r)' % momentum)
        if teacher_temp is not None:
            self.teacher_temp = teacher_temp
            self.contrast.set_teacher_temp(teacher_temp)
        if momentum is not None:
            self.momentum = momentum
            self.m_dev.fill_(momentum)

    def _loss(self, tape):
        s, t, c = self.model.model, self.model_ema.model, self.contrast
        x1, x2 = torch.chunk(self._static, 2, dim=1)               # views, read in place through the batch stride
        packed = self._packer_t is not None and self._packer_t_of is self._packer
        if packed:
            self._packer_t.run()
        zt1 = t.fwd(Tape(False), Var(x1)).t.contiguous()
        zt2 = t.fwd(Tape(False), Var(x2)).t.contiguous()
        if packed:
            self._packer_t.release()
        z1 = s.fwd(tape, Var(x1))
        z2 = s.fwd(tape, Var(x2))
        Cs, Ct = s.prototypes.weight, t.prototypes.weight
        ops.rows_normalize_(Cs.data)
        ops.rows_normalize_(Ct.data)
        a, b = z1.t.contiguous(), z2.t.contiguous()
        parts, dS = ops.dino_fwd(a, b, Cs.data, zt1, zt2, Ct.data, c.Ts, self.tt_dev, c.cm, c.center, True)
        c.l12, c.l21, c.ent = parts[1:2], parts[2:3], parts[3:4]
        lv = Var(parts[:1], True)

        def back():
            # d loss / d (zs1, zs2, Cs); the fp16-storage loss scale folds into the products' scale
            dz1, dz2 = ops.dino_bwd(a, b, Cs.data, dS, L._grad_of(Cs), True, gscale_dev=ops.LOSS_SCALE_STATE[0])
            z1.add_grad(dz1)
            z2.add_grad(dz2)
        tape.record(back)
        return lv

    def _outputs(self, lv):
        c = self.contrast
        return dict(loss=lv.t, l12=c.l12, l21=c.l21, ent=c.ent)

    def _update(self):
        super()._update()
        ops.ema_update_dev(self.arena_t.flat, self.arena.flat, self.m_dev)

    def train_step(self, images):
        out = super().train_step(images)
        if self._packer_t_of is not self._packer:                        # (re)built with the student's, after an eager step
            self._packer_t, self._packer_t_of = BatchedPacker(self.model_ema, (0,)), self._packer
        return out

    def state_dict(self, epoch=0):
        """_TwoViewTrainer's checkpoint plus the teacher (`model_ema`), the centre (`contrast`, in MoCo's place) and the two
        schedule values."""
        sd = super().state_dict(epoch)
        sd.update(model_ema=self.model_ema.state_dict(), contrast=self.contrast.state_dict(), teacher_temp=self.teacher_temp,
                  momentum=self.momentum)
        return sd

    def load_state_dict(self, sd):
        epoch = super().load_state_dict(sd)
        self.model_ema.load_state_dict(sd['model_ema'])
        self.contrast.load_state_dict(sd['contrast'])
        self.set_schedule(sd.get('teacher_temp'), sd.get('momentum'))
        return epoch


class MoCoV3Trainer(_TwoViewTrainer):
    """MoCo v3 pre-training (CONTRAST.MEM_TYPE 'mocov3'; output width CROSS.FEAT_DIM, hidden width CONTRAST.V3_HID, temperature
    CONTRAST.NCE_T, teacher momentum CONTRAST.ALPHA): Algorithm 1 of Chen, Xie, He 2021.  The student is _TwoViewTrainer's model
    (lib.modeling.graph_wrappers.MoCoV3: encoder + projector + predictor, both views through it with gradients); the teacher is
    a second wrapper without the predictor that sees both views without a tape (BatchNorm in train mode, as MoCo's key encoder)
    and follows the student's encoder and projector as an EMA.  One step:

        teacher forward, both views (no tape) -> k1, k2       student forward, both views (tape) -> q1, q2
        mocov3_fwd: 2 T (CE(q1 k2^T / T) + CE(q2 k1^T / T))   mocov3_bwd -> tape backward
        optimizer step                                        THEN the EMA of the teacher (keys came from the pre-update teacher)

    The teacher's parameter arena is exactly the leading part of the student's (same names, same offsets, the predictor last;
    checked at construction), so the EMA is ONE launch over arena.flat[:arena_t.total] with the momentum read from a device
    float: the captured step follows lib.solver.cosine_momentum through set_schedule without re-capture.  BatchNorm buffers
    are not averaged.  `out` carries `loss`, `l12`, `l21` (device scalars) and `rank` (2, N) int32.  The loss of a step is
    _pair_loss alone: BYOL would be this trainer with gca_negcos_fwd_bwd there.  One GPU only: the keys of the global batch
    need an all-gather between the ranks."""

    def __init__(self, cfg, device, ctx=None, use_graph=True, seed=None):
        super().__init__(cfg, device, ctx, use_graph, seed)
        self.model_ema.to(self.device)
        self.arena_t = arena_of(self.model_ema)
        a, t = self.arena, self.arena_t
        n = len(t.names)
        if not (n < len(a.names) and a.names[:n] == t.names and a.offsets[:n] == t.offsets and a.sizes[:n] == t.sizes
                and t.total == a.offsets[n] and all('.prediction.' in k for k in a.names[n:])
                and not any('.prediction.' in k for k in t.names)):
            raise RuntimeError("the teacher's parameter arena must be the leading part of the student's (same names and offsets, "
                               'the predictor last)')
        t.flat.copy_(a.flat[:t.total])                                     # the teacher starts as the student
        set_key_encoder_mode(self.model_ema)
        self.contrast = create_contrast(cfg, 0)
        self.inv_T = 1.0 / self.contrast.T
        self.momentum = float(cfg.CONTRAST.ALPHA)
        self.m_dev = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.set_schedule(self.momentum)
        self._packer_t, self._packer_t_of = None, None                     # the teacher's BatchedPacker, and the student's it was built next to
        self._l12 = self._l21 = self._rank = None

    def _check_cfg(self, cfg):
        if cfg.CONTRAST.MEM_TYPE != 'mocov3':
            raise ValueError('MoCoV3Trainer needs CONTRAST.MEM_TYPE == mocov3 (got %r)' % (cfg.CONTRAST.MEM_TYPE,))
        if self.ctx.active:
            raise NotImplementedError('MoCoV3Trainer runs on one GPU: the keys of the global batch need an all-gather between '
                                      'the ranks')

    def _check_model(self, ema):
        if ema is None:
            raise ValueError('MoCoV3Trainer needs the EMA twin that create_visual_model returns for CONTRAST.MEM_TYPE == mocov3')
        self.model_ema = ema                                              # the teacher; set up once the base class is done

    def set_schedule(self, momentum=None):
        """Write the teacher momentum of the following steps into its device scalar (outside the captured graph, which reads
        it).  ValueError for a momentum outside [0, 1]."""
        if momentum is not None:
            momentum = float(momentum)
            if not 0.0 <= momentum <= 1.0:
                raise ValueError('MoCoV3Trainer.set_schedule: momentum must lie in [0, 1] (got %r)' % momentum)
            self.momentum = momentum
            self.m_dev.fill_(momentum)

    def _pair_loss(self, q1, q2, k1, k2):
        """The loss of the student rows q1, q2 against the teacher rows k1, k2 -> (loss (1,), backward() -> (dq1, dq2))."""
        loss, lse, self._rank, _ = ops.mocov3_fwd(q1, q2, k1, k2, self.inv_T, want_rank=True)
        self._l12, self._l21 = loss[1:2], loss[2:3]

        def backward():
            # the fp16-storage loss scale folds into the products' scale
            return ops.mocov3_bwd(q1, q2, k1, k2, lse, self.inv_T, gscale_dev=ops.LOSS_SCALE_STATE[0])
        return loss[:1], backward

    def _loss(self, tape):
        s, t = self.model.model, self.model_ema.model
        x1, x2 = torch.chunk(self._static, 2, dim=1)               # views, read in place through the batch stride
        packed = self._packer_t is not None and self._packer_t_of is self._packer
        if packed:
            self._packer_t.run()
        k1 = t.fwd(Tape(False), Var(x1)).t.contiguous()
        k2 = t.fwd(Tape(False), Var(x2)).t.contiguous()
        if packed:
            self._packer_t.release()
        z1 = s.fwd(tape, Var(x1))
        z2 = s.fwd(tape, Var(x2))
        loss, backward = self._pair_loss(z1.t.contiguous(), z2.t.contiguous(), k1, k2)
        lv = Var(loss, True)

        def back():
            dq1, dq2 = backward()
            z1.add_grad(dq1)
            z2.add_grad(dq2)
        tape.record(back)
        return lv

    def _outputs(self, lv):
        return dict(loss=lv.t, l12=self._l12, l21=self._l21, rank=self._rank)

    def _update(self):
        super()._update()
        ops.ema_update_dev(self.arena_t.flat, self.arena.flat[:self.arena_t.total], self.m_dev)

    def train_step(self, images):
        out = super().train_step(images)
        if self._packer_t_of is not self._packer:                        # (re)built with the student's, after an eager step
            self._packer_t, self._packer_t_of = BatchedPacker(self.model_ema, (0,)), self._packer
        return out

    def state_dict(self, epoch=0):
        """_TwoViewTrainer's checkpoint plus the teacher (`model_ema`) and the momentum."""
        sd = super().state_dict(epoch)
        sd.update(model_ema=self.model_ema.state_dict(), momentum=self.momentum)
        return sd

    def load_state_dict(self, sd):
        epoch = super().load_state_dict(sd)
        self.model_ema.load_state_dict(sd['model_ema'])
        self.set_schedule(sd.get('momentum'))
        return epoch


class NNCLRTrainer(_TwoViewTrainer):
    """NNCLR pre-training (CONTRAST.MEM_TYPE 'nnclr'; output width CROSS.FEAT_DIM, hidden width CONTRAST.NN_HID, support set of
    CONTRAST.NCE_K rows, temperature CONTRAST.NCE_T): Algorithm 1 of Dwibedi et al. 2021.  The model is
    lib.modeling.graph_wrappers.NNCLR (encoder + projector + predictor, no momentum encoder); the support set is the `memory`
    of lib.memory.nnclr.NNCLRLoss.  One step:

        both views through fwd_zp (tape) -> z1, p1, z2, p2     nnclr_search of the PRE-enqueue support set -> nn1, nn2
        mocov3_fwd(nn1, nn2, p1, p2, w = 1/2)                  nnclr_bwd -> p1, p2 -> tape backward
        z1 enqueued at the device pointer, pointer advanced    optimizer step

    The queue pointer lives on the device (ptr_dev, as MoCoTrainer's), so replays of the captured step move it; the module's
    `index` is its host mirror.  `out` carries `loss`, `l12`, `l21` (device scalars), `rank` (2, N) int32 and the neighbours
    `idx` (2, N) int32 with their scores `sim`.  One GPU only: the support set of the global batch needs an all-gather of the
    projections between the ranks."""

    def __init__(self, cfg, device, ctx=None, use_graph=True, seed=None):
        super().__init__(cfg, device, ctx, use_graph, seed)
        self.contrast = create_contrast(cfg, 0).to(self.device)
        self.inv_T = 1.0 / self.contrast.T
        self.K = self.contrast.K
        self.ptr_dev = torch.zeros(1, dtype=torch.long, device=self.device)
        self._aux = {}

    def _check_cfg(self, cfg):
        if cfg.CONTRAST.MEM_TYPE != 'nnclr':
            raise ValueError('NNCLRTrainer needs CONTRAST.MEM_TYPE == nnclr (got %r)' % (cfg.CONTRAST.MEM_TYPE,))
        if self.ctx.active:
            raise NotImplementedError('NNCLRTrainer runs on one GPU: the support set of the global batch needs an all-gather '
                                      'of the projections between the ranks')

    def _check_model(self, ema):
        if ema is not None:
            raise ValueError('NNCLRTrainer needs CONTRAST.MEM_TYPE == nnclr (NNCLR has no momentum encoder)')

    def _loss(self, tape):
        m = self.model.model
        x1, x2 = torch.chunk(self._static, 2, dim=1)               # views, read in place through the batch stride
        z1, p1 = m.fwd_zp(tape, Var(x1))
        z2, p2 = m.fwd_zp(tape, Var(x2))
        mem = self.contrast.memory
        z1t = z1.t.contiguous()
        idx, sim, nn1, nn2 = ops.nnclr_search(z1t, z2.t.contiguous(), mem)      # the pre-enqueue support set
        p1t, p2t = p1.t.contiguous(), p2.t.contiguous()
        loss, lse, rank, _ = ops.mocov3_fwd(nn1, nn2, p1t, p2t, self.inv_T, w=ops.nnclr_weight(), want_rank=True)
        ops.queue_enqueue(mem, z1t, 0, ptr_dev=self.ptr_dev)
        ops.queue_advance(self.ptr_dev, z1t.shape[0], self.K)
        self._aux = dict(l12=loss[1:2], l21=loss[2:3], rank=rank, idx=idx, sim=sim)
        lv = Var(loss[:1], True)

        def back():
            # the fp16-storage loss scale folds into the products' scale
            dp1, dp2 = ops.nnclr_bwd(nn1, nn2, p1t, p2t, lse, self.inv_T, gscale_dev=ops.LOSS_SCALE_STATE[0])
            p1.add_grad(dp1)
            p2.add_grad(dp2)
        tape.record(back)
        return lv

    def _outputs(self, lv):
        return dict(loss=lv.t, **self._aux)

    def train_step(self, images):
        b = (images.stage.out_shape() if isinstance(images, StagedBatch) else images.shape)[0]
        if b > self.K:
            raise ValueError('NNCLRTrainer: cannot enqueue %d rows into a support set of %d' % (b, self.K))
        out = super().train_step(images)
        self.contrast.index = (self.contrast.index + b) % self.K          # host mirror of ptr_dev
        return out

    def state_dict(self, epoch=0):
        """_TwoViewTrainer's checkpoint plus the support set (`contrast`) and its pointer (`queue_index`)."""
        sd = super().state_dict(epoch)
        sd.update(contrast=self.contrast.state_dict(), queue_index=int(self.contrast.index))
        return sd

    def load_state_dict(self, sd):
        epoch = super().load_state_dict(sd)
        self.contrast.load_state_dict(sd['contrast'])
        self.contrast.index = int(sd.get('queue_index', 0)) % self.K
        self.ptr_dev.fill_(self.contrast.index)
        return epoch


class ActionTrainer(_TrainerBase):
    """Action-recognition fine-tuning and linear probing of a (pre-trained) encoder: the iteration of the reference's
    tools/train_ds.py:97-125 (train) and :170-190 (validation) on the HIP engine.  Eager, single GPU, fp32 storage.

    Fine-tune (default): recording tape through the encoder and the fused class head (engine.layers.f_classifier), backward,
    optional SOLVER.CLIP_GRADIENT, then make_optimizer(cfg, model)'s HipSGD / HipAdam / HipLARS over the whole model -- the
    reference's one-group-per-parameter rules.

    Linear probe (MODEL.LINEAR_PROBE): the encoder runs under model.train() on a non-recording tape, so nothing in it is
    recorded or updated except the running statistics of its training-mode BatchNorms (tools/train_ds.py:81-84 freezes the
    parameters, not the statistics); only the head is taped, and the optimizer is make_optimizer's over the head alone (group names
    `<prefix>fc.weight` / `<prefix>fc.bias`, same lr / weight-decay / bias rules).  The reference freezes every parameter
    whose name lacks `new_fc`, which with MODEL.DROPOUT == 0 freezes the head too and trains nothing; here the probe trains
    the head wherever it lives (base_model.fc or new_fc).

    Not built, refused at construction: fine-tuning under partial BatchNorm (SOLVER.NO_PARTIALBN False: backward through an
    eval-mode BatchNorm), fp16 storage, SOLVER.USE_TRICK, APEX.FLAG, more than one GPU, hipGraph capture."""

    def __init__(self, cfg, device, seed=None, ctx=None, use_graph=False):
        _check_unsupported(cfg)
        if ops.ACT_F16[0]:
            raise NotImplementedError('ActionTrainer runs on fp32 storage (ops.set_conv_math(\'fp16\') is active)')
        if bool(cfg.SOLVER.USE_TRICK):
            raise NotImplementedError('SOLVER.USE_TRICK (get_optim_policies, model_wrappers.py:150-213) is not built')
        if ctx is not None and ctx.active:
            raise NotImplementedError('ActionTrainer is single-GPU: an active DistCtx is not supported')
        if use_graph:
            raise NotImplementedError('ActionTrainer runs eagerly: hipGraph capture of the step is not built')
        self.probe = bool(getattr(cfg.MODEL, 'LINEAR_PROBE', False))
        if not self.probe and not bool(cfg.SOLVER.NO_PARTIALBN):
            raise NotImplementedError('fine-tuning under partial BatchNorm (SOLVER.NO_PARTIALBN False) needs the backward '
                                      'through eval-mode BatchNorm, which is not built; the linear probe accepts it')
        check_optimizer_name(cfg)
        self.cfg, self.device = cfg, torch.device(device)
        self.clip = clip_value_of(cfg)
        self.criterion = creat_criterion(cfg)          # (validates MODEL.METRIC_LOSS_TYPE; the step runs it fused with the head)
        if seed is not None:
            torch.manual_seed(seed)
        self.model = create_video_model(cfg)
        self.model.to(self.device)
        self.num_class = self.model.num_class
        if self.probe:
            head, prefix = self.model.classifier, self.model.classifier_prefix
            for name, prm in self.model.named_parameters():
                if not name.startswith(prefix):
                    prm.requires_grad = False
            self.optimizer = make_optimizer(cfg, head, name_prefix=prefix)
        else:
            arena_of(self.model)
            self.optimizer = make_optimizer(cfg, self.model)
        self.scheduler = make_lr_scheduler(cfg, self.optimizer)
        self.model.train()
        self.best_pred = 0.0
        self._segments = None
        self._staged_clips = None                      # (b * views, 3, T, H, W) fp32: where staged batches are prepared
        self.out = {}

    def load_pretrained(self, checkpoint):
        """Encoder weights of a pre-training checkpoint (a path, or the dict the pre-training trainers write), loaded BY NAME:
        the `encoder.base_model.*` entries of its state_dict go to `base_model.*` (lib.evaluation.encoder_state_dict).  The
        reference zips model keys with checkpoint values by position (tools/train_ds.py:73-77); where that works it is the
        same assignment.  The class head stays as initialised."""
        if not isinstance(checkpoint, dict):
            checkpoint = torch.load(checkpoint, map_location='cpu', weights_only=False)
        prefix = self.model.classifier_prefix
        enc = {k: v for k, v in encoder_state_dict(checkpoint['state_dict']).items() if not k.startswith(prefix)}
        res = self.model.load_state_dict(enc, strict=False)
        missing = [k for k in res.missing_keys if not k.startswith(prefix)]
        if missing or res.unexpected_keys:
            raise KeyError('pre-training checkpoint does not match the encoder: missing %s, unexpected %s'
                           % (missing[:4], list(res.unexpected_keys)[:4]))
        return self

    def _labels(self, target, b):
        """Range check on the host copy of the labels, then the int64 device vector.  (Device labels are copied back for the
        check: pass host labels to avoid that sync.)"""
        host = torch.as_tensor(target).detach().reshape(-1).to('cpu', torch.int64)
        if host.numel() != b:
            raise ValueError('one label per clip expected (got %d for %d clips)' % (host.numel(), b))
        if b and (int(host.min()) < 0 or int(host.max()) >= self.num_class):
            raise ValueError('labels must lie in [0, %d) (got %d .. %d)' % (self.num_class, int(host.min()), int(host.max())))
        return host.to(self.device)

    def _clips(self, images):
        if isinstance(images, StagedBatch):
            # uint8 source frames staged by engine.input.ActionInputStage: all views of the batch are cut, resized, flipped
            # and normalised into a buffer the trainer keeps (gca_clip_views), then the step proceeds as on fp32 clips
            stage = images.stage
            if not isinstance(stage, ActionInputStage):
                raise RuntimeError('ActionTrainer takes batches staged by an ActionInputStage')
            if stage.device != self.device:
                raise RuntimeError('batch was staged on %s, the trainer runs on %s' % (stage.device, self.device))
            shape = stage.out_shape()
            if self._staged_clips is None or tuple(self._staged_clips.shape) != shape:
                self._staged_clips = torch.empty(shape, dtype=torch.float32, device=self.device)
            return stage.prepare(images, self._staged_clips)
        if images.device != self.device or images.dtype != torch.float32 or images.dim() != 5:
            raise RuntimeError('fp32 clips (b, 3, T, H, W) already resident on %s are needed' % self.device)
        return images.contiguous()

    def train_step(self, images, target):
        """images (b, 3, T, H, W) fp32 on the device -- or a StagedBatch of engine.input.ActionInputStage (uint8 source frames
        on their way to the device) --, target (b,) integer labels -> dict of device tensors: loss (1,), logits (b, C), rank_ge
        (b,), prec1 / prec5 (1,) in percent (accuracy(), tools/train_ds.py:120, from the fused ranks: no host sync)."""
        x = self._clips(images)
        tgt = self._labels(target, x.shape[0])
        if not self.model.training:
            self.model.train()
        self.optimizer._sync_tables()
        self.optimizer.zero_grad()
        if self.probe:
            feat = self.model.features(Tape(False), Var(x))
            tape = Tape(True)
            lv, logits, _, rank = L.f_classifier(tape, self.model.classifier, Var(feat.t, False), tgt)
        else:
            tape = Tape(True)
            lv, logits, _, rank = self.model.fwd_loss(tape, Var(x), tgt)
        self._backward(tape, 0)
        clip = None
        if self.clip is not None:                      # tools/train_ds.py:113-116
            clip = self.optimizer.clip_grad_norm(self.clip)
        self.optimizer.step(grad_clip=clip)
        prec1, prec5 = accuracy_from_rank(rank, (1, 5))
        self.out = dict(loss=lv.t, logits=logits, rank_ge=rank, prec1=prec1, prec5=prec5)
        if clip is not None:
            self.out['grad_norm'] = clip
        return self.out

    def validate(self, batches):
        """Eval mode, no tape (tools/train_ds.py:160-190): -> dict(loss, top1, top5, count), loss and accuracies (percent)
        averaged by sample count.  One host sync, at the end.  A batch is (fp32 clips | StagedBatch, labels)."""
        self.model.eval()
        tot = torch.zeros(3, dtype=torch.float64, device=self.device)
        n = 0
        for images, target in batches:
            x = self._clips(images if isinstance(images, StagedBatch) else images.to(self.device))
            tgt = self._labels(target, x.shape[0])
            lv, _, _, rank = self.model.fwd_loss(Tape(False), Var(x), tgt)
            b = x.shape[0]
            tot += torch.stack([lv.t[0].double() * b, (rank < 1).sum().double(), (rank < 5).sum().double()])
            n += b
        self.model.train()
        if n == 0:
            raise ValueError('validate: no batches')
        loss, c1, c5 = (float(v) for v in tot.cpu())
        return dict(loss=loss / n, top1=100.0 * c1 / n, top5=100.0 * c5 / n, count=n)

    def state_dict(self, epoch=0):
        """The reference's checkpoint format (tools/train_ds.py:153-158): epoch, state_dict (the reference's model keys),
        optimizer (torch.optim.SGD's / Adam's wire format; LARS writes SGD's), best_pred.  In linear-probe mode the optimizer entry holds the class
        head's two groups only -- the probe's optimizer has no others."""
        return {'epoch': epoch, 'state_dict': self.model.state_dict(), 'optimizer': self.optimizer.state_dict(),
                'best_pred': self.best_pred}

    def load_state_dict(self, sd):
        """Resume from state_dict() (bit-exact: parameters, BatchNorm buffers, momentum, learning rates) -> the epoch."""
        self.model.load_state_dict(sd['state_dict'])
        self.optimizer.load_state_dict(sd['optimizer'])
        self.best_pred = float(sd.get('best_pred', 0.0))
        return int(sd.get('epoch', 0))
