"""LARS on the device: gca_lars_step against the fp64 specification (tests/lars_ref.py), its determinism, its agreement with
the SGD kernel where no trust ratio applies, HipLARS's wire format, the trainers' wiring by decomposition, and checkpoints.

Norms.  The kernels sum exact fp64 squares of fp32 values, so a tensor of n elements is within n * 2^-53 relative of the true
norm whatever the order of summation; the reference norms (exact sums, rounded once) are compared at that bar.  The trust ratio
is formed in fp64 and rounded once: 2 fp32 roundings against the fp64 q (one for the rounding, one as allowance for the norms).

The update.  Every comparison of a kernel result with the specification is per element

    |got - want| <= k * 2^-24 * max(|want|, |update|)

with |update| from lars_ref.update_magnitude and k the number of fp32 roundings on the kernel's own path to the value, counted
without crediting fused multiply-adds.  The specification is applied to the kernel's own state before the step and to the chunk
tables as the kernel reads them (fp32):

    buf  (7)  grad * coef (1), wd * p (1), their sum (1), q rounded to fp32 (1), q * d (1), momentum * buf (1), the sum (1)
    p    (9)  buf (7), lr * buf (1), the difference (1)
    p   (11)  under nesterov: d + momentum * buf carries d (5) and momentum * buf (7 + 1) on terms that |update| adds up, hence
              at most 8 on the sum, its own rounding (1), lr * that (1), the difference (1)"""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lars_ref as ref                   # noqa: E402
import classify_model as cm              # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
K_BUF, K_P, K_P_NESTEROV = 7, 9, 11
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53
MOM, TAU, EPS = 0.9, 0.001, 1e-8


def f64(t):
    return t.detach().double().cpu().numpy()


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def assert_step(tag, before, after, grad, sizes, lr, wd, adapt, trust, norms, nesterov=False, coef=1.0, skip=False,
                mom=MOM, tau=TAU, eps=EPS):
    """before / after: (p, buf) device tensors around one step; lr / wd: per TENSOR, as the kernel reads them; trust / norms: the
    device records after the step.  -> the fp64 q per tensor."""
    p0, b0 = (f64(a) for a in before)
    g = f64(grad)
    if skip:
        for name, x, y in zip(('p', 'buf'), before, after):
            assert torch.equal(bits(x), bits(y)), (tag, name)
        return None
    wp, wb, q, wn = ref.lars_step(p0, g, b0, sizes, lr, wd, adapt, mom, nesterov, tau, eps, coef)
    gn, gq = f64(norms), f64(trust)
    nbar = np.array(sizes, dtype=np.float64)[:, None] * EPS64 * wn
    assert (np.abs(gn - wn) <= nbar).all(), (tag, 'norms', gn, wn)
    assert (np.abs(gq - q) <= 2 * EPS32 * q).all(), (tag, 'trust', gq, q)
    up, ub = ref.update_magnitude(p0, g, b0, sizes, lr, wd, q, mom, nesterov, coef)
    worst = {}
    for name, k, got, w, u in (('p', K_P_NESTEROV if nesterov else K_P, after[0], wp, up), ('buf', K_BUF, after[1], wb, ub)):
        err = np.abs(f64(got) - w)
        scale = np.maximum(np.abs(w), u)
        ulps = err / np.maximum(EPS32 * scale, 1e-300)
        worst[name] = float(ulps.max())
        assert not (err > k * EPS32 * scale).any(), (tag, name, 'worst %.2f roundings (bar %d) at %d' % (ulps.max(), k, int(ulps.argmax())))
    print('MEASURED %s: worst error in roundings p %.2f buf %.2f (bars %d / %d); norms %.2f of n * 2^-53; trust %.2f roundings'
          % (tag, worst['p'], worst['buf'], K_P_NESTEROV if nesterov else K_P, K_BUF,
             float((np.abs(gn - wn) / np.maximum(nbar, 1e-300)).max()), float((np.abs(gq - q) / (EPS32 * q)).max())))
    return q


# ----------------------------------------------------------------------------- 1. kernels against the specification
def six(pkg):
    """The six tensors: one element (not adapted); 5 x 51 = 255 (no multiple of 4 or of a chunk); 700 with weight decay; three
    jobs, the last one partial; exactly one chunk of zero weights; a zero gradient.  -> (sizes, (lr, wd) per tensor, adapt)"""
    J = pkg._hip.lib.gca_lars_job_chunks()
    sizes = (1, 255, 700, 2 * J * 256 + 300, 256, 300)
    groups = ((0.1, 0.0), (0.2, 0.0), (0.1, 1e-2), (0.3, 5e-4), (0.1, 5e-4), (0.2, 1e-2))
    return sizes, groups, (False, True, True, True, True, True)


ZERO_W, ZERO_G = 4, 5


def arena_tensor(sizes, gen, zero=()):
    offs, total = ref.arena_layout(sizes)
    a = torch.zeros(total)
    for i, (o, n) in enumerate(zip(offs, sizes)):
        if i not in zero:
            a[o:o + n] = torch.randn(n, generator=gen)
    return a


class Arena:
    def __init__(self, pkg, seed, adapt=None):
        ops = pkg.engine.ops
        self.ops = ops
        self.sizes, groups, self.adapt = six(pkg)
        if adapt is not None:
            self.adapt = adapt
        self.offs, self.total = ref.arena_layout(self.sizes)
        self.gen = torch.Generator().manual_seed(seed)
        self.clr = torch.tensor(ref.chunk_table(self.sizes, [g[0] for g in groups]), dtype=torch.float32, device=DEV)
        self.cwd = torch.tensor(ref.chunk_table(self.sizes, [g[1] for g in groups]), dtype=torch.float32, device=DEV)
        first = np.array(self.offs) // ref.CHUNK
        self.lr, self.wd = f64(self.clr)[first], f64(self.cwd)[first]      # per tensor, as the kernel reads them
        self.plan = ops.LarsPlan(self.offs, self.sizes, self.total, DEV)
        assert self.plan.n_jobs == 8 and self.plan.n_params == 6
        self.plan.adapt.copy_(torch.tensor([int(a) for a in self.adapt], dtype=torch.int32))
        self.p = arena_tensor(self.sizes, self.gen, zero=(ZERO_W,)).to(DEV)
        self.buf = torch.zeros_like(self.p)
        self.pad = torch.from_numpy(ref.padding_mask(self.sizes)).to(DEV)

    def grad(self):
        return arena_tensor(self.sizes, self.gen, zero=(ZERO_G,)).to(DEV)

    def step(self, grad, nesterov, rec=None):
        self.ops.lars_step(self.p, grad, self.buf, self.clr, self.cwd, self.plan, MOM, nesterov, TAU, EPS, rec)
        torch.cuda.synchronize()


@pytest.mark.parametrize('nesterov', [False, True], ids=['plain', 'nesterov'])
def test_kernels_vs_specification(pkg, nesterov):
    a = Arena(pkg, 21 + nesterov)

    def one(tag, clip=None, coef=1.0, skip=False):
        grad = a.grad()
        before = (a.p.clone(), a.buf.clone())
        kept = (a.plan.trust.clone(), a.plan.norms.clone(), a.plan.chunk_trust.clone())
        rec = None if clip is None else torch.tensor(clip, dtype=torch.float32, device=DEV)
        a.step(grad, nesterov, rec)
        q = assert_step(tag, before, (a.p, a.buf), grad, a.sizes, a.lr, a.wd, a.adapt, a.plan.trust, a.plan.norms, nesterov,
                        coef, skip)
        for name, buf in (('p', a.p), ('buf', a.buf)):
            assert not buf[a.pad].any(), (tag, name, 'padding moved')
        if skip:                                         # the last trust record is kept
            for x, y in zip(kept, (a.plan.trust, a.plan.norms, a.plan.chunk_trust)):
                assert torch.equal(bits(x), bits(y)), tag
        else:                                            # the per-chunk table the update read is the per-tensor record
            want = torch.from_numpy(ref.chunk_table(a.sizes, f64(a.plan.trust))).float().to(DEV)
            assert torch.equal(bits(a.plan.chunk_trust), bits(want)), tag
        return q

    q = one('t=1')
    assert q[0] == 1.0 and q[ZERO_W] == 1.0 and q[ZERO_G] == 1.0 and all(0.0 < q[i] < 1.0 for i in (1, 2, 3))
    assert float(a.plan.trust[ZERO_W]) == 1.0 and float(a.plan.norms[ZERO_W, 0]) == 0.0 and float(a.plan.norms[ZERO_G, 1]) == 0.0
    q = one('t=2')
    assert q[ZERO_W] < 1.0                               # its weights have moved off zero
    one('t=3')
    q = one('clip 0.5', clip=(7.0, 0.5, 0.0, 0.0), coef=0.5)
    one('skip', clip=(float('inf'), 0.0, 1.0, 1024.0), skip=True)
    one('after skip')


@pytest.mark.parametrize('nesterov', [False, True], ids=['plain', 'nesterov'])
def test_step_is_deterministic_and_sgd_where_not_adapted(pkg, nesterov):
    """The same step twice from copies of the same state: every output bit-equal (data-parallel replicas rely on it).  And where
    no trust ratio applies -- the tensor that is not adapted, zero weights, zero gradient; then the whole arena with every adapt
    flag cleared -- the result is gca_sgd_step's on the same tables, bit for bit."""
    a = Arena(pkg, 31)
    a.buf.copy_(arena_tensor(a.sizes, a.gen))            # a momentum state, so that momentum * buf is in the sum
    grad = a.grad()
    rec = torch.tensor((3.0, 0.7, 0.0, 0.0), dtype=torch.float32, device=DEV)
    p0, b0 = a.p.clone(), a.buf.clone()
    outs = []
    for _ in range(2):
        a.p.copy_(p0)
        a.buf.copy_(b0)
        a.plan.partials.zero_()
        a.plan.norms.zero_()
        a.plan.trust.fill_(-1.0)
        a.plan.chunk_trust.fill_(-1.0)
        a.step(grad, nesterov, rec)
        outs.append([t.clone() for t in (a.p, a.buf, a.plan.trust, a.plan.norms, a.plan.chunk_trust, a.plan.partials)])
    for x, y in zip(*outs):
        assert torch.equal(bits(x), bits(y))
    ps, bs = p0.clone(), b0.clone()
    a.ops.sgd_step(ps, grad, bs, a.clr, a.cwd, 1.0, MOM, nesterov, rec)
    torch.cuda.synchronize()
    for i in (0, ZERO_W, ZERO_G):
        o, n = a.offs[i], a.sizes[i]
        assert float(a.plan.trust[i]) == 1.0
        assert torch.equal(bits(a.p[o:o + n]), bits(ps[o:o + n])) and torch.equal(bits(a.buf[o:o + n]), bits(bs[o:o + n])), i
    o, n = a.offs[3], a.sizes[3]
    assert not torch.equal(a.p[o:o + n], ps[o:o + n])
    b = Arena(pkg, 31, adapt=(False,) * 6)
    b.p.copy_(p0)
    b.buf.copy_(b0)
    b.step(grad, nesterov, rec)
    assert torch.equal(bits(b.p), bits(ps)) and torch.equal(bits(b.buf), bits(bs))
    assert bool((b.plan.trust == 1.0).all()) and bool((b.plan.norms[:4] > 0).all())


def test_ops_wrapper_refuses_misuse(pkg):
    ops = pkg.engine.ops
    z = torch.zeros(512, device=DEV)
    c = torch.zeros(2, device=DEV)
    plan = ops.LarsPlan([0, 256], [256, 3], 512, DEV)
    with pytest.raises(ValueError):                      # the plan is another arena's
        ops.lars_step(z[:256], z[:256], z[:256].clone(), c[:1], c[:1], plan, 0.9, False, TAU, EPS)
    for mom, tau, eps in ((1.0, TAU, EPS), (0.9, 0.0, EPS), (0.9, TAU, -1.0)):       # GCA_EINVAL
        with pytest.raises(RuntimeError):
            ops.lars_step(z, z, z.clone(), c, c, plan, mom, False, tau, eps)


# ----------------------------------------------------------------------------- 2. HipLARS and its wire format
class Six(torch.nn.Module):
    """The six tensors as a module's parameters: `ndim > 1` decides what is adapted."""

    def __init__(self, pkg, seed):
        super().__init__()
        J = pkg._hip.lib.gca_lars_job_chunks()
        gen = torch.Generator().manual_seed(seed)
        shapes = ((1,), (5, 51), (1, 700), (2, J * 256 + 150), (16, 16), (3, 100))
        self.w = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator=gen)) for s in shapes])
        with torch.no_grad():
            self.w[ZERO_W].zero_()


def hip_lars(pkg, model, **kw):
    _, groups, _ = six(pkg)
    return pkg.lib.solver.HipLARS(model, [{'params': [p], 'lr': lr, 'weight_decay': wd, 'name': n}
                                          for (n, p), (lr, wd) in zip(model.named_parameters(), groups)], **kw)


def set_grads(params, gen):
    for i, p in enumerate(params):
        p.grad.copy_(torch.zeros(p.shape) if i == ZERO_G else torch.randn(p.shape, generator=gen))


def per_tensor(opt):
    first = torch.tensor(opt.arena.offsets) // ref.CHUNK
    return f64(opt.chunk_lr)[first], f64(opt.chunk_wd)[first], [bool(g['lars_adapt']) for g in opt.param_groups]


def test_hip_lars_wire_format(pkg):
    gen = torch.Generator().manual_seed(41)
    model = Six(pkg, 1).to(DEV)
    opt = hip_lars(pkg, model, momentum=MOM, nesterov=True, trust_coef=TAU, eps=EPS)
    sizes, groups, adapt = six(pkg)
    assert tuple(opt.arena.sizes) == sizes and opt.plan.adapt.tolist() == [int(x) for x in adapt]
    params = list(model.parameters())
    for t in range(2):
        opt.zero_grad()
        set_grads(params, gen)
        before = (opt.arena.flat.clone(), opt.buf.clone())
        opt.step()
        torch.cuda.synchronize()
        lr, wd, ad = per_tensor(opt)
        assert_step('HipLARS t=%d' % (t + 1), before, (opt.arena.flat, opt.buf), opt.arena.grad, sizes, lr, wd, ad, opt.trust,
                    opt.norms, nesterov=True)
    sd = opt.state_dict()
    assert set(sd) == {'state', 'param_groups'} and list(sd['state']) == list(range(6))
    for i, g in enumerate(sd['param_groups']):
        assert g['params'] == [i] and (g['lr'], g['weight_decay']) == groups[i] and g['initial_lr'] == g['lr']
        assert (g['momentum'], g['nesterov'], g['trust_coef'], g['lars_eps'], g['lars_adapt']) == (MOM, True, TAU, EPS, adapt[i])
    for i, st in sd['state'].items():
        assert set(st) == {'momentum_buffer'} and st['momentum_buffer'].shape == params[i].shape
    # through the file format into a fresh HipLARS built with other settings: the loaded groups decide
    f = io.BytesIO()
    torch.save(sd, f)
    sd2 = torch.load(io.BytesIO(f.getvalue()), map_location='cpu', weights_only=False)
    model2 = Six(pkg, 2).to(DEV)
    with torch.no_grad():
        for q, p in zip(model2.parameters(), params):
            q.copy_(p)
    opt2 = hip_lars(pkg, model2, momentum=0.5, nesterov=False, trust_coef=0.01, eps=1e-6)
    opt2.load_state_dict(sd2)
    assert (opt2.momentum, opt2.nesterov, opt2.trust_coef, opt2.eps) == (MOM, True, TAU, EPS)
    assert torch.equal(bits(opt2.buf), bits(opt.buf)) and torch.equal(bits(opt2.arena.flat), bits(opt.arena.flat))
    sd3 = opt2.state_dict()
    assert all(torch.equal(bits(sd['state'][i]['momentum_buffer']), bits(sd3['state'][i]['momentum_buffer'])) for i in range(6))
    assert [{k: v for k, v in g.items()} for g in sd3['param_groups']] == sd['param_groups']
    opt.zero_grad()
    opt2.zero_grad()
    set_grads(params, gen)
    opt2.arena.grad.copy_(opt.arena.grad)
    opt.step()
    opt2.step()
    torch.cuda.synchronize()
    for x, y in ((opt.arena.flat, opt2.arena.flat), (opt.buf, opt2.buf), (opt.trust, opt2.trust), (opt.norms, opt2.norms)):
        assert torch.equal(bits(x), bits(y))
    # into torch.optim.SGD over the same parameters
    tparams = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    topt = torch.optim.SGD([{'params': [p]} for p in tparams], lr=0.5, momentum=0.1)
    topt.load_state_dict(sd)
    for i, tp in enumerate(tparams):
        assert torch.equal(topt.state[tp]['momentum_buffer'], sd['state'][i]['momentum_buffer'].cpu())
    assert topt.param_groups[3]['lr'] == groups[3][0] and topt.param_groups[0]['momentum'] == MOM
    # an SGD run resumes under LARS; Adam's format is refused
    m3 = Six(pkg, 3).to(DEV)
    sgd = pkg.lib.solver.HipSGD(m3, [{'params': [p], 'lr': 0.1, 'weight_decay': 0.0} for p in m3.parameters()])
    sgd.buf.fill_(0.25)
    opt2.load_state_dict(sgd.state_dict())
    o, n = opt2.arena.offsets[3], opt2.arena.sizes[3]
    assert bool((opt2.buf[o:o + n] == 0.25).all()) and not opt2.buf[o + n:o + n + 200].any() and opt2.trust_coef == TAU
    assert [g['lars_adapt'] for g in opt2.param_groups] == list(adapt) and opt2.param_groups[3]['lr'] == 0.1
    m4 = Six(pkg, 4).to(DEV)
    adam = pkg.lib.solver.HipAdam(m4, [{'params': [p], 'lr': 0.1, 'weight_decay': 0.0} for p in m4.parameters()])
    with pytest.raises(ValueError, match='momentum_buffer.*exp_avg'):
        opt2.load_state_dict(adam.state_dict())


# ----------------------------------------------------------------------------- 3. trainer wiring, by decomposition
def checked_step(tag, tr, run, record=None):
    """One train_step with the update decomposed: the gradient arena still holds this step's gradients afterwards, so the
    parameters and the momentum must be the specification applied to the state before the step with exactly those gradients.
    record: 'clip' when the step hands a (norm, coef, skip, -) record to the update (out['grad_norm']).  -> out"""
    opt = tr.optimizer
    before = (opt.arena.flat.clone(), opt.buf.clone())
    out = run()
    torch.cuda.synchronize()
    coef = 1.0
    if record is not None:
        rec = out['grad_norm'].cpu()
        coef = float(rec[1])
        assert 0.0 < coef < 1.0 and float(rec[2]) == 0.0, rec
    lr, wd, adapt = per_tensor(opt)
    assert np.array_equal(lr, np.array([np.float32(g['lr']) for g in opt.param_groups], dtype=np.float64))
    assert adapt == [p.ndim > 1 for p in opt.arena.params] and any(adapt) and not all(adapt)
    assert bool(opt.arena.grad.abs().max() > 0)
    q = assert_step(tag, before, (opt.arena.flat, opt.buf), opt.arena.grad, opt.arena.sizes, lr, wd, adapt, opt.trust, opt.norms,
                    bool(opt.nesterov), coef, mom=opt.momentum, tau=opt.trust_coef, eps=opt.eps)
    assert all(q[i] == 1.0 for i, a in enumerate(adapt) if not a) and any(q[i] != 1.0 for i, a in enumerate(adapt) if a)
    return out


def moco_cfg(pkg, parity, **solver):
    parity.register_tiny(pkg)
    solver.setdefault('OPTIMIZER_NAME', 'LARS')
    solver.setdefault('BASE_LR', 0.3)
    return parity.make_cfg(pkg, 'R2P1D10T', 'moco', 32, 20, 8, **solver)


def clips(seed, n=4, c=6):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(8, c, 8, 48, 48, generator=gen).to(DEV) for _ in range(n)]


@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'graph'])
def test_moco_trainer_steps(pkg, use_graph):
    """Eager: two steps.  With use_graph: four -- eager, eager, capture, replay -- so the three launches are captured and the
    replay reads the norms of its own gradients."""
    from tests import parity
    tr = pkg.MoCoTrainer(moco_cfg(pkg, parity), DEV, use_graph=use_graph, seed=5)
    assert type(tr.optimizer).__name__ == 'HipLARS' and tr.optimizer.trust_coef == 0.001 and tr.optimizer.eps == 1e-8
    seen = []
    for t, x in enumerate(clips(3, 4 if use_graph else 2), 1):
        checked_step('moco %s t=%d' % ('graph' if use_graph else 'eager', t), tr, lambda: tr.train_step(x))
        seen.append(tr.optimizer.norms[:, 1].clone())
    assert not torch.equal(seen[-1], seen[-2])
    if use_graph:
        assert tr._segments[0].graph is not None
    tr.close()


def test_moco_trainer_clipped(pkg):
    """CLIP_GRADIENT small enough to bite: the clip coefficient enters the trust ratio."""
    from tests import parity
    tr = pkg.MoCoTrainer(moco_cfg(pkg, parity, CLIP_GRADIENT=0.01, NESTEROV=True), DEV, use_graph=False, seed=5)
    assert tr.optimizer.nesterov is True
    for t, x in enumerate(clips(4, 2), 1):
        checked_step('moco clipped t=%d' % t, tr, lambda: tr.train_step(x), record='clip')
    tr.close()


def test_simsiam_trainer_step(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'simsiam', 32, 16, 8, OPTIMIZER_NAME='LARS', BASE_LR=0.3)
    tr = pkg.SimSiamTrainer(cfg, DEV, use_graph=False, seed=11)
    assert type(tr.optimizer).__name__ == 'HipLARS'
    x = clips(7, 1)[0]
    checked_step('simsiam t=1', tr, lambda: tr.train_step(x))
    tr.close()


def action_cfg(pkg, parity, probe, **solver):
    """The tiny model and config of tests/test_gpu_classify.py's action_cfg."""
    parity.register_tiny(pkg)
    cm.register()
    cfg = parity.make_cfg(pkg, cm.BACKBONE, 'moco', 32, 20, cm.T, **solver)
    cfg.merge_from_list(['DATASET.NUM_CLASS', cm.NUM_CLASS, 'MODEL.DROPOUT', 0.0, 'MODEL.LINEAR_PROBE', probe,
                         'SOLVER.NO_PARTIALBN', True])
    return cfg


LABELS = torch.tensor([0, 3, 6, 1, 2, 5, 4, 3])


def test_action_trainer_linear_probe_step(pkg):
    from tests import parity
    tr = pkg.ActionTrainer(action_cfg(pkg, parity, True, OPTIMIZER_NAME='LARS', BASE_LR=0.3), DEV, seed=43)
    opt = tr.optimizer
    assert type(opt).__name__ == 'HipLARS'
    assert [g['name'] for g in opt.param_groups] == ['base_model.fc.weight', 'base_model.fc.bias']
    assert [g['lars_adapt'] for g in opt.param_groups] == [True, False]
    frozen = {k: v.clone() for k, v in tr.model.named_parameters() if not k.startswith('base_model.fc.')}
    x = clips(9, 1, 3)[0]
    checked_step('action probe t=1', tr, lambda: tr.train_step(x, LABELS))
    for k, v in tr.model.named_parameters():
        if k in frozen:
            assert torch.equal(v, frozen[k]), k
    with pytest.raises(NotImplementedError, match='SGD, Adam, AdamW, LARS'):
        pkg.ActionTrainer(action_cfg(pkg, parity, True, OPTIMIZER_NAME='RMSprop'), DEV)


# ----------------------------------------------------------------------------- 4. checkpoint
def test_moco_lars_checkpoint_resume_is_exact(pkg):
    """Two steps on `a`, its state_dict through the file format into a fresh trainer `b` built with another seed, then one more
    step on both: loss, parameters, momentum, trust ratios and norms bit-identical."""
    from tests import parity
    cfg = moco_cfg(pkg, parity)
    xs = clips(15, 3)
    a = pkg.MoCoTrainer(cfg, DEV, use_graph=False, seed=5)
    for x in xs[:2]:
        a.train_step(x)
    f = io.BytesIO()
    torch.save(a.state_dict(epoch=7), f)
    b = pkg.MoCoTrainer(cfg, DEV, use_graph=False, seed=99)
    assert b.load_state_dict(torch.load(io.BytesIO(f.getvalue()), map_location='cpu', weights_only=False)) == 7
    oa, ob = a.train_step(xs[2]), b.train_step(xs[2])
    torch.cuda.synchronize()
    assert torch.equal(bits(oa['loss']), bits(ob['loss']))
    for x, y in ((a.optimizer.arena.flat, b.optimizer.arena.flat), (a.optimizer.buf, b.optimizer.buf),
                 (a.optimizer.trust, b.optimizer.trust), (a.optimizer.norms, b.optimizer.norms)):
        assert torch.equal(bits(x), bits(y))
    assert [g['lr'] for g in a.optimizer.param_groups] == [g['lr'] for g in b.optimizer.param_groups]
    a.close()
    b.close()
