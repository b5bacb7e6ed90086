"""Adam / AdamW on the device: gca_adam_step against the fp64 specification (tests/adam_ref.py), HipAdam's wire format
against torch.optim.Adam / AdamW, the trainers' wiring by decomposition, and checkpoints (SimSiam's included).

The error bar.  Every comparison of a kernel result with the specification is per element

    |got - want| <= k * 2^-24 * max(|want|, |update|)

with |update| from adam_ref.update_magnitude (the step with every term replaced by its absolute value: what a rounding of any
term is relative to) and k the number of fp32 roundings on the kernel's own path to the value, counted without crediting
fused multiply-adds.  The specification is applied to the kernel's own state before the step and to the chunk tables as the
kernel reads them (fp32), so the state and the tables carry no rounding of their own:

    g   (3)  grad * coef (1); under Adam wd * p (1) and the sum (1)
    m   (8)  g (3), (float)beta1 (1), (float)(1 - beta1) (1), beta1 * m (1), (1 - beta1) * g (1), the sum (1)
    v  (12)  g * g carries g twice (6) and its own rounding (1), (float)(1 - beta2) (1), its product (1), (float)beta2 (1),
             beta2 * v (1), the sum (1)
    p  (27)  under AdamW lr * wd, 1 - that, p * that (3); step size (float)(1 / bc1) and lr * that (2); denominator: sqrt of v
             halves v's 12 (6), sqrtf (1), (float)(1 / sqrt(bc2)) (1), their product (1), (float)eps (1), the sum (1); m (8);
             the quotient (1), step size * quotient (1), the difference (1)

(bc = 1 - beta^t comes from fp64 inside the kernel: its error is below 1e-13 relative and counts as none.)"""
import copy
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as ref                   # noqa: E402
import classify_model as cm              # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
K_P, K_M, K_V = 27, 8, 12
EPS32 = 2.0 ** -24
BETAS, EPS = (0.9, 0.999), 1e-8


def f64(t):
    return t.detach().double().cpu().numpy()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def assert_step(tag, before, after, grad, t, lr, wd, decoupled, coef=1.0, skip=False):
    """before / after: (p, m, v) device tensors around one kernel step t; lr / wd: per-ELEMENT fp64 arrays."""
    p0, m0, v0 = (f64(a) for a in before)
    g = f64(grad)
    want = ref.adam_step(p0, g, m0, v0, t, lr, wd, BETAS, EPS, decoupled, coef, skip)
    upd = want if skip else ref.update_magnitude(p0, g, m0, v0, t, lr, wd, BETAS, EPS, decoupled, coef)
    worst = {}
    for name, k, got, w, u in zip('pmv', (K_P, K_M, K_V), after, want, upd):
        if skip:
            assert torch.equal(bits(got), bits(before['pmv'.index(name)])), (tag, name)
            continue
        err = np.abs(f64(got) - w)
        scale = np.maximum(np.abs(w), u)
        ulps = err / np.maximum(EPS32 * scale, 1e-300)
        worst[name] = float(ulps.max())
        bad = err > k * EPS32 * scale
        assert not bad.any(), (tag, name, 'worst %.2f roundings (bar %d) at %d' % (ulps.max(), k, int(ulps.argmax())))
    print('MEASURED %s: worst error in roundings p %s m %s v %s (bars %d / %d / %d)'
          % (tag, *('%.2f' % worst.get(n, 0.0) for n in 'pmv'), K_P, K_M, K_V))


# ----------------------------------------------------------------------------- 1. kernel against the specification
SIZES = (1, 255, 700)
GROUPS = ((1e-3, 0.0), (2e-3, 5e-4), (1e-3, 1e-2))


def arena_tensor(gen, special=False):
    """Seeded normal values in the three tensors' places, exact zeros in the padding; special: a few exact zeros and a few
    values at 1e-12 (below eps) among them."""
    offs, total = ref.arena_layout(SIZES)
    a = torch.zeros(total)
    for o, n in zip(offs, SIZES):
        a[o:o + n] = torch.randn(n, generator=gen)
    if special:
        for o, n in zip(offs[1:], SIZES[1:]):
            a[o + 3], a[o + 100], a[o + n - 1] = 0.0, 0.0, 0.0
            a[o + 5], a[o + 101], a[o + n - 2] = 1e-12, -1e-12, 1e-12
    return a


@pytest.mark.parametrize('decoupled', [False, True], ids=['adam', 'adamw'])
def test_kernel_vs_specification(pkg, decoupled):
    ops = pkg.engine.ops
    gen = torch.Generator().manual_seed(21 + decoupled)
    offs, total = ref.arena_layout(SIZES)
    assert total == 1280 and offs == [0, 256, 512]
    pad = torch.from_numpy(ref.padding_mask(SIZES)).to(DEV)
    clr = torch.tensor(ref.chunk_table(SIZES, [g[0] for g in GROUPS]), dtype=torch.float32, device=DEV)
    cwd = torch.tensor(ref.chunk_table(SIZES, [g[1] for g in GROUPS]), dtype=torch.float32, device=DEV)
    lr, wd = f64(clr).repeat(ref.CHUNK), f64(cwd).repeat(ref.CHUNK)           # the tables as the kernel reads them
    p = arena_tensor(gen).to(DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    steps = torch.zeros(1, dtype=torch.int64, device=DEV)

    def one(tag, t, clip=None, coef=1.0, skip=False):
        grad = arena_tensor(gen, special=True).to(DEV)
        before = (p.clone(), m.clone(), v.clone())
        rec = None if clip is None else torch.tensor(clip, dtype=torch.float32, device=DEV)
        ops.adam_step(p, grad, m, v, clr, cwd, BETAS[0], BETAS[1], EPS, decoupled, steps, rec)
        torch.cuda.synchronize()
        assert_step(tag, before, (p, m, v), grad, t, lr, wd, decoupled, coef, skip)
        for name, buf in zip('pmv', (p, m, v)):
            assert not buf[pad].any(), (tag, name, 'padding moved')
        assert int(steps) == (t - 1 if skip else t), (tag, int(steps))

    for t in (1, 2, 3):                                  # from zero state: where the bias corrections move most
        one('t=%d' % t, t)
    steps.fill_(9999)
    one('t=10000', 10000)
    one('clip 0.5', 10001, clip=(7.0, 0.5, 0.0, 0.0), coef=0.5)
    one('skip', 10002, clip=(float('inf'), 0.0, 1.0, 1024.0), skip=True)
    one('after skip', 10002)                             # the skipped step was not counted


def test_ops_wrapper_refuses_misuse(pkg):
    ops = pkg.engine.ops
    z = torch.zeros(256, device=DEV)
    c = torch.zeros(1, device=DEV)
    with pytest.raises(TypeError):                       # the step count is an int64 record
        ops.adam_step(z, z, z.clone(), z.clone(), c, c, 0.9, 0.999, 1e-8, False, torch.zeros(1, device=DEV))
    with pytest.raises(RuntimeError):                    # n % 256 != 0: GCA_EINVAL
        ops.adam_step(z[:252], z[:252], z[:252].clone(), z[:252].clone(), c, c, 0.9, 0.999, 1e-8, False,
                      torch.zeros(1, dtype=torch.int64, device=DEV))


# ----------------------------------------------------------------------------- 2. wire format
def small_model(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))


SMALL_GROUPS = ((1e-3, 1e-2), (2e-3, 0.0), (1e-3, 5e-4), (3e-3, 0.0))


def hip_adam(pkg, model, decoupled):
    groups = [{'params': [p], 'lr': lr, 'weight_decay': wd, 'name': n}
              for (n, p), (lr, wd) in zip(model.named_parameters(), SMALL_GROUPS)]
    return pkg.lib.solver.HipAdam(model, groups, decoupled=decoupled)


def set_grads(params, gen):
    """Seeded gradients written into the arena views the device parameters' .grad point at; -> the host copies."""
    gs = [torch.randn(p.shape, generator=gen) for p in params]
    for p, g in zip(params, gs):
        p.grad.copy_(g)
    return gs


def element_tables(opt):
    return f64(opt.chunk_lr).repeat(ref.CHUNK), f64(opt.chunk_wd).repeat(ref.CHUNK)


def assert_matches_torch(tag, opt, before, tparams, topt, t, decoupled):
    """HipAdam's arena after step t against a CPU fp32 torch optimizer's parameters and state after the same step, at the
    bar of the kernel test (scales from the specification on HipAdam's state before the step)."""
    a = opt.arena
    p0, m0, v0 = (f64(x) for x in before)
    lr, wd = element_tables(opt)
    upd = ref.update_magnitude(p0, f64(a.grad), m0, v0, t, lr, wd, BETAS, EPS, decoupled)
    for name, k, got, u in zip('pmv', (K_P, K_M, K_V), (a.flat, opt.exp_avg, opt.exp_avg_sq), upd):
        got = f64(got)
        for o, n, tp in zip(a.offsets, a.sizes, tparams):
            want = {'p': tp, 'm': topt.state[tp]['exp_avg'], 'v': topt.state[tp]['exp_avg_sq']}[name]
            want = want.detach().double().reshape(-1).numpy()
            err = np.abs(got[o:o + n] - want)
            bar = k * EPS32 * np.maximum(np.abs(want), u[o:o + n])
            assert (err <= bar).all(), (tag, name, float((err / np.maximum(bar / k, 1e-300)).max()))


@pytest.mark.parametrize('decoupled', [False, True], ids=['adam', 'adamw'])
def test_wire_format_round_trip_with_torch(pkg, decoupled):
    gen = torch.Generator().manual_seed(31)
    model = small_model(1).to(DEV)
    opt = hip_adam(pkg, model, decoupled)
    params = list(model.parameters())
    for _ in range(3):
        opt.zero_grad()
        set_grads(params, gen)
        opt.step()
    sd = opt.state_dict()
    assert set(sd) == {'state', 'param_groups'} and list(sd['state']) == [0, 1, 2, 3]
    for i, g in enumerate(sd['param_groups']):
        assert g['params'] == [i] and g['betas'] == BETAS and g['eps'] == EPS and g['amsgrad'] is False
        assert (g['lr'], g['weight_decay']) == SMALL_GROUPS[i] and g['initial_lr'] == g['lr']
    for i, st in sd['state'].items():
        assert set(st) == {'step', 'exp_avg', 'exp_avg_sq'} and st['exp_avg'].shape == params[i].shape
        assert st['step'].dtype is torch.float32 and st['step'].dim() == 0 and float(st['step']) == 3.0
    # HipAdam -> torch
    tparams = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    topt = cls([{'params': [p]} for p in tparams], lr=0.5, weight_decay=0.5)
    topt.load_state_dict(sd)
    for i, tp in enumerate(tparams):
        assert torch.equal(topt.state[tp]['exp_avg'], sd['state'][i]['exp_avg'].cpu()) and float(topt.state[tp]['step']) == 3.0
    opt.zero_grad()
    gs = set_grads(params, gen)
    for tp, g in zip(tparams, gs):
        tp.grad = g.clone()
    before = (opt.arena.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone())
    opt.step()
    topt.step()
    torch.cuda.synchronize()
    assert_matches_torch('hip -> torch, step 4', opt, before, tparams, topt, 4, decoupled)
    # torch -> a fresh HipAdam
    model2 = small_model(2).to(DEV)
    with torch.no_grad():
        for q, tp in zip(model2.parameters(), tparams):
            q.copy_(tp)
    opt2 = hip_adam(pkg, model2, not decoupled)          # the loaded groups decide, not the constructor
    opt2.load_state_dict(topt.state_dict())
    assert int(opt2.steps) == 4 and opt2.decoupled is decoupled and opt2.betas == BETAS and opt2.eps == EPS
    for o, n, tp in zip(opt2.arena.offsets, opt2.arena.sizes, tparams):
        assert torch.equal(opt2.exp_avg[o:o + n].cpu(), topt.state[tp]['exp_avg'].reshape(-1))
        assert torch.equal(opt2.exp_avg_sq[o:o + n].cpu(), topt.state[tp]['exp_avg_sq'].reshape(-1))
    params2 = list(model2.parameters())
    opt2.zero_grad()
    gs = set_grads(params2, gen)
    for tp, g in zip(tparams, gs):
        tp.grad = g.clone()
    before = (opt2.arena.flat.clone(), opt2.exp_avg.clone(), opt2.exp_avg_sq.clone())
    opt2.step()
    topt.step()
    torch.cuda.synchronize()
    assert_matches_torch('torch -> hip, step 5', opt2, before, tparams, topt, 5, decoupled)
    assert float(opt2.state_dict()['state'][0]['step']) == 5.0
    # formats do not cross (device-side buffers)
    model3 = small_model(3).to(DEV)
    sgd = pkg.lib.solver.HipSGD(model3, [{'params': [p], 'lr': 0.1, 'weight_decay': 0.0} for p in model3.parameters()])
    with pytest.raises(ValueError, match='momentum_buffer.*exp_avg'):
        sgd.load_state_dict(opt.state_dict())
    with pytest.raises(ValueError, match='momentum_buffer.*exp_avg'):
        opt.load_state_dict(sgd.state_dict())


# ----------------------------------------------------------------------------- 3. trainer wiring, by decomposition
def snapshot(opt):
    return (opt.arena.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()), int(opt.steps)


def checked_step(tag, tr, run, decoupled=False, record=None):
    """One train_step with the update decomposed: the gradient arena still holds this step's gradients afterwards, so the
    parameters and moments must be the specification applied to the state before the step with exactly those gradients.
    record: 'clip' / 'scale' when the step hands a (norm, coef, skip, -) record to the update (out['grad_norm']): its
    coefficient and skip flag go into the specification.  -> (out, skipped?)"""
    opt = tr.optimizer
    before, t0 = snapshot(opt)
    out = run()
    torch.cuda.synchronize()
    coef, skip = 1.0, False
    if record is not None:
        rec = out['grad_norm'].cpu()
        coef, skip = float(rec[1]), float(rec[2]) != 0.0
        if record == 'clip':
            assert 0.0 < coef < 1.0 and not skip, rec
    lr, wd = element_tables(opt)
    groups = opt.param_groups
    assert np.array_equal(lr[np.array(opt.arena.offsets)], np.array([np.float32(g['lr']) for g in groups], dtype=np.float64))
    assert int(opt.steps) == (t0 if skip else t0 + 1), (tag, int(opt.steps))
    assert skip or bool(opt.arena.grad.abs().max() > 0)
    assert_step(tag, before, (opt.arena.flat, opt.exp_avg, opt.exp_avg_sq), opt.arena.grad, t0 + 1, lr, wd, decoupled, coef, skip)
    return out, skip


def moco_cfg(pkg, parity, **solver):
    parity.register_tiny(pkg)
    solver.setdefault('OPTIMIZER_NAME', 'Adam')
    return parity.make_cfg(pkg, 'R2P1D10T', 'moco', 32, 20, 8, BASE_LR=1e-3, **solver)


def clips(seed, n=4, c=6):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(8, c, 8, 48, 48, generator=gen).to(DEV) for _ in range(n)]


@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'graph'])
def test_moco_trainer_steps(pkg, use_graph):
    """Four steps; with use_graph they are eager, eager, capture, replay: the replay at t = 4 fails if the step count was baked
    into the graph."""
    from tests import parity
    tr = pkg.MoCoTrainer(moco_cfg(pkg, parity), DEV, use_graph=use_graph, seed=5)
    assert type(tr.optimizer).__name__ == 'HipAdam' and not tr.optimizer.decoupled
    for t, x in enumerate(clips(3), 1):
        checked_step('moco %s t=%d' % ('graph' if use_graph else 'eager', t), tr, lambda: tr.train_step(x))
    assert int(tr.optimizer.steps) == 4
    tr.close()


def test_moco_trainer_clipped(pkg):
    from tests import parity
    tr = pkg.MoCoTrainer(moco_cfg(pkg, parity, CLIP_GRADIENT=0.01), DEV, use_graph=False, seed=5)
    for t, x in enumerate(clips(4, 2), 1):
        checked_step('moco clipped t=%d' % t, tr, lambda: tr.train_step(x), record='clip')


def test_moco_trainer_schedule_under_graph(pkg):
    """The scheduler moves every group's lr between iterations (warm-up): the captured update must read the new tables."""
    from tests import parity
    tr = pkg.MoCoTrainer(moco_cfg(pkg, parity), DEV, use_graph=True, seed=5)
    seen = []
    for t, x in enumerate(clips(6), 1):
        checked_step('moco scheduled t=%d' % t, tr, lambda: tr.train_step(x))
        seen.append(tr.optimizer.param_groups[0]['lr'])
        tr.scheduler.step()
    assert len(set(seen)) == 4
    tr.close()


@pytest.mark.parametrize('kind', ['moco', 'simsiam'])
def test_fp16_storage_trainers_skip_and_step(pkg, kind, monkeypatch):
    """fp16 storage hands the update the record of gca_grad_unscale_clip (coefficient 1 / S, skip flag).  With a loss scale far
    too large (2^30) the first steps overflow: parameters, both moments and the step count stay bit-identical, hipGraph
    replays included; once the scale fits, every applied step is the specification with the coefficient of its record."""
    from tests import parity
    parity.register_tiny(pkg)
    ops = pkg.engine.ops
    monkeypatch.setenv('GCA_LOSS_SCALE', str(2.0 ** 30))
    default = ops.get_conv_math()
    ops.set_conv_math('fp16')
    try:
        if kind == 'moco':
            tr = pkg.MoCoTrainer(moco_cfg(pkg, parity), DEV, use_graph=True, seed=4)
        else:
            cfg = parity.make_cfg(pkg, 'R2P1D10T', 'simsiam', 32, 16, 8, OPTIMIZER_NAME='AdamW', BASE_LR=1e-3)
            tr = pkg.SimSiamTrainer(cfg, DEV, use_graph=True, seed=4)
        x = clips(2, 1)[0]
        skipped = applied = 0
        for step in range(40):
            _, skip = checked_step('%s fp16 step %d' % (kind, step), tr, lambda: tr.train_step(x), decoupled=kind == 'simsiam',
                                   record='scale')
            skipped, applied = skipped + skip, applied + (not skip)
            if applied >= 3:
                break
        assert skipped >= 3 and applied == 3 and int(tr.optimizer.steps) == 3, (skipped, applied)
        assert tr._segments[0].graph is not None
        sd = tr.state_dict()
        assert float(sd['loss_scale_state'][0]) == 2.0 ** 30 / 2.0 ** skipped and float(sd['loss_scale_state'][2]) == skipped
        tr.close()
    finally:
        ops.set_conv_math(default)


def test_simsiam_trainer_steps(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'simsiam', 32, 16, 8, OPTIMIZER_NAME='AdamW', BASE_LR=1e-3)
    tr = pkg.SimSiamTrainer(cfg, DEV, use_graph=True, seed=11)
    assert tr.optimizer.decoupled
    for t, x in enumerate(clips(7), 1):
        checked_step('simsiam adamw t=%d' % t, tr, lambda: tr.train_step(x), decoupled=True)
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


@pytest.mark.parametrize('probe,name', [(False, 'Adam'), (True, 'AdamW')], ids=['finetune-adam', 'probe-adamw'])
def test_action_trainer_steps(pkg, probe, name):
    from tests import parity
    tr = pkg.ActionTrainer(action_cfg(pkg, parity, probe, OPTIMIZER_NAME=name, BASE_LR=1e-3), DEV, seed=43)
    opt = tr.optimizer
    assert type(opt).__name__ == 'HipAdam' and opt.decoupled is (name == 'AdamW')
    if probe:
        assert [g['name'] for g in opt.param_groups] == ['base_model.fc.weight', 'base_model.fc.bias']
    else:
        assert len(opt.param_groups) == len(list(tr.model.parameters()))
    for t, x in enumerate(clips(9, 2, 3), 1):
        checked_step('action %s t=%d' % (name, t), tr, lambda: tr.train_step(x, LABELS), decoupled=name == 'AdamW')
    sd = tr.state_dict()
    assert float(sd['optimizer']['state'][0]['step']) == 2.0
    with pytest.raises(NotImplementedError, match='SGD, Adam, AdamW'):
        pkg.ActionTrainer(action_cfg(pkg, parity, probe, OPTIMIZER_NAME='RMSprop'), DEV)


# ----------------------------------------------------------------------------- 4. checkpoints
def optimizer_buffers(opt):
    if hasattr(opt, 'buf'):
        return [opt.buf]
    return [opt.exp_avg, opt.exp_avg_sq, opt.steps]


def assert_resume_is_exact(make, xs, keys):
    """Three steps on `a`, its state_dict through the file format into a fresh trainer `b` built with another seed, then two
    more steps on both: losses, parameters, BatchNorm buffers and optimizer state bit-identical."""
    a = make(5)
    for x in xs[:3]:
        a.train_step(x)
    sd = a.state_dict(epoch=7)
    assert set(sd) >= set(keys)
    buf = io.BytesIO()
    torch.save(sd, buf)
    b = make(99)
    assert b.load_state_dict(torch.load(io.BytesIO(buf.getvalue()), map_location='cpu', weights_only=False)) == 7
    for x in xs[3:]:
        oa, ob = a.train_step(x), b.train_step(x)
        torch.cuda.synchronize()
        assert torch.equal(bits(oa['loss']), bits(ob['loss']))
    sa, sb = a.model.state_dict(), b.model.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for x, y in zip(optimizer_buffers(a.optimizer), optimizer_buffers(b.optimizer)):
        assert torch.equal(x, y)
    assert [g['lr'] for g in a.optimizer.param_groups] == [g['lr'] for g in b.optimizer.param_groups]
    return a, b, sd


@pytest.mark.parametrize('name,lr', [('SGD', 0.06), ('Adam', 1e-3)])
def test_simsiam_checkpoint_resume_is_exact(pkg, name, lr):
    from tests import parity
    parity.register_tiny(pkg)
    cm.register()
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'simsiam', 32, 16, 8, OPTIMIZER_NAME=name, BASE_LR=lr)
    a, b, sd = assert_resume_is_exact(lambda seed: pkg.SimSiamTrainer(cfg, DEV, use_graph=False, seed=seed), clips(13, 5),
                                      ('epoch', 'state_dict', 'optimizer', 'contrast'))
    assert sd['contrast'] is None and 'model_ema' not in sd
    if name == 'Adam':
        assert int(a.optimizer.steps) == int(b.optimizer.steps) == 5
        return
    # the checkpoint is one "the pre-training trainers write": the action trainer and the retrieval loader take its encoder
    sd = copy.deepcopy(sd)
    tr = pkg.ActionTrainer(action_cfg(pkg, parity, False), DEV, seed=47)
    tr.load_pretrained(sd)
    n = 0
    for k, v in tr.model.state_dict().items():
        if not k.startswith('base_model.fc.'):
            src = [s for s in sd['state_dict'] if s.endswith('encoder.' + k)]
            assert len(src) == 1 and torch.equal(v, sd['state_dict'][src[0]].to(v.device)), k
            n += 1
    assert n == 126
    enc = pkg.lib.evaluation.load_encoder(sd, 'R2P1D10T', 8)
    assert not enc.training


def test_moco_adam_checkpoint_resume_is_exact(pkg):
    from tests import parity
    cfg = moco_cfg(pkg, parity)
    a, b, sd = assert_resume_is_exact(lambda seed: pkg.MoCoTrainer(cfg, DEV, use_graph=False, seed=seed), clips(15, 5),
                                      ('epoch', 'state_dict', 'optimizer', 'contrast', 'model_ema'))
    assert float(sd['optimizer']['state'][0]['step']) == 3.0 and int(a.optimizer.steps) == 5
    assert torch.equal(a.contrast.memory, b.contrast.memory)
    for (k, x), (_, y) in zip(a.model_ema.state_dict().items(), b.model_ema.state_dict().items()):
        assert torch.equal(x, y), k
