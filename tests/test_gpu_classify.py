"""gca_classifier_fwd / gca_classifier_bwd, the class-head model, ActionTrainer and the video-level test on the device.

Kernels: held to the fp64 specification tests/classify_ref.py.  On operands that are exact in fp32 the logits must be the
specification's bits and every output must repeat bit for bit.  On float operands the bars are the project's existing ones
(tests/test_gpu_edges.py, InfoNCE): logits 1e-5 relative max-norm; row_lse and loss within 1e-5 * max(max|logits|, ln C) of
the fp64 value of the kernel's OWN logits; rank_ge equal to the count on the kernel's own logits; gradients 1e-4 relative
max-norm.  Model / trainer: against the fp64 oracle of tests/classify_model.py at the model bar of 1e-3, gradients by
tests/parity.check_grad_errors.  Every measured error is printed with its bar (MEASURED ...).

Measured on an MI355X (worst over the eight float shapes; the bars in brackets):
    logits 9.7e-7 [1e-5]   row_lse 1.6e-6, loss 3.1e-6 on the +-160 logits [1.6e-3]; 1.1e-6 / 4.4e-7 elsewhere [1.9e-6 .. 8.4e-5]
    dw 7.1e-7, dbias 4.2e-7, dx 1.1e-6 [1e-4]   C = 1: exact zeros
    model logits 2.9e-6 (train) / 3.5e-7 (eval) [1e-3]   fine-tune step: loss 5.7e-8, logits 3.8e-6, buffers 1.2e-6 [1e-3],
    gradients median 3.1e-6 / worst 7.5e-6 [2e-4 / 1e-1]   linear probe: updated head 3.8e-7 [2e-4]
"""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import classify_model as cm              # noqa: E402
import classify_ref as ref               # noqa: E402
import ref64                             # noqa: E402
from conftest import rel_err             # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = -1


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def offset_copy(t, off):
    """A device copy of t whose base pointer is `off` floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=DEV)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * off) % 16 and v.is_contiguous()
    return v


# ----------------------------------------------------------------------------- exact operands
def exact_case():
    b, Fd, Cc = 33, 520, 130
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-32, 33, (b, Fd), generator=g).float() / 8
    w = torch.randint(-32, 33, (Cc, Fd), generator=g).float() / 8
    for dup, src in ((7, 3), (64, 3), (129, 100), (33, 32)):        # duplicate classes: tied logits in every row
        w[dup] = w[src]
    bias = torch.randint(-64, 65, (Cc,), generator=g).float() / 64
    for dup, src in ((7, 3), (64, 3), (129, 100), (33, 32)):
        bias[dup] = bias[src]
    t = torch.randint(0, Cc, (b,), generator=g)
    t[:4] = torch.tensor([3, 7, 64, 100])                           # targets among the tied classes
    return x, w, bias, t


def run_all(pkg, x, w, bias, t, want_dx=True):
    ops = pkg.engine.ops
    logits, lse, rank, loss = ops.classifier_fwd(x, w, bias, t)
    dw = torch.empty_like(w)
    db = None if bias is None else torch.empty_like(bias)
    dx = torch.empty_like(x) if want_dx else None
    ops.classifier_bwd(x, w, logits, lse, t, dw, db, False, dx, False)
    torch.cuda.synchronize()
    return dict(logits=logits, lse=lse, rank=rank, loss=loss, dw=dw, db=db, dx=dx)


def test_exact_operands_bitwise(pkg):
    x, w, bias, t = exact_case()
    want, _, _, wrank = ref.forward(x, w, bias, t)
    assert torch.equal(want.float().double(), want) and float(want.abs().max()) < 2 ** 14      # <= 20 significant bits
    a = run_all(pkg, x.to(DEV), w.to(DEV), bias.to(DEV), t.to(DEV))
    assert torch.equal(bits(a['logits']), bits(want.float()))
    assert torch.equal(a['rank'].cpu(), wrank) and int(wrank[:4].min()) >= 1                     # ties count against the target
    assert torch.equal(a['rank'].cpu().long(), ref64.rank_ge(a['logits'], t).long())
    b2 = run_all(pkg, x.to(DEV), w.to(DEV), bias.to(DEV), t.to(DEV))
    for k in a:
        assert torch.equal(bits(a[k]), bits(b2[k])), k
    assert all(bool(torch.isfinite(v.float()).all()) for v in a.values())


# ----------------------------------------------------------------------------- float operands
FLOAT_CASES = [
    # b, F, C, bias, dx, accumulate, gscale_dev, offset, wide
    (1, 512, 101, True, True, False, False, False, False),
    (3, 1024, 51, False, True, True, True, False, False),
    (32, 2048, 400, True, True, False, False, True, False),
    (33, 518, 5, True, False, True, False, False, False),
    (2, 512, 1, True, True, False, True, False, False),
    (65, 100, 1000, False, True, False, False, True, False),
    (129, 36, 130, True, True, True, True, True, False),
    (8, 512, 101, True, True, False, False, False, True),
]


@pytest.mark.parametrize('b,Fd,Cc,has_bias,want_dx,acc,gs,off,wide', FLOAT_CASES)
def test_float_operands(pkg, b, Fd, Cc, has_bias, want_dx, acc, gs, off, wide):
    ops = pkg.engine.ops
    g = torch.Generator().manual_seed(1000 * b + Cc)
    x = torch.randn(b, Fd, generator=g).abs()                        # pooled post-ReLU features
    w = torch.randn(Cc, Fd, generator=g) * 0.05
    bias = torch.randn(Cc, generator=g) * 0.1 if has_bias else None
    t = torch.randint(0, Cc, (b,), generator=g)
    if wide:
        w *= 160.0 / float(ref.logits(x, w, bias).abs().max())
    wl, wlse, wloss, _ = ref.forward(x, w, bias, t)
    if wide:
        assert float(wl.max()) > 100 and float(wl.min()) < -100
    scale_dev, scale_host = (torch.tensor([0.5], device=DEV), 3.0) if gs else (None, 1.0)
    wdw, wdb, wdx = ref.backward(x, w, wl, wlse, t, 1.5 if gs else 1.0)
    xd, wd = (offset_copy(x, 1), offset_copy(w, 1)) if off else (x.to(DEV), w.to(DEV))
    bd, td = None if bias is None else bias.to(DEV), t.to(DEV)
    logits, lse, rank, loss = ops.classifier_fwd(xd, wd, bd, td)
    pre = {}
    gp = torch.Generator().manual_seed(5)
    for name, wantg in (('dw', wdw), ('db', wdb), ('dx', wdx)):
        fill = torch.randn(wantg.shape, generator=gp) * max(float(wantg.abs().max()), 1e-3) if acc else torch.full(wantg.shape, 7.0)
        pre[name] = fill.float()
    dw, db = pre['dw'].to(DEV), pre['db'].to(DEV) if has_bias else None
    dx = pre['dx'].to(DEV) if want_dx else None
    ops.classifier_bwd(xd, wd, logits, lse, td, dw, db, acc, dx, acc, gscale_dev=scale_dev, gscale_host=scale_host)
    torch.cuda.synchronize()
    tag = 'classifier float (b=%d, F=%d, C=%d)' % (b, Fd, Cc)
    e = rel_err(logits, wl)
    print('MEASURED %s logits rel max-norm %.3e (bar 1e-5)' % (tag, e))
    assert e < 1e-5
    own = logits.double().cpu()
    bar = 1e-5 * max(float(own.abs().max()), math.log(Cc))
    e_lse = float((lse.double().cpu() - ref.row_lse(own)).abs().max())
    e_loss = abs(float(loss) - float(ref.loss(own, t)))
    print('MEASURED %s row_lse abs %.3e, loss abs %.3e (bar %.3e)' % (tag, e_lse, e_loss, bar))
    assert e_lse <= bar and e_loss <= bar
    assert torch.equal(rank.cpu(), ref.rank_ge(own, t)) and rank.dtype == torch.int32
    outs = [('dw', dw, wdw)] + ([('db', db, wdb)] if has_bias else []) + ([('dx', dx, wdx)] if want_dx else [])
    for name, got, want in outs:
        want = want + pre[name].double() if acc else want
        assert bool(torch.isfinite(got).all())
        if Cc == 1:
            assert float((got.double().cpu() - want).abs().max()) == 0.0, name
            continue
        e = rel_err(got, want)
        print('MEASURED %s %s rel max-norm %.3e (bar 1e-4)' % (tag, name, e))
        assert e < 1e-4, name
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(loss).all())
    if Cc == 1:
        assert float(loss) == 0.0 and int(rank.sum()) == 0
        assert float(dw.abs().max()) == 0.0 and float(db.abs().max()) == 0.0 and float(dx.abs().max()) == 0.0


@pytest.mark.parametrize('b,Fd,Cc,acc', [(513, 40, 33, False), (1100, 36, 40, True)])
def test_long_batch_folds_dw_slabs(pkg, b, Fd, Cc, acc):
    """b > 512: the dw launch cuts the batch into ceil(b / 512) runs and a third launch adds their slabs in run order (the
    scratch grows by the slabs).  Same bars, and the same bits from call to call."""
    H, ops = pkg._hip, pkg.engine.ops
    runs = -(-b // 512)
    assert H.lib.gca_classifier_ws_bytes(b, Fd, Cc) == -(-b * 4 // 16) * 16 + runs * (Cc * Fd + Cc) * 4
    assert H.lib.gca_classifier_ws_bytes(512, Fd, Cc) == 512 * 4
    g = torch.Generator().manual_seed(b)
    x, w, bias = torch.randn(b, Fd, generator=g).abs(), torch.randn(Cc, Fd, generator=g) * 0.2, torch.randn(Cc, generator=g) * 0.1
    t = torch.randint(0, Cc, (b,), generator=g)
    wl, wlse, _, _ = ref.forward(x, w, bias, t)
    wdw, wdb, wdx = ref.backward(x, w, wl, wlse, t)
    xd, wd, bd, td = x.to(DEV), w.to(DEV), bias.to(DEV), t.to(DEV)
    logits, lse, rank, loss = ops.classifier_fwd(xd, wd, bd, td)
    assert rel_err(logits, wl) < 1e-5
    pre = [torch.randn(v.shape, generator=g).float() * float(v.abs().max()) if acc else torch.full(v.shape, 7.0) for v in (wdw, wdb, wdx)]
    runs_out = []
    for _ in range(2):
        dw, db, dx = (p.to(DEV) for p in pre)
        ops.classifier_bwd(xd, wd, logits, lse, td, dw, db, acc, dx, acc)
        runs_out.append((dw, db, dx))
    torch.cuda.synchronize()
    for name, got, again, want, p0 in zip(('dw', 'db', 'dx'), runs_out[0], runs_out[1], (wdw, wdb, wdx), pre):
        e = rel_err(got, want + p0.double() if acc else want)
        print('MEASURED classifier long batch (b=%d, F=%d, C=%d) %s rel max-norm %.3e (bar 1e-4)' % (b, Fd, Cc, name, e))
        assert e < 1e-4 and torch.equal(bits(got), bits(again)), name


def test_eval_path_and_criterion(pkg):
    """target == NULL writes logits only (row_lse optional); the criterion of creat_criterion is the row pass on given logits."""
    ops = pkg.engine.ops
    g = torch.Generator().manual_seed(2)
    x, w, bias = torch.randn(37, 100, generator=g).abs(), torch.randn(11, 100, generator=g) * 0.1, torch.randn(11, generator=g)
    t = torch.randint(0, 11, (37,), generator=g)
    full = ops.classifier_fwd(x.to(DEV), w.to(DEV), bias.to(DEV), t.to(DEV))
    only = ops.classifier_fwd(x.to(DEV), w.to(DEV), bias.to(DEV))
    both = ops.classifier_fwd(x.to(DEV), w.to(DEV), bias.to(DEV), want_lse=True)
    assert torch.equal(bits(only), bits(full[0])) and torch.equal(bits(both[0]), bits(full[0])) and torch.equal(bits(both[1]), bits(full[1]))
    crit = pkg.creat_criterion(pkg.get_defaults())
    assert torch.equal(bits(crit(full[0], t.to(DEV))), bits(full[3]))
    lse, rank, loss = ops.cross_entropy_fwd(full[0], t.to(DEV))
    assert torch.equal(bits(lse), bits(full[1])) and torch.equal(rank, full[2])


# ----------------------------------------------------------------------------- invalid arguments
def test_invalid_arguments_launch_nothing(pkg):
    H, ops = pkg._hip, pkg.engine.ops
    b, Fd, Cc = 4, 8, 5
    x, w, bias = torch.ones(b, Fd, device=DEV), torch.ones(Cc, Fd, device=DEV), torch.zeros(Cc, device=DEV)
    t = torch.zeros(b, dtype=torch.int64, device=DEV)
    nbytes = H.lib.gca_classifier_ws_bytes(b, Fd, Cc)
    assert nbytes >= 4 * b and H.lib.gca_classifier_ws_bytes(b, 0, Cc) == EINVAL and H.lib.gca_classifier_ws_bytes(-1, Fd, Cc) == EINVAL
    assert H.lib.gca_classifier_ws_bytes(b, Fd, 2 ** 31) == EINVAL
    ws = ops.WS.get(nbytes, DEV)
    logits, lse = torch.full((b, Cc), 77.0, device=DEV), torch.full((b,), 77.0, device=DEV)
    rank, loss = torch.full((b,), 77, dtype=torch.int32, device=DEV), torch.full((1,), 77.0, device=DEV)
    dw, db, dx = torch.full((Cc, Fd), 77.0, device=DEV), torch.full((Cc,), 77.0, device=DEV), torch.full((b, Fd), 77.0, device=DEV)

    def fwd(b_=b, F_=Fd, C_=Cc, tgt=t, lse_=lse, loss_=loss, wsb=nbytes):
        return H.lib.gca_classifier_fwd(H.ptr(x), H.ptr(w), H.ptr(bias), H.ptr(tgt), b_, F_, C_, H.ptr(logits), H.ptr(lse_),
                                        H.ptr(rank) if tgt is not None else None, H.ptr(loss_), H.ptr(ws), wsb, H.stream())

    def bwd(b_=b, F_=Fd, C_=Cc, wsb=nbytes):
        return H.lib.gca_classifier_bwd(H.ptr(x), H.ptr(w), H.ptr(logits), H.ptr(lse), H.ptr(t), None, 1.0, b_, F_, C_, H.ptr(dw),
                                        H.ptr(db), 0, H.ptr(dx), 0, H.ptr(ws), wsb, H.stream())
    torch.cuda.synchronize()
    assert fwd(F_=0) == EINVAL and fwd(C_=0) == EINVAL and fwd(F_=-3) == EINVAL and fwd(b_=-1) == EINVAL
    assert fwd(wsb=nbytes - 1) == EINVAL
    assert fwd(tgt=None) == EINVAL                          # loss without target
    assert fwd(lse_=None, loss_=None) == EINVAL             # target without row_lse
    assert bwd(F_=0) == EINVAL and bwd(C_=0) == EINVAL and bwd(b_=-1) == EINVAL and bwd(wsb=nbytes - 1) == EINVAL
    assert fwd(b_=0) == 0 and bwd(b_=0) == 0               # nothing to do, nothing launched
    torch.cuda.synchronize()
    for buf in (logits, lse, loss, dw, db, dx):
        assert bool((buf == 77.0).all())
    assert bool((rank == 77).all())
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert bool((logits == float(Fd)).all()) and bool((rank == Cc - 1).all()) and abs(float(loss) - math.log(Cc)) < 1e-5
    with pytest.raises(ValueError):
        ops.classifier_fwd(x, torch.ones(Cc, Fd + 1, device=DEV))
    with pytest.raises(ValueError):
        ops.classifier_fwd(x, w, bias, t.to(torch.int32))


# ----------------------------------------------------------------------------- model
@pytest.fixture(scope='module')
def tiny(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    cm.register()
    return parity


def product_model(pkg, dropout, seed=3, partial_bn=False):
    torch.manual_seed(seed)
    return pkg.lib.modeling.VideoModelWrapper(cm.NUM_CLASS, cm.T, 'RGB', backbone_name=cm.BACKBONE, backbone_type='3D',
                                              dropout=dropout, partial_bn=partial_bn)


def oracle_of(model, dropout, partial_bn=False):
    o = cm.OracleVideoModel(dropout=dropout, partial_bn=partial_bn)
    o.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    return o.double()


def run_fwd(pkg, model, x):
    Tape, Var = pkg.engine.tape.Tape, pkg.engine.tape.Var
    with torch.no_grad():
        return model.fwd(Tape(False), Var(x.to(DEV))).t


CLIPS = torch.randn(4, 3, 8, 48, 48, generator=torch.Generator().manual_seed(17))


@pytest.mark.parametrize('dropout,mode', [(0.0, 'train'), (0.0, 'eval'), (0.5, 'eval')])
def test_model_logits_vs_oracle(pkg, tiny, dropout, mode):
    m = product_model(pkg, dropout)
    o = oracle_of(m, dropout)
    m.to(DEV)
    m.train(mode == 'train'), o.train(mode == 'train')
    with torch.no_grad():
        want = o(CLIPS.double())
    got = run_fwd(pkg, m, CLIPS)
    e = rel_err(got, want)
    print('MEASURED model logits dropout=%s %s: %.3e (bar 1e-3)' % (dropout, mode, e))
    assert got.shape == (4, cm.NUM_CLASS) and e < 1e-3


def test_model_dropout_is_seeded(pkg, tiny):
    m = product_model(pkg, 0.5).to(DEV).train()
    outs = []
    for seed in (1, 1, 2):
        torch.manual_seed(seed)
        outs.append(run_fwd(pkg, m, CLIPS))
    assert torch.equal(bits(outs[0]), bits(outs[1])) and not torch.equal(bits(outs[0]), bits(outs[2]))


# ----------------------------------------------------------------------------- trainer
def action_cfg(pkg, tiny, dropout=0.0, probe=False, no_partial_bn=True, **solver):
    cfg = tiny.make_cfg(pkg, cm.BACKBONE, 'moco', 32, 20, cm.T, **solver)
    cfg.merge_from_list(['DATASET.NUM_CLASS', cm.NUM_CLASS, 'MODEL.DROPOUT', dropout, 'MODEL.LINEAR_PROBE', probe,
                         'SOLVER.NO_PARTIALBN', no_partial_bn])
    return cfg


STEP_CLIPS = torch.randn(8, 3, 8, 48, 48, generator=torch.Generator().manual_seed(23))
STEP_LABELS = torch.tensor([0, 3, 6, 1, 2, 5, 4, 3])


def oracle_sgd(o, trainer, names):
    """torch.optim.SGD over the oracle parameters `names`, one group each, with the trainer's own lr / weight decay."""
    groups = {g['name']: g for g in trainer.optimizer.param_groups}
    params = dict(o.named_parameters())
    return torch.optim.SGD([{'params': [params[n]], 'lr': groups[n]['lr'], 'weight_decay': groups[n]['weight_decay']} for n in names],
                           momentum=trainer.cfg.SOLVER.MOMENTUM, nesterov=trainer.cfg.SOLVER.NESTEROV)


def buffers_err(model, o, only=None):
    sd, worst = model.state_dict(), 0.0
    for k, v in o.state_dict().items():
        if ('running_' in k) and (only is None or k in only):
            worst = max(worst, rel_err(sd[k], v))
    return worst


def test_finetune_step_vs_oracle(pkg, tiny):
    tr = pkg.ActionTrainer(action_cfg(pkg, tiny), DEV, seed=41)
    o = oracle_of(tr.model, 0.0).train()
    names = [n for n, _ in o.named_parameters()]
    assert [g['name'] for g in tr.optimizer.param_groups] == names
    opt = oracle_sgd(o, tr, names)
    out = tr.train_step(STEP_CLIPS.to(DEV), STEP_LABELS)
    want = o(STEP_CLIPS.double())
    wloss = F.cross_entropy(want, STEP_LABELS)
    wloss.backward()
    torch.cuda.synchronize()
    gaps = (want.detach() - want.detach().gather(1, STEP_LABELS[:, None])).abs()
    gaps[torch.arange(8), STEP_LABELS] = float('inf')
    assert float(gaps.min()) > 1e-3 * float(want.detach().abs().max()), 'the oracle logits are not tie-free'
    e_loss, e_logits = rel_err(out['loss'].reshape(()), wloss), rel_err(out['logits'], want)
    print('MEASURED fine-tune step: loss %.3e, logits %.3e (bar 1e-3)' % (e_loss, e_logits))
    assert e_loss < 1e-3 and e_logits < 1e-3
    g64 = {n: p.grad for n, p in o.named_parameters()}
    errs = {n: rel_err(p.grad, g64[n]) for n, p in tr.model.named_parameters() if float(g64[n].abs().max()) > 0}
    med, p95, worst = tiny.check_grad_errors(errs)
    print('MEASURED fine-tune step: gradient rel err median %.3e, p95 %.3e, worst %.3e (bars 2e-4 / - / 1e-1)' % (med, p95, worst))
    opt.step()
    e_buf = buffers_err(tr.model, o)
    print('MEASURED fine-tune step: BatchNorm buffers %.3e (bar 1e-3)' % e_buf)
    assert e_buf < 1e-3
    sd = tr.model.state_dict()
    post = {n: rel_err(sd[n], p) for n, p in o.named_parameters()}
    tiny.check_grad_errors(post, 'updated parameters')
    rank = ref.rank_ge(want.detach(), STEP_LABELS)
    assert torch.equal(out['rank_ge'].cpu(), rank)
    assert float(out['prec1']) == 100.0 * float((rank < 1).sum()) / 8 and float(out['prec5']) == 100.0 * float((rank < 5).sum()) / 8


@pytest.mark.parametrize('dropout,no_partial_bn', [(0.0, True), (0.5, True), (0.0, False)])
def test_linear_probe_step(pkg, tiny, dropout, no_partial_bn):
    tr = pkg.ActionTrainer(action_cfg(pkg, tiny, dropout=dropout, probe=True, no_partial_bn=no_partial_bn), DEV, seed=43)
    prefix = 'base_model.fc.' if dropout == 0 else 'new_fc.'
    assert tr.model.classifier_prefix == prefix
    assert [g['name'] for g in tr.optimizer.param_groups] == [prefix + 'weight', prefix + 'bias']
    assert list(tr.state_dict()['optimizer']['state'].keys()) == [0, 1]
    o = oracle_of(tr.model, dropout, partial_bn=not no_partial_bn).train()
    before = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    opt = oracle_sgd(o, tr, [prefix + 'weight', prefix + 'bias'])
    mask = None
    if dropout > 0:        # the product draws its keep mask from torch's device generator: draw the same one for the oracle
        torch.manual_seed(9)
        mask = torch.empty(8, tr.model.feature_dim, device=DEV).bernoulli_(1.0 - dropout).mul_(1.0 / (1.0 - dropout)).double().cpu()
        torch.manual_seed(9)
    out = tr.train_step(STEP_CLIPS.to(DEV), STEP_LABELS)
    want = o(STEP_CLIPS.double(), mask=mask)
    F.cross_entropy(want, STEP_LABELS).backward()
    opt.step()
    torch.cuda.synchronize()
    assert rel_err(out['logits'], want) < 1e-3
    after = tr.model.state_dict()
    pnames = set(n for n, _ in tr.model.named_parameters())
    moved = []
    for k, v in after.items():
        if k in pnames and not k.startswith(prefix):
            assert torch.equal(bits(v), bits(before[k])), k                  # every encoder parameter bitwise unchanged
        elif 'running_' in k and not torch.equal(bits(v), bits(before[k])):
            moved.append(k)
    stats = [k for k in after if 'running_' in k]
    if no_partial_bn:
        assert moved == stats
    else:
        assert moved == stats[:2] and moved[0].endswith('running_mean') and moved[1].endswith('running_var')
    e_buf = buffers_err(tr.model, o)
    print('MEASURED linear probe (%s): BatchNorm buffers %.3e (bar 1e-3)' % (prefix, e_buf))
    assert e_buf < 1e-3
    od = dict(o.named_parameters())
    post = {k: rel_err(after[k], od[k]) for k in (prefix + 'weight', prefix + 'bias')}
    print('MEASURED linear probe (%s): updated head rel err %s (bar 2e-4)' % (prefix, post))
    assert max(post.values()) < 2e-4
    assert not torch.equal(bits(after[prefix + 'weight']), bits(before[prefix + 'weight']))


@pytest.fixture(scope='module')
def pretrain_checkpoint(pkg, tiny):
    """A checkpoint dict as the MoCo trainer writes it, after one step (as in tests/test_gpu_retrieval.py)."""
    cfg = tiny.make_cfg(pkg, cm.BACKBONE, 'moco', 32, 20, cm.T)
    trainer = pkg.MoCoTrainer(cfg, DEV, use_graph=False, seed=5)
    trainer.train_step(torch.randn(8, 6, 8, 48, 48, generator=torch.Generator().manual_seed(3)).to(DEV))
    sd = trainer.state_dict(epoch=1)
    return {'epoch': 1, 'state_dict': {n: t.detach().cpu().clone() for n, t in sd['state_dict'].items()}}


def test_load_pretrained_by_name(pkg, tiny, pretrain_checkpoint):
    tr = pkg.ActionTrainer(action_cfg(pkg, tiny), DEV, seed=47)
    head = {k: v.detach().clone() for k, v in tr.model.classifier.state_dict().items()}
    tr.load_pretrained(pretrain_checkpoint)
    src = pretrain_checkpoint['state_dict']
    n = 0
    for k, v in tr.model.state_dict().items():
        if k.startswith('base_model.fc.'):
            assert torch.equal(v, head[k[len('base_model.fc.'):]])
        else:
            assert torch.equal(v.cpu(), src['model.encoder.' + k]), k
            n += 1
    assert n == 126
    with pytest.raises(KeyError):
        tr.load_pretrained({'state_dict': {k: v for k, v in src.items() if 'layer4' not in k}})


def test_checkpoint_round_trip_is_bit_exact(pkg, tiny, golden):
    cfg = action_cfg(pkg, tiny)
    a = pkg.ActionTrainer(cfg, DEV, seed=51)
    a.train_step(STEP_CLIPS.to(DEV), STEP_LABELS)
    a.best_pred = 12.5
    sd = copy.deepcopy(a.state_dict(epoch=3))
    assert list(sd) == ['epoch', 'state_dict', 'optimizer', 'best_pred']
    assert list(sd['state_dict'].keys()) == [str(k) for k in golden('classify').z['keys:d0']]
    b = pkg.ActionTrainer(cfg, DEV, seed=52)
    assert b.load_state_dict(sd) == 3 and b.best_pred == 12.5
    clips2 = torch.randn(8, 3, 8, 48, 48, generator=torch.Generator().manual_seed(29)).to(DEV)
    oa, ob = a.train_step(clips2, STEP_LABELS), b.train_step(clips2, STEP_LABELS)
    torch.cuda.synchronize()
    for k in ('loss', 'logits', 'rank_ge', 'prec1', 'prec5'):
        assert torch.equal(bits(oa[k].float()), bits(ob[k].float())), k
    sa, sb = a.model.state_dict(), b.model.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(bits(a.optimizer.buf), bits(b.optimizer.buf))


def test_validate_matches_oracle(pkg, tiny):
    tr = pkg.ActionTrainer(action_cfg(pkg, tiny), DEV, seed=41)
    o = oracle_of(tr.model, 0.0).eval()
    batches = [(STEP_CLIPS[:5], STEP_LABELS[:5]), (STEP_CLIPS[5:], STEP_LABELS[5:])]
    res = tr.validate(batches)
    with torch.no_grad():
        want = o(STEP_CLIPS.double())
    rank = ref.rank_ge(want, STEP_LABELS)
    assert res['count'] == 8 and abs(res['loss'] - float(F.cross_entropy(want, STEP_LABELS))) < 1e-3 * float(F.cross_entropy(want, STEP_LABELS))
    assert res['top1'] == 100.0 * float((rank < 1).sum()) / 8 and res['top5'] == 100.0 * float((rank < 5).sum()) / 8
    assert tr.model.training


# ----------------------------------------------------------------------------- video-level test
def test_eval_video_and_evaluate(pkg, tiny):
    C = pkg.lib.evaluation.classify
    m = product_model(pkg, 0.0, seed=61)
    o = oracle_of(m, 0.0).eval()
    m.to(DEV).eval()
    B, crops, clips, T = 2, 3, 2, cm.T
    data = torch.randn(B, 3, clips * crops * T, 48, 48, generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        views = [o(data[:, :, v * T:(v + 1) * T].double()) for v in range(clips * crops)]
        want = torch.stack(views, 1).mean(1)
    got = C.eval_video(m, data.to(DEV), crops, T)
    assert got.shape == want.shape == (B, cm.NUM_CLASS) and rel_err(got, want) < 1e-3
    assert rel_err(C.eval_video(m, data.to(DEV), crops, T, softmax=True), torch.softmax(want, dim=-1)) < 1e-3
    assert float((views[0] - views[1]).abs().max()) > 1e-3 * float(want.abs().max())       # the views do differ
    labels = [torch.tensor([2, 5]), torch.tensor([2, 0])]
    res = C.evaluate(m, [(data, labels[0]), (data.flip(0), labels[1])], crops, T, device=DEV)
    scores, lab = res['scores'], np.array([2, 5, 2, 0])
    assert scores.shape == (4, cm.NUM_CLASS) and np.array_equal(res['labels'], lab)
    cf = ref.confusion(lab, scores.argmax(1), cm.NUM_CLASS)
    assert np.array_equal(res['confusion'], cf) and res['mean_class_acc'] == ref.mean_class_acc(cf)
    rank = ref.rank_ge(torch.from_numpy(scores), torch.from_numpy(lab))
    assert res['top1'] == 100.0 * float((rank < 1).sum()) / 4 and res['top5'] == 100.0 * float((rank < 5).sum()) / 4
    m.train()
    with pytest.raises(RuntimeError):
        C.eval_video(m, data.to(DEV), crops, T)


# ----------------------------------------------------------------------------- refusals
def test_trainer_refusals(pkg, tiny):
    ops, par = pkg.engine.ops, pkg.parallel
    with pytest.raises(NotImplementedError):
        pkg.ActionTrainer(action_cfg(pkg, tiny, no_partial_bn=False), DEV)          # fine-tune under partial BN
    with pytest.raises(NotImplementedError):
        pkg.ActionTrainer(action_cfg(pkg, tiny, USE_TRICK=True), DEV)
    cfg = action_cfg(pkg, tiny)
    cfg.APEX.FLAG = True
    with pytest.raises(NotImplementedError):
        pkg.ActionTrainer(cfg, DEV)
    with pytest.raises(NotImplementedError):
        pkg.ActionTrainer(action_cfg(pkg, tiny), DEV, ctx=par.DistCtx(force_active=True))
    with pytest.raises(NotImplementedError):
        pkg.ActionTrainer(action_cfg(pkg, tiny), DEV, use_graph=True)
    default = ops.get_conv_math()
    ops.set_conv_math('fp16')
    try:
        with pytest.raises(NotImplementedError):
            pkg.ActionTrainer(action_cfg(pkg, tiny), DEV)
    finally:
        ops.set_conv_math(default)
    with pytest.raises(ValueError):
        pkg.ActionTrainer(_s3d_cfg(pkg, tiny), DEV)                             # S3D needs MODEL.DROPOUT > 0
    tr = pkg.ActionTrainer(action_cfg(pkg, tiny), DEV, seed=1)
    before = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    for bad in (torch.tensor([0, 1, 2, 7]), torch.tensor([0, -1, 2, 3])):
        with pytest.raises(ValueError):
            tr.train_step(CLIPS.to(DEV), bad)
    with pytest.raises(ValueError):
        tr.train_step(CLIPS.to(DEV), torch.tensor([0, 1, 2]))
    with pytest.raises(RuntimeError):
        tr.train_step(CLIPS, torch.tensor([0, 1, 2, 3]))                          # clips not on the device
    for k, v in tr.model.state_dict().items():
        assert torch.equal(v, before[k]), k


def _s3d_cfg(pkg, tiny):
    cfg = action_cfg(pkg, tiny)
    cfg.MODEL.BACKBONE = 'S3D'
    return cfg
