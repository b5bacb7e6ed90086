"""CPU tests of the action-recognition ground: the fp64 specification (tests/classify_ref.py) against torch autograd,
ref64.rank_ge and sklearn; the product's VideoModelWrapper (keys, key order, train() flags, refusals) and the tests' oracle
model (tests/classify_model.py) against the fixture generated from the reference (tests/golden/classify.npz)."""
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


def _problem(b, Fd, Cc, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, Fd, generator=g, dtype=torch.float64).abs()
    w = torch.randn(Cc, Fd, generator=g, dtype=torch.float64) * 0.1
    bv = torch.randn(Cc, generator=g, dtype=torch.float64) if bias else None
    t = torch.randint(0, Cc, (b,), generator=g)
    return x, w, bv, t


# ----------------------------------------------------------------------------- the specification
@pytest.mark.parametrize('b,Fd,Cc,bias', [(5, 12, 7, True), (33, 40, 130, False), (2, 9, 1, True)])
def test_specification_vs_autograd(b, Fd, Cc, bias):
    x, w, bv, t = _problem(b, Fd, Cc, 3, bias)
    xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    ba = None if bv is None else bv.clone().requires_grad_(True)
    lg = F.linear(xa, wa, ba)
    loss = F.cross_entropy(lg, t)
    (2.5 * loss).backward()
    slg, slse, sloss, srank = ref.forward(x, w, bv, t)
    assert torch.allclose(slg, lg.detach(), rtol=1e-13, atol=1e-13)
    assert torch.allclose(slse, torch.logsumexp(lg.detach(), 1), rtol=1e-13, atol=1e-13)
    assert abs(float(sloss) - float(loss.detach())) <= 1e-13 * max(1.0, abs(float(loss.detach())))
    assert torch.equal(srank.long(), ref64.rank_ge(slg, t).long())
    dw, db, dx = ref.backward(x, w, slg, slse, t, 2.5)
    assert torch.allclose(dw, wa.grad, rtol=1e-11, atol=1e-14) and torch.allclose(dx, xa.grad, rtol=1e-11, atol=1e-14)
    if ba is not None:
        assert torch.allclose(db, ba.grad, rtol=1e-11, atol=1e-14)
    if Cc == 1:
        assert float(sloss) == 0.0 and float(dw.abs().max()) == 0.0 and float(dx.abs().max()) == 0.0 and int(srank.sum()) == 0


def test_rank_counts_ties_against_the_target():
    lg = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0]])
    assert ref.rank_ge(lg, torch.tensor([1, 3])).tolist() == [1, 3]
    assert ref.rank_ge(lg, torch.tensor([3, 0])).tolist() == ref64.rank_ge(lg, torch.tensor([3, 0])).tolist() == [3, 3]


def test_confusion_and_mean_class_acc_vs_sklearn(pkg):
    rng = np.random.RandomState(4)
    labels = rng.randint(0, 9, size=200)
    labels[labels == 5] = 4                       # class 5 never occurs as a label
    pred = np.where(rng.rand(200) < 0.6, labels, rng.randint(0, 9, size=200))
    cf = ref.confusion(labels, pred, 9)
    C = pkg.lib.evaluation.classify
    assert np.array_equal(C.confusion(labels, pred, 9), cf)
    assert cf[5].sum() == 0 and cf.sum() == 200
    accs = [cf[c, c] / cf[c].sum() for c in range(9) if c != 5]
    assert abs(ref.mean_class_acc(cf) - np.mean(accs)) < 1e-15
    assert abs(C.mean_class_acc(cf) - ref.mean_class_acc(cf)) < 1e-15
    with pytest.raises(ValueError):
        C.confusion([0, 9], [0, 0], 9)
    sk = pytest.importorskip('sklearn.metrics')
    assert np.array_equal(sk.confusion_matrix(labels, pred, labels=list(range(9))), cf)
    with np.errstate(invalid='ignore', divide='ignore'):
        ref_acc = np.diag(cf.astype(float)) / cf.astype(float).sum(axis=1)      # tools/test_ds.py:190-194: NaN for class 5
    assert np.isnan(ref_acc[5]) and abs(np.nanmean(ref_acc) - ref.mean_class_acc(cf)) < 1e-15


# ----------------------------------------------------------------------------- the wrapper against the reference fixture
@pytest.fixture(scope='module')
def tiny(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    cm.register()
    return pkg.lib.modeling.VideoModelWrapper


@pytest.mark.parametrize('dropout,group', [(0.0, 'keys:d0'), (0.5, 'keys:d05')])
def test_state_dict_keys_and_order(tiny, golden, dropout, group):
    want = [str(k) for k in golden('classify').z[group]]
    m = tiny(cm.NUM_CLASS, cm.T, 'RGB', backbone_name=cm.BACKBONE, backbone_type='3D', dropout=dropout)
    assert list(m.state_dict().keys()) == want
    assert list(cm.OracleVideoModel(dropout=dropout).state_dict().keys()) == want
    head = 'base_model.fc.' if dropout == 0 else 'new_fc.'
    assert want[-2:] == [head + 'weight', head + 'bias'] and m.classifier_prefix == head
    assert (m.new_fc is None) == (dropout == 0)
    assert tuple(m.classifier.weight.shape) == (cm.NUM_CLASS, m.feature_dim) and float(m.classifier.bias.abs().max()) == 0.0
    assert 0.0005 < float(m.classifier.weight.std()) < 0.002               # normal_(0, 0.001)


def test_train_flags_under_partial_bn(tiny, pkg, golden):
    want = [bool(v) for v in golden('classify').z['bn_training:pbn']]
    BN = pkg.engine.layers.HipBatchNorm3d
    m = tiny(cm.NUM_CLASS, cm.T, 'RGB', backbone_name=cm.BACKBONE, backbone_type='3D', dropout=0, partial_bn=True)
    m.train()
    bns = [b for b in m.base_model.modules() if isinstance(b, BN)]
    assert [b.training for b in bns] == want and sum(want) == 1 and len(want) == 21
    assert [b.weight.requires_grad for b in bns] == want and [b.bias.requires_grad for b in bns] == want
    assert m.classifier.training and m.classifier.weight.requires_grad
    o = cm.OracleVideoModel(partial_bn=True).train()
    assert [b.training for b in o.base_model.modules() if isinstance(b, torch.nn.BatchNorm3d)] == want
    free = tiny(cm.NUM_CLASS, cm.T, 'RGB', backbone_name=cm.BACKBONE, backbone_type='3D', dropout=0, partial_bn=False).train()
    assert all(b.training for b in free.modules() if isinstance(b, BN)) and all(p.requires_grad for p in free.parameters())


def test_refusals_at_construction(tiny, pkg):
    with pytest.raises(ValueError):
        tiny(cm.NUM_CLASS, 16, 'RGB', backbone_name='S3D', backbone_type='3D', dropout=0)
    with pytest.raises(ValueError):
        tiny(cm.NUM_CLASS, cm.T, 'RGB', backbone_name=cm.BACKBONE, backbone_type='2D', dropout=0)
    with pytest.raises(ValueError):
        tiny(cm.NUM_CLASS, cm.T, 'Flow', backbone_name=cm.BACKBONE, backbone_type='3D', dropout=0)
    cfg = pkg.get_defaults()
    assert cfg.MODEL.LINEAR_PROBE is False and cfg.MODEL.METRIC_LOSS_TYPE == 'CrossEntropyLoss' and cfg.TEST.BATCH_SIZE == 128
    cfg.MODEL.METRIC_LOSS_TYPE = 'TripletLoss'
    with pytest.raises(NotImplementedError):
        pkg.creat_criterion(cfg)


def _golden_run(golden, dtype):
    g = golden('classify')
    m = cm.golden_model(g, dtype)
    x, t = g.x('xspec').to(dtype), g.t('target')
    m.train()
    y = m(x)
    loss = F.cross_entropy(y, t)
    loss.backward()
    m.eval()
    with torch.no_grad():
        ye = m(x)
    return g, m, y.detach(), loss.detach(), ye


def test_oracle_model_reproduces_the_reference_fp32(golden):
    """Same ATen calls in the same order as the reference: agreement to rounding noise."""
    g, m, y, loss, ye = _golden_run(golden, torch.float32)
    for got, key in ((y, 'logits_train'), (loss, 'loss'), (ye, 'logits_eval'), (m.base_model.fc.weight.grad, 'dw_fc'),
                     (m.base_model.fc.bias.grad, 'db_fc'), (m.base_model.conv1_s.weight.grad, 'dw_conv1_s')):
        assert rel_err(got, g.t(key)) < 1e-5, key


def test_oracle_model_fp64_vs_reference(golden):
    """The fp64 oracle used on the GPU against the reference's fp32 numbers: the project's model bar of 1e-3 for forward
    quantities and the head's gradients (linear in the features); the first conv's gradient passes through every ReLU
    mask of the net, so it gets the worst-case bar of tests/parity.check_grad_errors."""
    g, m, y, loss, ye = _golden_run(golden, torch.float64)
    for got, key in ((y, 'logits_train'), (loss, 'loss'), (ye, 'logits_eval'), (m.base_model.fc.weight.grad, 'dw_fc'),
                     (m.base_model.fc.bias.grad, 'db_fc')):
        e = rel_err(got, g.t(key))
        print('MEASURED fp64 oracle vs reference %s: %.3e (bar 1e-3)' % (key, e))
        assert e < 1e-3, key
    e = rel_err(m.base_model.conv1_s.weight.grad, g.t('dw_conv1_s'))
    print('MEASURED fp64 oracle vs reference dw_conv1_s: %.3e (bar 1e-1)' % e)
    assert e < 1e-1
    rank = ref.rank_ge(y, g.t('target'))
    assert float((rank < 1).sum()) * 25.0 == float(g.t('prec1')) and float((rank < 5).sum()) * 25.0 == float(g.t('prec5'))
