"""CPU checks of tests/ref64.py: (1) every fp64 reference agrees with the authority the suite already trusts (ATen modules,
torch.optim.SGD, the oracle package) to 1e-12 at benign inputs, both sides in double; (2) every precondition the GPU edge
tests (tests/test_gpu_edges.py) rely on holds for the seeded inputs they use."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import ref64
from ref64 import F64, rel

TOL = 1e-12


# ----------------------------------------------------------------------------- references vs the trusted authorities
@pytest.mark.parametrize('shape,relu,res', [((4, 6, 2, 3, 4), True, True), ((3, 5, 1, 2, 5), False, False), ((8, 6), False, False),
                                            ((2, 5), True, False)])
def test_bn_train_reference_vs_aten(shape, relu, res):
    torch.manual_seed(1)
    x = torch.randn(shape, dtype=F64) * 1.5 + 0.3
    Cc = shape[1]
    bn = (nn.BatchNorm3d if len(shape) == 5 else nn.BatchNorm1d)(Cc).double()
    bn.weight.data.uniform_(0.5, 1.5)
    bn.bias.data.normal_()
    bn.running_mean.normal_()
    bn.running_var.uniform_(0.5, 2.0)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    r = torch.randn(shape, dtype=F64) if res else None
    xr = x.clone().requires_grad_(True)
    rr = r.clone().requires_grad_(True) if res else None
    z = bn(xr)
    if res:
        z = z + rr
    if relu:
        z = F.relu(z)
    dz = torch.randn(shape, dtype=F64)
    z.backward(dz)
    N = shape[0]
    got = ref64.bn_train(x.reshape(N, Cc, -1), bn.weight.data, bn.bias.data, bn.eps, 0.1, rm0, rv0,
                         None if r is None else r.reshape(N, Cc, -1), relu, dz.reshape(N, Cc, -1))
    assert rel(got['z'].reshape(shape), z) < TOL
    assert rel(got['rmean'], bn.running_mean) < TOL and rel(got['rvar'], bn.running_var) < TOL
    assert rel(got['dx'].reshape(shape), xr.grad) < TOL
    assert rel(got['dgamma'], bn.weight.grad) < TOL and rel(got['dbeta'], bn.bias.grad) < TOL
    if res:
        assert rel(got['dres'].reshape(shape), rr.grad) < TOL
    # the saved-statistics form of the backward, fed the exact statistics, is the same function
    sv = ref64.bn_bwd_saved(dz.reshape(N, Cc, -1), x.reshape(N, Cc, -1), bn.weight.data, got['mean'], got['invstd'],
                            (got['z'] > 0) if relu else None)
    for key in ('dx', 'dgamma', 'dbeta'):
        assert rel(sv[key], got[key]) < TOL
    if res:
        assert rel(sv['dres'], got['dres']) < TOL
    # eval-mode fold against the module in eval mode (it now holds the updated running statistics)
    bn.eval()
    scale, shift = ref64.bn_eval_fold(bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, bn.eps)
    v = (1, Cc) + (1,) * (len(shape) - 2)
    assert rel(x * scale.reshape(v) + shift.reshape(v), bn(x)) < TOL


def test_l2norm_and_negcos_references_vs_aten():
    torch.manual_seed(2)
    x = torch.randn(6, 40, dtype=F64)
    x[2] = 0                                            # below the eps clamp: y = 0, dx = dy / eps
    xr = x.clone().requires_grad_(True)
    yr = F.normalize(xr, dim=1, eps=1e-12)
    dy = torch.randn_like(yr)
    yr.backward(dy)
    got = ref64.l2norm(x, 1e-12, dy)
    assert rel(got['y'], yr) < TOL and rel(got['dx'], xr.grad) < TOL
    assert float(got['inv'][2]) == 1e12 and float(got['y'][2].abs().max()) == 0
    p, z = torch.randn(5, 24, dtype=F64), torch.randn(5, 24, dtype=F64)
    pr = p.clone().requires_grad_(True)
    cos = F.cosine_similarity(pr, z, dim=-1)
    (-cos.mean() * 0.5).backward()
    got = ref64.negcos(p, z, 0.5)
    assert rel(got['cos'], cos) < TOL and rel(got['loss'], -cos.mean() * 0.5) < TOL and rel(got['dp'], pr.grad) < TOL


@pytest.mark.parametrize('nesterov', [True, False])
def test_sgd_reference_vs_torch_optim(nesterov):
    torch.manual_seed(3)
    n = 256 * 5
    p0, gr = torch.randn(n, dtype=F64), torch.randn(n, dtype=F64)
    lr = torch.where(torch.arange(n // 256) % 2 == 0, 0.06, 0.12).double().repeat_interleave(256)
    wd = torch.where(torch.arange(n // 256) % 2 == 0, 5e-4, 0.0).double().repeat_interleave(256)
    groups = [{'params': [nn.Parameter(p0[i * 256:(i + 1) * 256].clone())], 'lr': float(lr[i * 256]),
               'weight_decay': float(wd[i * 256])} for i in range(n // 256)]
    opt = torch.optim.SGD(groups, momentum=0.9, nesterov=nesterov)
    p, buf = p0.clone(), torch.zeros(n, dtype=F64)
    for step in range(3):
        gs = gr * (step + 1)
        for i, gp in enumerate(groups):
            gp['params'][0].grad = gs[i * 256:(i + 1) * 256].clone()
        opt.step()
        p, buf = ref64.sgd(p, gs, buf, lr, wd, 0.9, nesterov, first=step == 0)
    assert rel(p, torch.cat([gp['params'][0].data for gp in groups])) < TOL
    # a clip coefficient is a scaled gradient
    a = ref64.sgd(p0, gr, buf, lr, wd, 0.9, nesterov, coef=0.25)
    b = ref64.sgd(p0, 0.25 * gr, buf, lr, wd, 0.9, nesterov)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('b,K,D,index', [(4, 10, 16, 8), (5, 64, 24, 0)])
def test_infonce_reference_vs_oracle_with_snapshot(b, K, D, index):
    from oracle.moco import RGBMoCo, NCESoftmaxLoss
    torch.manual_seed(4)
    mo = RGBMoCo(D, K=K, T=0.07).double()
    mo.index = index
    q = F.normalize(torch.randn(b, D, dtype=F64)).requires_grad_(True)
    k = F.normalize(torch.randn(b, D, dtype=F64))
    mem0 = mo.memory.clone()
    logits, _ = mo(q, k)
    loss = NCESoftmaxLoss()(logits)
    loss.backward()
    ids = (torch.arange(b) + index) % K
    assert not torch.equal(mo.memory, mem0)             # the enqueue has happened: only the snapshot rule recovers mem0
    got = ref64.infonce(q, k, mo.memory, 1 / 0.07, ov_start=index, ov_rows=mem0[ids])
    assert rel(got['logits'], logits) < TOL and rel(got['loss'], loss) < TOL
    assert rel(got['lse'], torch.logsumexp(logits.detach(), 1)) < TOL
    assert rel(got['dq'], q.grad) < TOL
    assert rel(ref64.infonce_bwd(logits, k, mo.memory, 1 / 0.07, index, mem0[ids]), q.grad) < TOL
    lr = logits.detach().clone().requires_grad_(True)
    NCESoftmaxLoss()(lr).backward()
    assert rel(ref64.nce_dlogits(logits), lr.grad) < TOL
    # rank: position of the positive in the descending order (no ties in randn data) = what topk-accuracy tests
    order = logits.detach().argsort(1, descending=True)
    assert torch.equal(got['rank'], (order == 0).float().argmax(1))


def test_rank_ge_reference_vs_topk():
    torch.manual_seed(5)
    out = torch.randn(9, 300, dtype=F64)
    tgt = torch.randint(0, 300, (9,))
    tgt[0], tgt[1] = 0, 299
    rk = ref64.rank_ge(out, tgt)
    for kk in (1, 5, 50):
        hit = (out.topk(kk, 1).indices == tgt[:, None]).any(1)
        assert torch.equal(hit, rk < kk)
    assert torch.equal(rk == 0, out.max(1).indices == tgt)
    tied = torch.tensor([[1.0, 2.0, 2.0, 0.5, 2.0]], dtype=F64)
    assert int(ref64.rank_ge(tied, torch.tensor([1]))) == 2      # ties count against the target


class _Const(nn.Module):
    def __init__(self, t):
        super().__init__()
        self.t = t

    def forward(self, x):
        return self.t


@pytest.mark.parametrize('T,HW,max_hop,temp', [(5, 7, 1, 0.5), (8, 12, 3, 1.0), (3, 8, 5, 1.0), (1, 4, 0, 1.0)])
def test_graph_references_vs_oracle(T, HW, max_hop, temp):
    from oracle.graph import GCNLayer, TemporalGraphAug, hop_distance, relaxed_bernoulli_rsample
    torch.manual_seed(6)
    B, Ci = 2, 6
    gq = (torch.randn(B, Ci, T, HW, 1, dtype=F64) * 0.4).requires_grad_(True)
    gk = (torch.randn(B, Ci, T, HW, 1, dtype=F64) * 0.4).requires_grad_(True)
    u = torch.rand(B, T, T, dtype=F64)
    dadj = torch.randn(B, T, T, dtype=F64)
    aug = TemporalGraphAug(4, alpha=0.5, temperature=temp, max_hop=max_hop)
    aug.g_q, aug.g_k = _Const(gq), _Const(gk)
    sim = aug.sim_adj(gq)
    pre = aug.hop_weighted(sim, hop_distance(T, max_hop))
    adj = relaxed_bernoulli_rsample(pre, u, temp)           # in double the oracle clamps at fp64's eps
    adj.backward(dadj)
    got = ref64.graph_adj(gq, gk, u, max_hop, 0.5, temp, dadj, eps=float(torch.finfo(F64).eps))
    for key, want in (('sim', sim), ('pre', pre), ('adj', adj), ('dgq', gq.grad), ('dgk', gk.grad)):
        assert rel(got[key], want) < TOL, key
    # at the fp32 clamp (the default, what the kernels use) the saved-tensor form of the backward is the same function
    full = ref64.graph_adj(gq, gk, u, max_hop, 0.5, temp, dadj)
    sv = ref64.graph_adj_bwd_saved(dadj, gq, gk, full['sim'], full['pre'], full['adj'], max_hop, 0.5, temp)
    assert rel(sv['dgq'], full['dgq']) < TOL and rel(sv['dgk'], full['dgk']) < TOL
    # and the fp32 oracle agrees with it to fp32 accuracy (the clamp of out-of-band entries included)
    adj32 = relaxed_bernoulli_rsample(aug.hop_weighted(sim.float(), hop_distance(T, max_hop)), u.float(), temp)
    assert rel(adj32, full['adj']) < 1e-5
    # message passing
    gcn = GCNLayer(Ci).double()
    gcn.conv.weight.data.copy_(torch.eye(Ci, dtype=F64).reshape(Ci, Ci, 1, 1, 1))
    s = torch.randn(B, Ci, T, HW, 1, dtype=F64, requires_grad=True)
    ar = adj.detach().clone().requires_grad_(True)
    out = gcn(s, ar)
    dout = torch.randn_like(out)
    out.backward(dout)
    gg = ref64.graph_gcn(ar, s, dout)
    assert rel(gg['out'], out) < TOL and rel(gg['ds'], s.grad) < TOL and rel(gg['dadj'], ar.grad) < TOL


# ----------------------------------------------------------------------------- preconditions of the GPU edge tests
@pytest.mark.parametrize('case', ref64.INFONCE_CASES, ids=[c[0] for c in ref64.INFONCE_CASES])
def test_infonce_exact_inputs_are_exact_and_tied(case):
    """fp32 and fp64 products of the quantised inputs agree BIT FOR BIT (so the kernels' logits must equal the reference
    whatever their summation order), every row has >= 3 exact ties with its positive, and the shape takes the path the
    case is named after under the dispatch rule of gca_moco_logits_fwd."""
    name, b, K, D, counter, aligned, path = case
    q, k, queue = ref64.infonce_exact_inputs(b, K, D)
    for t in (q, k, queue):
        assert float(t.abs().max()) <= 2 and torch.equal(t * 8, (t * 8).round())
    l32 = torch.cat(((q * k).sum(1, keepdim=True), q @ queue.t()), 1) * ref64.INFONCE_INV_T
    ref = ref64.infonce(q, k, queue, ref64.INFONCE_INV_T)
    assert torch.equal(l32.double(), ref['logits'])
    assert torch.equal(ref['logits'].float().double(), ref['logits'])
    # another order: reversed feature axis, and per-half partial sums
    h = D // 2
    l32b = torch.cat(((q * k).flip(1).sum(1, keepdim=True), q[:, h:] @ queue[:, h:].t() + q[:, :h] @ queue[:, :h].t()), 1) * 16.0
    assert torch.equal(l32b, l32)
    ties = (ref['logits'][:, 1:] == ref['logits'][:, :1]).sum(1)
    assert int(ties.min()) >= ref64.INFONCE_TIES
    assert int(ref['rank'].min()) >= ref64.INFONCE_TIES
    assert ref64.infonce_path(b, K, D, counter, aligned) == path


def test_infonce_cases_cover_every_path_and_width():
    paths = {c[6][:2] for c in ref64.INFONCE_CASES}
    assert paths == {('persist', 1), ('persist', 2), ('persist', 4), ('fused', 1), ('fused', 2), ('fused', 4), ('fused', 8),
                     ('plain', 1), ('plain', 4)}
    capped = [c for c in ref64.INFONCE_CASES if c[0] == 'persist-capped'][0]
    ncb = -(-capped[2] // 32)
    assert capped[6][2] == 256 and ncb > 256 * 4 and ncb % (256 * 4) != 0 and capped[2] % 32 != 0      # several tiles per wave, ragged
    assert any(c[6][0] == 'fused' and c[1] <= 32 for c in ref64.INFONCE_CASES)


def test_infonce_wide_spread_inputs_force_the_rescale():
    q, k, queue = ref64.infonce_wide_inputs()
    ref = ref64.infonce(q, k, queue, 1 / 0.07)
    lg = ref['logits']
    assert float((lg.max(1).values - lg.median(1).values).max()) > 48     # > 2 x the 24 threshold: taken in ANY visiting order
    assert float(lg.abs().max()) > 300
    for i in (0, 1):                                                       # dominated rows: loss_i = lse_i - l0_i cancels
        assert float(lg[i, 0] - lg[i, 1:].max()) > 30
        assert float(ref['lse'][i] - lg[i, 0]) < 1e-12
    assert int(ref['rank'][2:].min()) > 0


def test_graph_clamp_case_masks_at_most_half():
    gq, gk = ref64.graph_onehot_inputs()
    u = torch.rand(2, 4, 4, generator=torch.Generator().manual_seed(7))
    ref = ref64.graph_adj(gq, gk, u, 3, 0.5, 1.0)
    pre = ref['pre']
    inside = (pre > 2 * ref64.EPS32) & (pre < 1 - 2 * ref64.EPS32)
    assert float((~inside).double().mean()) <= 0.5
    assert bool((pre[0] <= ref64.EPS32).any()) and bool((pre[0] >= 1 - ref64.EPS32).any())      # both clamps are hit
    assert bool(inside[1].all())


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('k', ref64.BN_RATIOS)
@pytest.mark.parametrize('shape', ref64.BN_SHAPES)
def test_bn_envelope_inputs_realise_the_intended_ratio(shape, k, dtype):
    x, sigma = ref64.bn_envelope_input(*shape, k, dtype=dtype)
    assert float((ref64.bn_ratio(x) - k).abs().max()) <= 0.05 * max(k, 1)
    x3 = ref64.d(x)
    std = ((x3 - x3.mean((0, 2), keepdim=True)) ** 2).mean((0, 2)).sqrt()
    assert float((std / sigma - 1).abs().max()) < 0.05


@pytest.mark.parametrize('n,parts', [(96, 1), (40000, 5), (8192, 1)])
@pytest.mark.parametrize('k', [0, 3, 10, 30, 300])
def test_bn_variance_bound_covers_the_fp32_partial_emulation(n, parts, k):
    """The derived bound (1 + 3 k^2) 2^-24 on var = E[x^2] - mean^2 with fp32-rounded partials holds for a CPU emulation of
    exactly that rounding."""
    g = torch.Generator().manual_seed(n + k)
    worst = 0.0
    for _ in range(20):
        x = (k + torch.randn(n, generator=g, dtype=F64)).float().double()
        m, var = ref64.emulate_fp32_partials(x, parts)
        want = float(((x - x.mean()) ** 2).mean())
        worst = max(worst, abs(var - want) / want)
    assert worst <= ref64.bn_var_bound(k)
