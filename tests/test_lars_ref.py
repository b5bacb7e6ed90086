"""CPU checks of the LARS feature: the fp64 specification (tests/lars_ref.py) against torch.optim.SGD fed the trust-scaled
gradients, the specification's edge cases, the arguments gca_lars_step refuses before any launch, the job tables, the
optimizer factory and the state formats HipLARS takes and refuses."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lars_ref as ref                   # noqa: E402

SIZES = (1, 255, 700)
GROUPS = ((0.1, 0.0), (0.2, 5e-4), (0.1, 1e-2))            # (lr, weight_decay) per tensor
ADAPT = (False, True, True)
MOM, TAU, EPS = 0.9, 0.001, 1e-8


def to_arena(tensors):
    offs, total = ref.arena_layout(SIZES)
    a = np.zeros(total)
    for o, n, t in zip(offs, SIZES, tensors):
        a[o:o + n] = t.detach().numpy()
    return a


@pytest.mark.parametrize('nesterov', [False, True])
def test_specification_equals_torch_in_fp64(nesterov):
    """Five steps of torch.optim.SGD (fp64, weight_decay 0, momentum 0.9) over three tensors, fed q * (g + wd * w) with q from
    torch.linalg.vector_norm, against the specification on the flat arena: 1e-12 relative (both sides fp64; only the order of
    a few operations differs).  Padding stays exactly 0."""
    gen = torch.Generator().manual_seed(11)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen, dtype=torch.float64)) for n in SIZES]
    opt = torch.optim.SGD([{'params': [p], 'lr': lr} for p, (lr, _) in zip(params, GROUPS)], lr=1.0, momentum=MOM,
                          weight_decay=0.0, nesterov=nesterov)
    offs, total = ref.arena_layout(SIZES)
    lr, wd = [g[0] for g in GROUPS], [g[1] for g in GROUPS]
    p, buf = to_arena(params), np.zeros(total)
    pad = ref.padding_mask(SIZES)
    for t in range(1, 6):
        grads = [torch.randn(n, generator=gen, dtype=torch.float64) for n in SIZES]
        g = to_arena(grads)
        qs = []
        for prm, gr, w_, a in zip(params, grads, wd, ADAPT):
            nw, ng = torch.linalg.vector_norm(prm.detach()), torch.linalg.vector_norm(gr)
            q = TAU * nw / (ng + w_ * nw + EPS) if a and nw > 0 and ng > 0 else torch.tensor(1.0, dtype=torch.float64)
            qs.append(float(q))
            prm.grad = q * (gr + w_ * prm.detach())
        opt.step()
        p, buf, q, norms = ref.lars_step(p, g, buf, SIZES, lr, wd, ADAPT, MOM, nesterov, TAU, EPS)
        assert q[0] == 1.0 and np.abs(q - np.array(qs)).max() <= 1e-12 * max(qs)
        for i, (o, n, prm) in enumerate(zip(offs, SIZES, params)):
            for name, got, want in (('p', p, prm.detach()), ('buf', buf, opt.state[prm]['momentum_buffer'])):
                want = want.numpy()
                err = np.abs(got[o:o + n] - want).max() / np.abs(want).max()
                assert err < 1e-12, (t, i, name, err)
        assert not p[pad].any() and not buf[pad].any()


def test_edge_cases_of_the_specification():
    gen = np.random.default_rng(3)
    sizes = (300, 300, 300)
    offs, total = ref.arena_layout(sizes)
    p, g, buf = gen.standard_normal(total), gen.standard_normal(total), gen.standard_normal(total)
    pad = ref.padding_mask(sizes)
    p[pad] = g[pad] = buf[pad] = 0.0
    p[offs[0]:offs[0] + 300] = 0.0                           # zero weights -> q == 1
    g[offs[1]:offs[1] + 300] = 0.0                           # zero gradient -> q == 1
    lr, wd = (0.1, 0.2, 0.3), (1e-2, 5e-4, 1e-3)
    p1, b1, q, norms = ref.lars_step(p, g, buf, sizes, lr, wd, (True, True, True), MOM, False, TAU, EPS)
    assert q[0] == 1.0 and q[1] == 1.0 and 0.0 < q[2] < 1.0 and norms[0, 0] == 0.0 and norms[1, 1] == 0.0
    want = TAU * norms[2, 0] / (norms[2, 1] + wd[2] * norms[2, 0] + EPS)
    assert q[2] == want
    # a tensor that is not adapted takes the SGD specification, bit for bit
    p2, b2, q2, _ = ref.lars_step(p, g, buf, sizes, lr, wd, (True, True, False), MOM, True, TAU, EPS)
    ps, bs = ref.sgd_step(p, g, buf, ref.expand_chunks(sizes, lr), ref.expand_chunks(sizes, wd), MOM, True)
    assert q2[2] == 1.0 and np.array_equal(p2, ps) and np.array_equal(b2, bs)
    # skip leaves the state equal
    p3, b3, q3, n3 = ref.lars_step(p, g, buf, sizes, lr, wd, (True, True, True), MOM, False, TAU, EPS, skip=True)
    assert np.array_equal(p3, p) and np.array_equal(b3, buf) and q3 is None and n3 is None
    # the clip coefficient is a halved gradient, inside the trust ratio too
    a = ref.lars_step(p, g, buf, sizes, lr, wd, (True, True, True), MOM, False, TAU, EPS, coef=0.5)
    b = ref.lars_step(p, 0.5 * g, buf, sizes, lr, wd, (True, True, True), MOM, False, TAU, EPS)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert a[2][2] > q[2]


def test_lars_step_refuses_bad_arguments_before_launching(pkg):
    """Null operands, n <= 0, n % 256 != 0, tau <= 0, eps < 0 or NaN and momentum outside [0, 1) are GCA_EINVAL (-1) before
    anything is launched: the operands are dummy pointers, so a launch attempt would report GCA_ELAUNCH (-2) or fault."""
    lib = pkg._hip.lib
    d = 1 << 20
    #       p  g  buf n     clr cwd jobs nj par adp np part nrm tr ctr mom nest tau   eps  clip stream
    good = [d, d, d, 1280, d, d, d, 5, d, d, 3, d, d, d, d, 0.9, 0, 0.001, 1e-8, None, None]
    for i in (0, 1, 2, 4, 5, 6, 8, 9, 11, 12, 13, 14):
        args = list(good)
        args[i] = None
        assert lib.gca_lars_step(*args) == -1, i
    for n in (0, -256, 1, 255, 1279, 1284):
        args = list(good)
        args[3] = n
        assert lib.gca_lars_step(*args) == -1, n
    nan = float('nan')
    for i, bad in ((17, 0.0), (17, -0.001), (17, nan), (18, -1e-8), (18, nan), (15, 1.0), (15, -0.1), (15, nan),
                   (7, 0), (7, 2), (7, 6), (10, 0), (10, 6)):         # and table sizes that cannot describe 5 chunks
        args = list(good)
        args[i] = bad
        assert lib.gca_lars_step(*args) == -1, (i, bad)


def test_job_tables(pkg):
    """Jobs never cross a tensor, hold at most J chunks, and cover every chunk of the arena once, in order."""
    ops = pkg.engine.ops
    J = pkg._hip.lib.gca_lars_job_chunks()
    assert J >= 1
    sizes = (1, 255, 256, 257, J * 256, J * 256 + 1, 2 * J * 256 + 300)
    offs, total = ref.arena_layout(sizes)
    jobs, params = ops.lars_job_tables(offs, sizes, total)
    assert jobs.dtype is torch.int32 and params.dtype is torch.int32
    assert [int(x) for x in params[:, 1]] == [1, 1, 1, 1, 1, 2, 3]
    covered = []
    for i, (j0, nj, c0, nc) in enumerate(params.tolist()):
        assert (c0, nc) == (offs[i] // 256, (sizes[i] + 255) // 256)
        mine = jobs[j0:j0 + nj].tolist()
        assert all(t == i and 1 <= n <= J for t, _, n in mine)
        for _, c, n in mine:
            covered.extend(range(c, c + n))
    assert covered == list(range(total // 256)) and int(params[-1, 0] + params[-1, 1]) == jobs.shape[0]
    assert jobs[-1].tolist() == [6, offs[6] // 256 + 2 * J, 2]          # the last job is the partial one
    with pytest.raises(ValueError):
        ops.lars_job_tables([0, 100], [50, 50], 512)


def _cfg(pkg, name):
    cfg = pkg.get_defaults()
    cfg.SOLVER.OPTIMIZER_NAME = name
    return cfg


def test_factory_builds_lars(pkg):
    cfg = _cfg(pkg, 'LARS')
    assert (cfg.SOLVER.LARS_TRUST_COEF, cfg.SOLVER.LARS_EPS) == (0.001, 1e-8)
    cfg.SOLVER.NESTEROV = True
    opt = pkg.make_optimizer(cfg, torch.nn.Linear(3, 2))
    assert type(opt) is pkg.lib.solver.HipLARS and [g['name'] for g in opt.param_groups] == ['weight', 'bias']
    assert [g['lars_adapt'] for g in opt.param_groups] == [True, False]
    w, b = opt.param_groups
    assert (w['lr'], w['weight_decay']) == (cfg.SOLVER.BASE_LR, cfg.SOLVER.WEIGHT_DECAY) and w['initial_lr'] == w['lr']
    assert (b['lr'], b['weight_decay']) == (cfg.SOLVER.BASE_LR * cfg.SOLVER.BIAS_LR_FACTOR, cfg.SOLVER.WEIGHT_DECAY_BIAS)
    for g in (w, b):
        assert (g['momentum'], g['nesterov'], g['trust_coef'], g['lars_eps']) == (cfg.SOLVER.MOMENTUM, True, 0.001, 1e-8)
    assert (opt.momentum, opt.nesterov, opt.trust_coef, opt.eps) == (cfg.SOLVER.MOMENTUM, True, 0.001, 1e-8)
    assert opt.trust.shape == (2,) and opt.trust.dtype is torch.float32
    assert opt.norms.shape == (2, 2) and opt.norms.dtype is torch.float64
    assert opt.plan.adapt.tolist() == [1, 0]
    b['lars_adapt'] = True                                   # the flag is the caller's to change: re-uploaded with the tables
    opt._sync_tables()
    assert opt.plan.adapt.tolist() == [1, 1]
    assert 'LARS' in pkg.lib.solver.build.OPTIMIZERS
    with pytest.raises(NotImplementedError, match='SGD, Adam, AdamW, LARS are built'):
        pkg.make_optimizer(_cfg(pkg, 'RMSprop'), torch.nn.Linear(3, 2))


def test_state_formats(pkg):
    """HipLARS speaks torch.optim.SGD's format: it loads its own state and a plain SGD one (keeping its LARS settings), and
    refuses Adam's with the ValueError that names both formats; one trust_coef for all groups.  (Host tensors: nothing is
    launched by construction, state_dict or load_state_dict.)"""
    lars = pkg.make_optimizer(_cfg(pkg, 'LARS'), torch.nn.Linear(3, 2))
    sgd = pkg.make_optimizer(_cfg(pkg, 'SGD'), torch.nn.Linear(3, 2))
    adam = pkg.make_optimizer(_cfg(pkg, 'Adam'), torch.nn.Linear(3, 2))
    with pytest.raises(ValueError, match='momentum_buffer.*exp_avg'):
        lars.load_state_dict(adam.state_dict())
    with pytest.raises(ValueError, match='momentum_buffer.*exp_avg'):
        adam.load_state_dict(lars.state_dict())
    # a plain SGD state: HipSGD's, and torch's own
    sgd.buf[:6] = torch.arange(6.0)
    sd = sgd.state_dict()
    sd['param_groups'][0]['lr'] = 0.5
    assert 'trust_coef' not in sd['param_groups'][0]
    lars.load_state_dict(sd)
    assert torch.equal(lars.buf[:6], torch.arange(6.0)) and lars.param_groups[0]['lr'] == 0.5
    assert [g['lars_adapt'] for g in lars.param_groups] == [True, False] and lars.trust_coef == 0.001
    assert all(g['trust_coef'] == 0.001 and g['lars_eps'] == 1e-8 for g in lars.param_groups)
    tparams = [torch.nn.Parameter(torch.zeros(2, 3)), torch.nn.Parameter(torch.zeros(2))]
    topt = torch.optim.SGD([{'params': [p]} for p in tparams], lr=0.25, momentum=0.8, nesterov=True)
    for p in tparams:
        p.grad = torch.ones_like(p)
    topt.step()
    lars.load_state_dict(topt.state_dict())
    assert (lars.momentum, lars.nesterov, lars.trust_coef) == (0.8, True, 0.001) and lars.param_groups[1]['lr'] == 0.25
    assert torch.equal(lars.buf[:6], torch.ones(6)) and torch.equal(lars.buf[256:258], torch.ones(2))
    # its own, and back into torch and HipSGD
    sd = lars.state_dict()
    assert set(sd) == {'state', 'param_groups'} and all(set(st) == {'momentum_buffer'} for st in sd['state'].values())
    assert sd['param_groups'][0]['trust_coef'] == 0.001 and sd['param_groups'][0]['params'] == [0]
    lars.load_state_dict(sd)
    topt.load_state_dict(sd)
    sgd.load_state_dict(sd)
    assert sgd.momentum == 0.8 and sgd.nesterov is True
    # one trust coefficient for all groups: refused before anything changes
    before = (lars.buf.clone(), [dict(g) for g in lars.param_groups])
    sd = lars.state_dict()
    sd['param_groups'][1]['trust_coef'] = 0.002
    sd['state'][0]['momentum_buffer'] = torch.full((2, 3), 7.0)
    with pytest.raises(NotImplementedError):
        lars.load_state_dict(sd)
    assert torch.equal(lars.buf, before[0]) and [dict(g) for g in lars.param_groups] == before[1] and lars.trust_coef == 0.001
    for key, bad in (('momentum', 0.5), ('nesterov', False), ('lars_eps', 1e-6)):
        sd = lars.state_dict()
        sd['param_groups'][1][key] = bad
        with pytest.raises(NotImplementedError):
            lars.load_state_dict(sd)
    with pytest.raises(NotImplementedError):
        S = pkg.lib.solver
        m = torch.nn.Linear(3, 2)
        S.HipLARS(m, [{'params': [p], 'lr': 0.1, 'weight_decay': 0.0, 'trust_coef': t} for p, t in zip(m.parameters(), (0.001, 0.002))])
