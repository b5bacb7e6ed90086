"""tests/ressl_ref.py (the fp64 specification of the ReSSL kernels and module) held to torch's fp64 autograd of the literal loss,
the preconditions of the inputs that tests/test_gpu_ressl.py relies on, the wrong variants that must miss the bar, what fp32
arithmetic alone costs on those inputs, the dispatch rule against the library's, the refusals and factories that need no GPU,
and the step oracle (tests/ressl_model.py)."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ressl_ref as rr                   # noqa: E402

BAR = rr.BAR


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def f32(x):
    return float(np.float32(x))


# ----------------------------------------------------------------------------- the specification against autograd
@pytest.mark.parametrize('N,D,K', rr.SPEC_CASES)
@pytest.mark.parametrize('Ts,Tt', rr.TEMPS)
def test_specification_is_the_literal_loss(N, D, K, Ts, Tt):
    q, k, Q = rr.inputs('easy', N, D, K)
    ref = rr.ressl(q, k, Q, 1.0 / Ts, 1.0 / Tt, g=3.0)
    tq, tk, tQ = (torch.from_numpy(np.asarray(x, dtype=np.float64)) for x in (q, k, Q))
    tq.requires_grad_(True)
    tk.requires_grad_(True)
    loss = rr.torch_chain(tq, tk, tQ, Ts, Tt)
    (3.0 * loss).backward()
    assert abs(float(loss.detach()) - ref['loss']) <= 1e-12 * max(abs(ref['loss']), 1.0)
    assert np.abs(tq.grad.numpy() - ref['dq']).max() <= 1e-12 * max(ref['oscale'], 1e-300)
    assert tk.grad is None                                                     # nothing flows to the teacher
    # the second form of the loss, through O_t
    alt = ref['lse_s'] - (1.0 / Ts) * (np.asarray(q, dtype=np.float64) * ref['Ot']).sum(axis=1)
    assert np.abs(alt - ref['row_loss']).max() <= 1e-12 * ref['smax']
    t = (1.0 / Tt) * np.asarray(k, dtype=np.float64) @ np.asarray(Q, dtype=np.float64).T
    p = torch.softmax(torch.from_numpy(t), dim=1)
    ent = -(p * torch.log_softmax(torch.from_numpy(t), dim=1)).sum(dim=1).numpy()
    assert np.abs(ent - ref['row_ent']).max() <= 1e-12 * ref['smax']
    if K == 1:
        assert ref['loss'] == 0.0 and ref['ent'] == 0.0 and not ref['dq'].any()


# ----------------------------------------------------------------------------- preconditions of the GPU inputs
def float_runs():
    for N, D, K in rr.FLOAT_CASES:
        for Ts, Tt in rr.TEMPS:
            for kind in rr.KINDS:
                yield N, D, K, Ts, Tt, kind


def test_preconditions_of_the_float_inputs():
    for N, D, K, Ts, Tt, kind in float_runs():
        q, k, Q = rr.inputs(kind, N, D, K)
        ref = rr.ressl(q, k, Q, f32(1.0 / Ts), f32(1.0 / Tt))
        what = (N, D, K, Ts, Tt, kind)
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in (q, k, Q)), what
        if kind == 'hard':
            assert ref['ent'] < 1e-3, (what, ref['ent'])                        # a peaked teacher
        if kind == 'overflow' and Tt == 0.04:
            assert ref['tmax'] > 200.0, (what, ref['tmax'])                     # exp(t) is inf in fp32 without the max subtraction
            with np.errstate(over='ignore'):
                assert np.isinf(np.exp(np.float32(ref['tmax'])))
        if K > 1:
            assert np.abs(ref['dq']).max() >= 0.01 * ref['oscale'], (what, np.abs(ref['dq']).max() / ref['oscale'])
    # the planted columns are distinct
    for N, D, K in rr.FLOAT_CASES:
        cols = [(7 * i + 3) % K if K > 7 else i for i in range(min(N, K))]
        assert len(set(cols)) == len(cols), (N, D, K)


def test_fp32_arithmetic_alone_is_inside_the_bar():
    """The same formulas in plain fp32 numpy: the reference itself leaves room under the kernel bar on every float input."""
    worst = dict(loss=0.0, lse=0.0, dq=0.0)
    for N, D, K, Ts, Tt, kind in float_runs():
        q, k, Q = rr.inputs(kind, N, D, K)
        its, itt = f32(1.0 / Ts), f32(1.0 / Tt)
        ref, got = rr.ressl(q, k, Q, its, itt), rr.ressl_f32(q, k, Q, its, itt)
        e = dict(loss=max(np.abs(got['row_loss'] - ref['row_loss']).max(), abs(got['loss'] - ref['loss']), abs(got['ent'] - ref['ent'])) / ref['smax'],
                 lse=max(np.abs(got['lse_s'] - ref['lse_s']).max(), np.abs(got['lse_t'] - ref['lse_t']).max()) / ref['smax'],
                 dq=np.abs(got['dq'] - ref['dq']).max() / ref['oscale'])
        for n in worst:
            worst[n] = max(worst[n], float(e[n]))
    print('MEASURED ressl cpu fp32 restatement, worst over the float inputs: %s' % ' '.join('%s %.3e' % kv for kv in worst.items()))
    assert max(worst.values()) <= BAR


# ----------------------------------------------------------------------------- wrong variants
@pytest.mark.parametrize('N,D,K', [(33, 128, 100), (64, 128, 3075)])
def test_wrong_variants_miss_the_bar_by_100x(N, D, K):
    assert K % 32 != 0 and N > 1
    Ts, Tt = rr.TEMPS[0]
    g, index = 3.0, 5
    q, k, Q = rr.inputs('easy', N, D, K)
    ref = rr.ressl(q, k, Q, f32(1.0 / Ts), f32(1.0 / Tt), g)
    seen = {}
    for name, w in rr.wrong_variants(q, k, Q, f32(1.0 / Ts), f32(1.0 / Tt), g, index).items():
        seen[name] = max(abs(w['loss'] - ref['loss']) / (BAR * ref['smax']), np.abs(w['dq'] - ref['dq']).max() / (BAR * ref['oscale']))
    print('MEASURED ressl wrong variants N=%d D=%d K=%d, in bars: %s' % (N, D, K, ', '.join('%s %.0f' % kv for kv in seen.items())))
    assert len(seen) == 6 and min(seen.values()) > 100.0, seen


# ----------------------------------------------------------------------------- dispatch
def c_path(lib, which, N, D, K, al):
    w, s = C.c_int32(-1), C.c_int32(-1)
    rc = getattr(lib, 'gca_ressl_%s_path' % which)(N, D, K, int(al), C.addressof(w), C.addressof(s))
    return ('generic', 'fast')[rc] if rc in (0, 1) else rc, w.value, s.value


def test_path_rule_is_the_librarys(pkg):
    lib = pkg._hip.lib
    for N in (1, 5, 32, 33, 64, 97, 256, 4096, 65536):
        for D in (1, 8, 32, 127, 128, 130, 256, 260):
            for K in (1, 7, 31, 32, 33, 65, 100, 129, 200, 1000, 3075, 65536, 98304):
                if not rr.sizes_ok(N, D, K):
                    continue
                for al in (False, True):
                    for which, sides in (('fwd', 1), ('bwd', 2)):
                        want = rr.path(N, D, K, al, sides)
                        assert c_path(lib, which, N, D, K, al) == want[:3], (which, N, D, K, al)
                        kt, splits, tps = -(-K // 32), want[2], want[3]
                        assert 1 <= splits <= kt and (splits - 1) * tps < kt <= splits * tps      # no split is empty
                assert lib.gca_ressl_fwd_ws_bytes(N, D, K) >= 24 * N * max(rr.path(N, D, K, a, 1)[2] for a in (False, True))
                assert lib.gca_ressl_bwd_ws_bytes(N, D, K) >= 8 * N * D * max(rr.path(N, D, K, a, 2)[2] for a in (False, True))
    assert [rr.path(N, D, K)[0] for N, D, K in rr.FLOAT_CASES] == rr.FLOAT_PATHS
    assert rr.path(64, 128, 3075)[2] > 1 and 97 % rr.path(64, 128, 3075)[3] != 0          # several splits, the last one short
    for N, D, K in ((0, 8, 8), (-1, 8, 8), (65537, 8, 8), (8, 0, 8), (8, 8, 0), (8, 8, 2 ** 31), (65536, 32768, 8), (8, 32768, 65536)):
        for which in ('fwd', 'bwd'):
            assert getattr(lib, 'gca_ressl_%s_path' % which)(N, D, K, 1, None, None) == -1
            assert getattr(lib, 'gca_ressl_%s_ws_bytes' % which)(N, D, K) == -1


def test_refused_entry_arguments_without_a_device(pkg):
    """The entries check sizes, scalars, NULLs, the workspace and overlaps before anything is launched: host pointers are enough."""
    lib = pkg._hip.lib
    N, D, K = 4, 8, 6
    buf = (C.c_float * 8192)()
    base = C.addressof(buf)
    q, k, Q, lse, rl, out, dq, ws = (base + 4 * o for o in (0, 64, 128, 256, 320, 384, 448, 1024))
    nf, nb = lib.gca_ressl_fwd_ws_bytes(N, D, K), lib.gca_ressl_bwd_ws_bytes(N, D, K)
    assert 0 < nf <= 4 * 1024 and 0 < nb <= 4 * 4096

    def fwd(**kw):
        a = dict(q=q, k=k, Q=Q, N=N, D=D, K=K, its=10.0, itt=25.0, lse=lse, rl=rl, out=out, ws=ws, wb=nf)
        a.update(kw)
        return lib.gca_ressl_fwd(a['q'], a['k'], a['Q'], a['N'], a['D'], a['K'], a['its'], a['itt'], a['lse'], a['rl'], a['out'],
                                 a['ws'], a['wb'], None)
    for kw in (dict(N=0), dict(N=65537), dict(D=0), dict(K=0), dict(K=2 ** 31), dict(its=0.0), dict(its=-1.0), dict(its=float('nan')),
               dict(its=float('inf')), dict(itt=0.0), dict(itt=float('nan')), dict(itt=float('inf')), dict(q=None), dict(k=None),
               dict(Q=None), dict(lse=None), dict(rl=None), dict(out=None), dict(ws=None), dict(wb=nf - 1), dict(lse=q), dict(rl=k + 4),
               dict(out=Q + 4 * (K * D - 1)), dict(rl=lse + 4 * (2 * N - 1)), dict(out=rl), dict(out=lse + 4)):
        assert fwd(**kw) == -1, kw

    def bwd(**kw):
        a = dict(q=q, k=k, Q=Q, lse=lse, N=N, D=D, K=K, its=10.0, itt=25.0, dq=dq, ws=ws, wb=nb)
        a.update(kw)
        return lib.gca_ressl_bwd(a['q'], a['k'], a['Q'], a['lse'], a['N'], a['D'], a['K'], a['its'], a['itt'], None, 1.0, a['dq'],
                                 a['ws'], a['wb'], None)
    for kw in (dict(N=0), dict(N=65537), dict(D=0), dict(K=0), dict(K=2 ** 31), dict(its=0.0), dict(its=float('nan')), dict(its=float('inf')),
               dict(itt=-2.0), dict(itt=float('nan')), dict(q=None), dict(k=None), dict(Q=None), dict(lse=None), dict(dq=None), dict(ws=None),
               dict(wb=nb - 1), dict(dq=q), dict(dq=k + 4), dict(dq=Q + 4 * (K * D - 1)), dict(dq=lse)):
        assert bwd(**kw) == -1, kw


# ----------------------------------------------------------------------------- the host layers
def test_ops_refuse_before_any_device_is_touched(pkg):
    ops = pkg.engine.ops
    z, Q = torch.zeros(4, 8), torch.zeros(6, 8)
    bad_shapes = ((z, torch.zeros(3, 8), Q), (z, z, torch.zeros(6, 9)), (z.double(), z, Q), (z, z, Q.double()), (z[0], z[0], Q), (z, z, Q[0]),
                  (torch.zeros(0, 8), torch.zeros(0, 8), Q), (z, z, torch.zeros(0, 8)),
                  (torch.zeros(65537, 1), torch.zeros(65537, 1), torch.zeros(2, 1)))
    for args in bad_shapes:
        with pytest.raises(ValueError, match='ressl_fwd'):
            ops.ressl_fwd(*args, 10.0, 25.0)
        with pytest.raises(ValueError, match='ressl_bwd'):
            ops.ressl_bwd(*args, torch.zeros(2 * max(args[0].shape[0], 1)), 10.0, 25.0)
    for bad in (0.0, -1.0, float('nan'), float('inf'), 1e39):
        for ts in ((bad, 25.0), (10.0, bad)):
            with pytest.raises(ValueError, match='ressl_fwd'):
                ops.ressl_fwd(z, z, Q, *ts)
            with pytest.raises(ValueError, match='ressl_bwd'):
                ops.ressl_bwd(z, z, Q, torch.zeros(8), *ts)
    with pytest.raises(ValueError, match='row_lse'):
        ops.ressl_bwd(z, z, Q, torch.zeros(4), 10.0, 25.0)
    with pytest.raises(ValueError, match='row_lse'):
        ops.ressl_bwd(z, z, Q, torch.zeros(8).double(), 10.0, 25.0)
    for gs in (float('inf'), float('nan'), 1e39):
        with pytest.raises(ValueError, match='gscale_host'):
            ops.ressl_bwd(z, z, Q, torch.zeros(8), 10.0, 25.0, gscale_host=gs)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.ressl_fwd(z, z, Q, 10.0, 25.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.ressl_bwd(z, z, Q, torch.zeros(8), 10.0, 25.0)


def ressl_cfg(pkg, **solver):
    from tests import parity
    import ressl_model as rm
    parity.register_tiny(pkg)
    cfg = parity.make_cfg(pkg, 'R2P1D10T', 'ressl', rm.OUT, rm.QUEUE_K, 8, **solver)
    cfg.CONTRAST.RESSL_TS, cfg.CONTRAST.RESSL_TT, cfg.CONTRAST.ALPHA = rm.TS, rm.TT, rm.ALPHA
    return cfg


def test_factories(pkg):
    from tests import parity
    import ressl_model as rm
    ReSSLLoss = importlib.import_module(pkg.__name__ + '.lib.memory.ressl').ReSSLLoss
    build = importlib.import_module(pkg.__name__ + '.lib.modeling.build')
    d = pkg.get_defaults().CONTRAST
    assert (d.RESSL_TS, d.RESSL_TT) == (0.1, 0.04)                              # the paper's values
    cfg = ressl_cfg(pkg)
    torch.manual_seed(3)
    c = pkg.create_contrast(cfg, 100)
    assert isinstance(c, ReSSLLoss) and (c.Ts, c.Tt, c.K, c.index) == (rm.TS, rm.TT, rm.QUEUE_K, 0) and c.ent is None
    assert list(c.state_dict()) == ['memory'] and tuple(c.memory.shape) == (rm.QUEUE_K, rm.OUT)
    assert float((c.memory.norm(dim=1) - 1).abs().max()) < 1e-6                 # normalised randn, as RGBMoCo's
    torch.manual_seed(3)
    moco = pkg.create_contrast(parity.make_cfg(pkg, 'R2P1D10T', 'moco', rm.OUT, rm.QUEUE_K, 8), 100)
    assert torch.equal(moco.memory, c.memory) and list(moco.state_dict()) == list(c.state_dict())
    for bad in (0.0, -0.2, float('nan'), float('inf'), 1e-39):
        for kw in (dict(Ts=bad), dict(Tt=bad)):
            with pytest.raises(ValueError, match='ReSSLLoss'):
                ReSSLLoss(**{**dict(n_dim=8, K=16, Ts=0.1, Tt=0.04), **kw})
            bad_cfg = ressl_cfg(pkg)
            setattr(bad_cfg.CONTRAST, 'RESSL_' + list(kw)[0].upper(), bad)
            with pytest.raises(ValueError, match='ReSSLLoss'):
                pkg.create_contrast(bad_cfg, 0)
    with pytest.raises(ValueError, match='sharper'):                            # the teacher must be the sharper one ...
        ReSSLLoss(8, 16, Ts=0.04, Tt=0.1)
    assert ReSSLLoss(8, 16, Ts=0.2, Tt=0.2).Tt == 0.2                           # ... equal is allowed
    for bad in (dict(n_dim=0), dict(K=0), dict(K=2.5), dict(n_dim=True)):
        with pytest.raises(ValueError, match='ReSSLLoss'):
            ReSSLLoss(**{**dict(n_dim=8, K=16), **bad})
    z = torch.zeros(4, rm.OUT)
    for args in ((z, torch.zeros(4, 9)), (z, torch.zeros(5, rm.OUT)), (z[0], z[0])):
        with pytest.raises(ValueError, match='ReSSLLoss'):
            c(*args)
    big = torch.zeros(rm.QUEUE_K + 1, rm.OUT)
    with pytest.raises(ValueError, match='cannot enqueue'):                     # before any device is touched
        c(z, z, all_k=big)
    assert c.index == 0
    with pytest.raises(NotImplementedError, match='mem not suported: nope'):
        pkg.create_contrast(parity.make_cfg(pkg, 'R2P1D10T', 'nope', 32, 16, 8), 0)
    # the model factory: MoCo's model and a teacher of the same layout
    torch.manual_seed(5)
    model, ema = build.create_visual_model(cfg)
    torch.manual_seed(5)
    m2, e2 = build.create_visual_model(parity.make_cfg(pkg, 'R2P1D10T', 'moco', rm.OUT, rm.QUEUE_K, 8))
    assert ema is not None and list(model.state_dict()) == list(ema.state_dict()) == list(m2.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), m2.state_dict().values()))
    # the oracle reads the same state
    rm.oracle_ressl('R2P1D10T', 8, rm.OUT, {k: v.detach().clone() for k, v in model.state_dict().items()})


def test_trainer_is_exported_and_refuses_without_a_device(pkg):
    from tests import parity
    parity.register_tiny(pkg)
    assert issubclass(pkg.ReSSLTrainer, pkg.MoCoTrainer) and pkg.ReSSLTrainer is not pkg.MoCoTrainer
    own = [n for n in vars(pkg.ReSSLTrainer) if not n.startswith('__') or n == '__init__']
    assert sorted(own) == ['__init__', '_phase_query_rest']
    for mem in ('simsiam', 'moco', 'simclr', 'mocov3', 'nnclr', 'bank'):
        with pytest.raises(ValueError, match='ressl'):
            pkg.ReSSLTrainer(parity.make_cfg(pkg, 'R2P1D10T', mem, 32, 16, 8), 'cpu')
    with pytest.raises(NotImplementedError, match='one GPU'):
        pkg.ReSSLTrainer(ressl_cfg(pkg), 'cpu', ctx=pkg.parallel.DistCtx(force_active=True))
    for other in (pkg.SimCLRTrainer, pkg.DINOTrainer, pkg.MoCoV3Trainer, pkg.NNCLRTrainer):
        with pytest.raises(ValueError):
            other(ressl_cfg(pkg), 'cpu')


# ----------------------------------------------------------------------------- the step oracle
def oracle_run(pkg, state=None):
    """The three oracle steps the GPU trainer test follows."""
    import ressl_model as rm
    cfg = ressl_cfg(pkg, WARMUP_FACTOR=1.0, BASE_LR=rm.LR)
    if state is None:                                                            # the trainer's own initialisation, on the CPU
        build = importlib.import_module(pkg.__name__ + '.lib.modeling.build')
        torch.manual_seed(rm.MODEL_SEED)
        state = {k: v.detach().clone() for k, v in build.create_visual_model(cfg)[0].state_dict().items()}
    xs, shs = rm.clip_batches(), rm.shuffles()
    model, ema = rm.oracle_ressl('R2P1D10T', 8, rm.OUT, state)
    Q0 = rm.queue0()
    Q = Q0.double().clone()
    losses, index = rm.oracle_steps(model, ema, Q, 0, [x.double() for x in xs], shs, rm.LR, rm.ALPHA, rm.TS, rm.TT)
    return dict(cfg=cfg, state=state, xs=xs, shs=shs, Q0=Q0, losses=losses, Q=Q, index=index, model=model, ema=ema)


def test_step_oracle(pkg):
    import ressl_model as rm
    run = oracle_run(pkg)
    assert run['index'] == (3 * rm.CLIP[0]) % rm.QUEUE_K == 4 and all(np.isfinite(run['losses']))
    Q, Q0 = run['Q'], run['Q0'].double()
    assert bool(((Q - Q0).abs().amax(dim=1) > 0).all())                         # 24 rows into 20: every row was overwritten
    assert float((Q.norm(dim=1) - 1).abs().max()) < 1e-9                        # the teacher's rows are unit rows
    # the teacher moved, by the EMA and not by the optimizer: it stays within (1 - alpha^3) of the student's total move
    p0 = torch.cat([run['state'][n].double().reshape(-1) for n, _ in run['model'].named_parameters()])
    ps = torch.cat([p.detach().reshape(-1) for p in run['model'].parameters()])
    pt = torch.cat([p.detach().reshape(-1) for p in run['ema'].parameters()])
    assert 0 < float((pt - p0).abs().max()) < float((ps - p0).abs().max())
    # the loss of step 1 is the specification's on the oracle's own rows
    model, ema = rm.oracle_ressl('R2P1D10T', 8, rm.OUT, run['state'])
    loss, q, k = rm.model_loss(model, ema, run['xs'][0].double(), Q0, rm.TS, rm.TT)
    ref = rr.ressl(q.detach().numpy(), k.numpy(), Q0.numpy(), 1.0 / rm.TS, 1.0 / rm.TT)
    assert abs(float(loss.detach()) - run['losses'][0]) <= 1e-12 and abs(ref['loss'] - run['losses'][0]) <= 1e-12 * ref['smax']
