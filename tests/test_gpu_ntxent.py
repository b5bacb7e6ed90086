"""gca_ntxent_fwd / gca_ntxent_bwd, ops.ntxent_*, lib.memory.NTXent, the SimCLR wrapper and SimCLRTrainer on the device, against
tests/ntxent_ref.py (fp64 numpy) and tests/ntxent_model.py (the fp64 torch oracle of the model).

Exact inputs (entries k / 8, inv_T = 16: every s[i,j] is the same number in fp32 and fp64, tests/test_ntxent_ref.py): pos_logit
bit for bit, rank exactly -- ties with the positive and with the diagonal included -- lse and loss within 1e-5 * max|s|, the
suite's bar on the logit scale.  max|s| is 16 D there, far past exp's fp32 range: the max subtraction is exercised.

Float inputs (unit rows, T = 0.07 and 0.5): loss, lse and dz within 1e-5 (max-norm relative) of the fp64 specification on the
same fp32 inputs, the suite's per-op bar; the unfused fp32 torch chain sits at 2e-7 .. 9e-7 on dz at these sizes, so the bar
leaves a 10x margin over fp32 arithmetic while a wrong mask, a missing P^T term or a wrong positive misses it by orders of
magnitude.  The `hard` inputs (row norms spread 4x, rows sharing a direction, one row equal to its positive) run at T = 0.5,
where their logits stay below 8.5 in magnitude -- the scale of unit rows at T = 0.125 -- and are held to the same bar.

Measured on an MI355X (printed as `MEASURED ntxent ...`), worst over the cases:
    exact inputs   |lse - fp64| 7.42e-6 (b = 33, D = 128; bar 2.05e-2)    |loss - fp64| 6.77e-6 (b = 17, D = 128; bar 2.05e-2)
    unit rows      loss 8.61e-8 (b = 256, T = 0.5)    lse 1.96e-7 (b = 256, T = 0.5)    dz 2.27e-7 (b = 5, T = 0.07)    [bar 1e-5]
    hard rows      loss 3.75e-8    lse 1.23e-7    dz 5.72e-7 (fast path, b = 33), 4.16e-7 (generic, b = 40, D = 130)    [bar 1e-5]
    model          loss of SimCLR.forward against the fp64 oracle: 7.36e-7 relative    [bar 1e-3]
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ntxent_ref as nr                  # noqa: E402
import ntxent_model as nm                # noqa: E402
from parity import make_cfg, register_tiny, rel           # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = -1
BAR = 1e-5


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def c_fwd(pkg, z, inv_T, want_pos=True, want_rank=True):
    """gca_ntxent_fwd itself -> (loss, lse, pos_logit | None, rank | None) as device tensors."""
    N, D = z.shape
    lib, H = pkg._hip.lib, pkg._hip
    lse = torch.empty(N, device=DEV)
    pos = torch.empty(N, device=DEV) if want_pos else None
    rank = torch.empty(N, dtype=torch.int32, device=DEV) if want_rank else None
    loss = torch.empty(1, device=DEV)
    ws = torch.empty(lib.gca_ntxent_ws_bytes(N, D), dtype=torch.uint8, device=DEV)
    rc = lib.gca_ntxent_fwd(H.ptr(z), N, D, inv_T, H.ptr(lse), H.ptr(pos), H.ptr(rank), H.ptr(loss), H.ptr(ws), H.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return loss, lse, pos, rank


def aligned(*ts):
    return all(t.data_ptr() % 16 == 0 for t in ts)


# ----------------------------------------------------------------------------- 1. the kernels against the specification
@pytest.mark.parametrize('case,path', list(zip(nr.EXACT_CASES, nr.EXACT_PATHS)), ids=['b%d-D%d' % c for c in nr.EXACT_CASES])
def test_exact_inputs(pkg, case, path):
    b, D = case
    z = nr.exact_inputs(b, D)
    ref = nr.ntxent(z, nr.EXACT_INV_T)
    zd = dev(z)
    assert nr.ntxent_path(2 * b, D, aligned(zd))[0] == path
    loss, lse, pos, rank = c_fwd(pkg, zd, nr.EXACT_INV_T)
    assert np.array_equal(pos.cpu().numpy().astype(np.float64), ref['sp'])
    assert np.array_equal(rank.cpu().numpy().astype(np.int64), ref['rank'])
    smax = float(np.abs(ref['s']).max())
    e_lse, e_loss = float(np.abs(lse.cpu().numpy().astype(np.float64) - ref['lse']).max()), abs(float(loss) - ref['loss'])
    print('MEASURED ntxent exact b=%d D=%d: |lse err| %.3e |loss err| %.3e (bar %.3e)' % (b, D, e_lse, e_loss, BAR * smax))
    assert e_lse <= BAR * smax and e_loss <= BAR * smax
    # the gradient of the same inputs (N = 2: exactly zero)
    dz = pkg.engine.ops.ntxent_bwd(zd, lse, nr.EXACT_INV_T)
    torch.cuda.synchronize()
    if b == 1:
        assert float(loss) == 0.0 and float(dz.abs().max()) == 0.0 and torch.equal(lse, pos)
    else:
        assert rel(dz, torch.from_numpy(ref['dz'])) <= BAR


def float_case(pkg, z, T, tag):
    inv_T = 1.0 / T
    ref = nr.ntxent(z, np.float32(inv_T))
    zd = dev(z)
    loss, lse, rank = pkg.engine.ops.ntxent_fwd(zd, inv_T, want_rank=True)
    dz = pkg.engine.ops.ntxent_bwd(zd, lse, inv_T)
    torch.cuda.synchronize()
    e = (abs(float(loss) - ref['loss']) / abs(ref['loss']), rel(lse, torch.from_numpy(ref['lse'])), rel(dz, torch.from_numpy(ref['dz'])))
    print('MEASURED ntxent %s T=%g: rel_err loss %.3e lse %.3e dz %.3e' % (tag, T, e[0], e[1], e[2]))
    assert max(e) <= BAR, e
    # rank wherever no negative sits within the kernel's own rounding of the positive
    gap = np.abs(ref['s'] - ref['sp'][:, None])
    N = z.shape[0]
    gap[np.arange(N), np.arange(N)] = np.inf
    gap[np.arange(N), nr.pos_index(N)] = np.inf
    clear = gap.min(axis=1) > 1e-5 * np.abs(ref['s']).max() if N > 2 else np.ones(N, dtype=bool)
    assert clear.sum() >= N // 2
    assert np.array_equal(rank.cpu().numpy()[clear], ref['rank'][clear])
    return e


@pytest.mark.parametrize('T', nr.FLOAT_TS)
@pytest.mark.parametrize('b,D', nr.FLOAT_CASES)
def test_float_inputs(pkg, b, D, T):
    assert nr.ntxent_path(2 * b, D)[0] == 'fast'
    float_case(pkg, nr.float_inputs(b, D), T, 'unit b=%d D=%d' % (b, D))


@pytest.mark.parametrize('b,D', [(33, 128), (40, 130)], ids=['fast', 'generic'])
def test_mistakes_that_must_show(pkg, b, D):
    """Row norms spread 4x, P far from symmetric, row 0 equal to its positive (properties: tests/test_ntxent_ref.py)."""
    float_case(pkg, nr.float_inputs(b, D, hard=True), 0.5, 'hard b=%d D=%d' % (b, D))


def test_unaligned_rows_take_the_generic_path_to_the_same_answer(pkg):
    b, D = 17, 128
    z = nr.float_inputs(b, D)
    ref = nr.ntxent(z, np.float32(2.0))
    buf = torch.zeros(2 * b * D + 1, device=DEV)
    zo = buf[1:].view(2 * b, D)
    zo.copy_(dev(z))
    assert not aligned(zo) and nr.ntxent_path(2 * b, D, aligned(zo))[0] == 'generic'
    loss, lse, _, _ = c_fwd(pkg, zo, 2.0)
    assert rel(lse, torch.from_numpy(ref['lse'])) <= BAR and abs(float(loss) - ref['loss']) <= BAR * abs(ref['loss'])


@pytest.mark.parametrize('b,D', [(33, 128), (100, 128), (33, 130)])
def test_deterministic(pkg, b, D):
    zd = dev(nr.float_inputs(b, D, seed=3))
    ops = pkg.engine.ops
    outs = []
    for _ in range(2):
        loss, lse, rank = ops.ntxent_fwd(zd, 1.0 / 0.07, want_rank=True)
        outs.append((loss, lse, rank, ops.ntxent_bwd(zd, lse, 1.0 / 0.07)))
    torch.cuda.synchronize()
    for a, b_ in zip(*outs):
        assert torch.equal(bits(a), bits(b_))


@pytest.mark.parametrize('b,D', [(33, 128), (100, 128), (33, 130)])
def test_gradient_scale(pkg, b, D):
    zd = dev(nr.float_inputs(b, D, seed=5))
    ops = pkg.engine.ops
    _, lse, _ = ops.ntxent_fwd(zd, 1.0 / 0.07)
    one = ops.ntxent_bwd(zd, lse, 1.0 / 0.07)
    scaled = ops.ntxent_bwd(zd, lse, 1.0 / 0.07, gscale_dev=torch.tensor([1024.0, 7.0], device=DEV))
    half = ops.ntxent_bwd(zd, lse, 1.0 / 0.07, gscale_host=0.5)
    both = ops.ntxent_bwd(zd, lse, 1.0 / 0.07, gscale_dev=torch.tensor([4.0], device=DEV), gscale_host=0.25)
    torch.cuda.synchronize()
    assert float(one.abs().max()) > 0
    assert torch.equal(bits(scaled), bits(one * 1024.0)) and torch.equal(bits(half), bits(one * 0.5))
    assert torch.equal(bits(both), bits(one))


def test_refused_arguments_touch_nothing(pkg):
    lib, H = pkg._hip.lib, pkg._hip
    z = dev(nr.float_inputs(4, 8))
    SENT = 12345.0
    lse, pos, loss, dz = (torch.full((n,), SENT, device=DEV) for n in (9, 9, 1, 9 * 8))
    rank = torch.full((9,), 777, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(lib.gca_ntxent_ws_bytes(8, 8), 1 << 16), dtype=torch.uint8, device=DEV)
    p = H.ptr
    nan, inf = float('nan'), float('inf')

    def fwd(zp=p(z), N=8, D=8, inv_T=2.0, lp=p(lse), lo=p(loss), w=p(ws)):
        return lib.gca_ntxent_fwd(zp, N, D, inv_T, lp, p(pos), p(rank), lo, w, H.stream())

    def bwd(zp=p(z), N=8, D=8, inv_T=2.0, lp=p(lse), dp=p(dz), w=p(ws)):
        return lib.gca_ntxent_bwd(zp, lp, N, D, inv_T, None, 1.0, dp, w, H.stream())

    for f in (fwd, bwd):
        for kw in (dict(N=7), dict(N=9), dict(N=0), dict(N=-2), dict(N=65538, D=1), dict(D=0), dict(D=-1), dict(N=65536, D=32768),
                   dict(inv_T=0.0), dict(inv_T=-1.0), dict(inv_T=inf), dict(inv_T=nan), dict(zp=None), dict(lp=None), dict(w=None)):
            assert f(**kw) == EINVAL, (f.__name__, kw)
    assert fwd(lo=None) == EINVAL and bwd(dp=None) == EINVAL
    torch.cuda.synchronize()
    for t in (lse, pos, loss, dz):
        assert float(t.min()) == SENT == float(t.max())
    assert int(rank.min()) == 777 == int(rank.max())
    # the optional outputs may be NULL, and the accepted call writes exactly N rows
    assert lib.gca_ntxent_fwd(p(z), 8, 8, 2.0, p(lse), None, None, p(loss), p(ws), H.stream()) == 0
    torch.cuda.synchronize()
    assert float(lse[8]) == SENT and float(lse[:8].max()) < SENT and float(pos.min()) == SENT


def test_ops_refuse_what_the_entry_refuses(pkg):
    ops = pkg.engine.ops
    with pytest.raises(ValueError):
        ops.ntxent_fwd(torch.zeros(3, 8, device=DEV), 2.0)
    with pytest.raises(ValueError):
        ops.ntxent_fwd(torch.zeros(4, 8, device=DEV), float('nan'))
    with pytest.raises(ValueError):
        ops.ntxent_bwd(torch.zeros(4, 8, device=DEV), torch.zeros(3, device=DEV), 2.0)


def test_capturable_in_a_graph(pkg):
    """Forward and backward inside one captured graph: replays track the static input and equal the eager bits."""
    ops = pkg.engine.ops
    zs = torch.empty(200, 128, device=DEV)
    zs.copy_(dev(nr.float_inputs(100, 128)))
    eager = ops.ntxent_fwd(zs, 2.0, want_rank=True)
    eager_dz = ops.ntxent_bwd(zs, eager[1], 2.0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss, lse, rank = ops.ntxent_fwd(zs, 2.0, want_rank=True)
        dz = ops.ntxent_bwd(zs, lse, 2.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(loss), bits(eager[0])) and torch.equal(rank, eager[2]) and torch.equal(bits(dz), bits(eager_dz))
    zs.copy_(dev(nr.float_inputs(100, 128, seed=9)))
    g.replay()
    torch.cuda.synchronize()
    ref = nr.ntxent(zs.cpu().numpy(), np.float32(2.0))
    assert abs(float(loss) - ref['loss']) <= BAR * abs(ref['loss']) and rel(dz, torch.from_numpy(ref['dz'])) <= BAR
    g.reset()


# ----------------------------------------------------------------------------- 2. the module
def test_module_forward_backward(pkg):
    import importlib
    NTXent = importlib.import_module(pkg.__name__ + '.lib.memory.ntxent').NTXent
    b, D, T = 33, 128, 0.07
    z = nr.float_inputs(b, D, seed=2)
    ref = nr.ntxent(z, np.float32(1.0 / T), g=3.0)
    z1, z2 = dev(z[:b]).requires_grad_(True), dev(z[b:]).requires_grad_(True)
    crit = NTXent(T)
    loss = crit(z1, z2)
    assert loss.dim() == 0 and abs(float(loss.detach()) - ref['loss']) <= BAR * abs(ref['loss'])
    (loss * 3.0).backward()
    torch.cuda.synchronize()
    assert rel(z1.grad, torch.from_numpy(ref['dz'][:b])) <= BAR and rel(z2.grad, torch.from_numpy(ref['dz'][b:])) <= BAR
    assert crit.rank.dtype is torch.int32 and tuple(crit.rank.shape) == (2 * b,)
    assert int(crit.rank.sum()) == int(ref['rank'].sum())


# ----------------------------------------------------------------------------- 3. model and trainer
CLIP = (8, 6, 8, 48, 48)


def clips(seed, n=4):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*CLIP, generator=gen).to(DEV) for _ in range(n)]


def simclr_cfg(pkg, **solver):
    register_tiny(pkg)
    return make_cfg(pkg, 'R2P1D10T', 'simclr', 32, 16, 8, **solver)


def test_model_loss_against_the_fp64_oracle(pkg):
    tr = pkg.SimCLRTrainer(simclr_cfg(pkg), DEV, use_graph=False, seed=21)
    state = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    x = clips(31, 1)[0]
    oracle = nm.oracle_simclr('R2P1D10T', 8, 32, state)
    want, z64 = nm.simclr_loss(oracle, x.cpu().double(), 0.07)
    want = want.detach()
    with torch.no_grad():
        got = tr.model(x)
    torch.cuda.synchronize()
    rank = tr.model.model.rank.cpu().numpy()
    err = abs(float(got) - float(want)) / abs(float(want))
    print('MEASURED ntxent model loss %.6f vs oracle %.6f: rel err %.3e' % (float(got), float(want), err))
    assert got.dim() == 0 and err < 1e-3
    ref = nr.ntxent(z64.detach().numpy(), 1.0 / 0.07)
    assert np.abs(rank - ref['rank']).max() <= 1 and tuple(rank.shape) == (16,)
    # differentiable as one node: every parameter receives a gradient
    tr.optimizer.zero_grad()
    tr.model(x).backward()
    torch.cuda.synchronize()
    assert float(tr.arena.grad.abs().max()) > 0 and bool(torch.isfinite(tr.arena.grad).all())
    tr.close()


def test_trainer_graph_equals_eager_and_loss_decreases(pkg):
    cfg = simclr_cfg(pkg, WARMUP_FACTOR=1.0, BASE_LR=0.03)
    x = clips(33, 1)[0]
    runs = {}
    for use_graph in (True, False):
        tr = pkg.SimCLRTrainer(cfg, DEV, use_graph=use_graph, seed=7)
        losses, ranks = [], []
        for _ in range(5):
            out = tr.train_step(x)
            torch.cuda.synchronize()
            assert set(out) >= {'loss', 'rank'} and out['rank'].dtype is torch.int32 and tuple(out['rank'].shape) == (16,)
            losses.append(out['loss'].detach().clone())
            ranks.append(out['rank'].detach().clone())
        assert (tr._segments[0].graph is not None) == use_graph
        runs[use_graph] = (losses, ranks, tr.arena.flat.detach().clone())
        sd = tr.state_dict()
        assert sd['contrast'] is None and 'model_ema' not in sd
        tr.close()
    for a, b_ in zip(runs[True][0][:3] + runs[True][1][:3], runs[False][0][:3] + runs[False][1][:3]):
        assert torch.equal(bits(a), bits(b_))
    assert torch.equal(bits(runs[True][2]), bits(runs[False][2]))
    vals = [float(v) for v in runs[False][0]]
    print('MEASURED ntxent trainer losses on one repeated batch: %s' % ' '.join('%.4f' % v for v in vals))
    assert all(np.isfinite(vals)) and vals[-1] < vals[0]


def test_checkpoint_resume_is_exact_and_loads_downstream(pkg):
    import copy
    import classify_model as cm
    from test_gpu_adam import action_cfg, assert_resume_is_exact
    cm.register()
    cfg = simclr_cfg(pkg)
    a, b_, sd = assert_resume_is_exact(lambda seed: pkg.SimCLRTrainer(cfg, DEV, use_graph=False, seed=seed), clips(13, 5),
                                       ('epoch', 'state_dict', 'optimizer', 'contrast'))
    assert sd['contrast'] is None and 'model_ema' not in sd
    assert all(k.startswith(('model.encoder.', 'model.proj_head.')) for k in sd['state_dict'])
    sd = copy.deepcopy(sd)
    from tests import parity
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
    a.close(), b_.close()


def test_trainer_refusals(pkg):
    register_tiny(pkg)
    for mem in ('simsiam', 'moco'):
        with pytest.raises(ValueError, match='simclr'):
            pkg.SimCLRTrainer(make_cfg(pkg, 'R2P1D10T', mem, 32, 16, 8), DEV)
    with pytest.raises(NotImplementedError, match='one GPU'):
        pkg.SimCLRTrainer(simclr_cfg(pkg), DEV, ctx=pkg.parallel.DistCtx(force_active=True))


def test_lars_step_changes_every_adapted_tensor(pkg):
    tr = pkg.SimCLRTrainer(simclr_cfg(pkg, OPTIMIZER_NAME='LARS', BASE_LR=0.3), DEV, use_graph=False, seed=11)
    assert type(tr.optimizer).__name__ == 'HipLARS'
    before = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
    out = tr.train_step(clips(7, 1)[0])
    torch.cuda.synchronize()
    assert np.isfinite(float(out['loss']))
    adapted = [n for n, p in tr.model.named_parameters() if p.ndim > 1]
    assert len(adapted) > 20
    for n, p in tr.model.named_parameters():
        assert bool(torch.isfinite(p).all()), n
        if p.ndim > 1:
            assert not torch.equal(p.detach(), before[n]), n
    tr.close()
