"""CPU checks of the Adam / AdamW feature: the fp64 specification (tests/adam_ref.py) against torch's own optimizers, the
arguments gca_adam_step refuses before any launch, the optimizer factory's refusal and the cross-format state errors."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as ref                   # noqa: E402

SIZES = (1, 255, 700)
GROUPS = ((1e-3, 0.0), (2e-3, 5e-4), (1e-3, 1e-2))         # (lr, weight_decay) per tensor


@pytest.mark.parametrize('decoupled', [False, True])
def test_specification_equals_torch_in_fp64(decoupled):
    """Five steps of torch.optim.Adam / AdamW in fp64 over three tensors with their own (lr, weight_decay) against the
    specification on the flat arena: 1e-12 relative (both sides fp64; only the order of a few operations differs)."""
    gen = torch.Generator().manual_seed(11)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen, dtype=torch.float64)) for n in SIZES]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([{'params': [p], 'lr': lr, 'weight_decay': wd} for p, (lr, wd) in zip(params, GROUPS)])
    offs, total = ref.arena_layout(SIZES)
    lr, wd = ref.expand_chunks(SIZES, [g[0] for g in GROUPS]), ref.expand_chunks(SIZES, [g[1] for g in GROUPS])
    p = np.zeros(total)
    for o, n, prm in zip(offs, SIZES, params):
        p[o:o + n] = prm.detach().numpy()
    m, v = np.zeros(total), np.zeros(total)
    for t in range(1, 6):
        g = np.zeros(total)
        for o, n, prm in zip(offs, SIZES, params):
            prm.grad = torch.randn(n, generator=gen, dtype=torch.float64)
            g[o:o + n] = prm.grad.numpy()
        opt.step()
        p, m, v = ref.adam_step(p, g, m, v, t, lr, wd, decoupled=decoupled)
        for i, (o, n, prm) in enumerate(zip(offs, SIZES, params)):
            st = opt.state[prm]
            for name, got, want in (('p', p, prm.detach()), ('exp_avg', m, st['exp_avg']), ('exp_avg_sq', v, st['exp_avg_sq'])):
                want = want.numpy()
                err = np.abs(got[o:o + n] - want).max() / np.abs(want).max()
                assert err < 1e-12, (t, i, name, err)
        pad = ref.padding_mask(SIZES)
        assert not p[pad].any() and not m[pad].any() and not v[pad].any()


def test_skip_and_coef_of_the_specification():
    p, g, m, v = (np.array([0.5, -2.0]), np.array([1.0, 3.0]), np.array([0.1, 0.2]), np.array([0.3, 0.4]))
    q = ref.adam_step(p, g, m, v, 4, 1e-3, 1e-2, skip=True)
    assert all(np.array_equal(a, b) for a, b in zip(q, (p, m, v)))
    a = ref.adam_step(p, g, m, v, 4, 1e-3, 0.0, coef=0.5)
    b = ref.adam_step(p, 0.5 * g, m, v, 4, 1e-3, 0.0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_adam_step_refuses_bad_arguments_before_launching(pkg):
    """Null operands, n <= 0 and n % 256 != 0 are GCA_EINVAL (-1) before anything is launched: the operands are dummy pointers,
    so a launch attempt would report GCA_ELAUNCH (-2) or fault."""
    lib = pkg._hip.lib
    d = 1 << 20
    good = [d, d, d, d, 1280, d, d, 0.9, 0.999, 1e-8, 0, None, d, None]
    for i in (0, 1, 2, 3, 5, 6, 12):                       # p, grad, exp_avg, exp_avg_sq, chunk_lr, chunk_wd, state
        args = list(good)
        args[i] = None
        assert lib.gca_adam_step(*args) == -1, i
    for n in (0, -256, 1, 255, 1279, 1284):
        args = list(good)
        args[4] = n
        assert lib.gca_adam_step(*args) == -1, n
    for i, bad in ((7, 1.0), (7, -0.1), (8, 1.0), (9, 0.0), (9, float('nan'))):     # 0 <= beta < 1, eps > 0
        args = list(good)
        args[i] = bad
        assert lib.gca_adam_step(*args) == -1, (i, bad)
    assert lib.gca_adam_advance(None, None, None) == -1


def _cfg(pkg, name):
    cfg = pkg.get_defaults()
    cfg.SOLVER.OPTIMIZER_NAME = name
    return cfg


def test_factory_names(pkg):
    model = torch.nn.Linear(3, 2)
    with pytest.raises(NotImplementedError, match='SGD, Adam, AdamW'):
        pkg.make_optimizer(_cfg(pkg, 'RMSprop'), model)
    S = pkg.lib.solver
    cfg = _cfg(pkg, 'SGD')
    for name, cls, dec in (('SGD', S.HipSGD, None), ('Adam', S.HipAdam, False), ('AdamW', S.HipAdam, True)):
        opt = pkg.make_optimizer(_cfg(pkg, name), torch.nn.Linear(3, 2))
        assert type(opt) is cls and [g['name'] for g in opt.param_groups] == ['weight', 'bias']
        w, b = opt.param_groups
        assert (w['lr'], w['weight_decay']) == (cfg.SOLVER.BASE_LR, cfg.SOLVER.WEIGHT_DECAY) and w['initial_lr'] == w['lr']
        assert (b['lr'], b['weight_decay']) == (cfg.SOLVER.BASE_LR * cfg.SOLVER.BIAS_LR_FACTOR, cfg.SOLVER.WEIGHT_DECAY_BIAS)
        if dec is not None:
            assert opt.decoupled is dec and w['betas'] == (0.9, 0.999) and w['eps'] == 1e-8 and w['amsgrad'] is False
            assert 'momentum' not in w


def test_cross_format_state_is_refused(pkg):
    """An SGD-format state handed to HipAdam, and an Adam-format one handed to HipSGD, raise ValueError naming both formats
    (the state buffers live on the host here: nothing is launched by construction, state_dict or load_state_dict)."""
    sgd = pkg.make_optimizer(_cfg(pkg, 'SGD'), torch.nn.Linear(3, 2))
    adam = pkg.make_optimizer(_cfg(pkg, 'Adam'), torch.nn.Linear(3, 2))
    for opt, sd in ((adam, sgd.state_dict()), (sgd, adam.state_dict()),
                    (adam, {'momentum_buffer': torch.zeros(512), 'param_groups': sgd.state_dict()['param_groups']})):
        with pytest.raises(ValueError, match='momentum_buffer.*exp_avg'):
            opt.load_state_dict(sd)
    # each still loads its own, and torch's
    sgd.load_state_dict(sgd.state_dict())
    sd = adam.state_dict()
    assert all(float(st['step']) == 0.0 and st['step'].dtype is torch.float32 for st in sd['state'].values())
    adam.load_state_dict(sd)
    for g in sd['param_groups']:
        g['amsgrad'] = True
    with pytest.raises(NotImplementedError):
        adam.load_state_dict(sd)
    sd = adam.state_dict()
    sd['param_groups'][1]['betas'] = (0.8, 0.999)
    with pytest.raises(NotImplementedError):
        adam.load_state_dict(sd)
