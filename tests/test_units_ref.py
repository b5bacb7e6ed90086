"""CPU tests of tests/units_ref.py: every precondition the GPU cases of tests/test_gpu_units.py rest on, asserted from the fp64
reference alone, and every route selection the host side of the library can decide without a device."""
import pytest
import torch
import torch.nn.functional as F

import units_ref as U


def _cases():
    return [('single', a) for a in U.SINGLES] + [('chain', (n,)) for n in U.CHAINS]


def _case(kind, args):
    return U.single(*args) if kind == 'single' else U.chain(*args)


@pytest.mark.parametrize('kind,args', _cases())
def test_first_units_are_exact_and_decided(kind, args):
    """Dyadic budget below 1 (the conv output is the fp64 answer in any summation order); every pre-activation of a first unit
    with a ReLU at least 64 fp32 roundings of its own terms away from zero, for EVERY element; the mask is mixed."""
    c = _case(kind, args)
    for name, share in c.budgets.items():
        assert share < 1, (name, share)
    for name in c.first:
        worst, active = U.first_unit_margin(c.units[name])
        print('%s %s unit %s: margin %.2f x (64 roundings), active %.3f, %d elements' % (kind, args, name, worst, active, c.units[name]['p'].numel()))
        assert worst >= 1.0, (name, worst)
        assert 0.2 < active < 0.8, (name, active)
    for name, u in c.units.items():
        if u['relu']:
            assert 0.2 < float((u['p'] > 0).double().mean()) < 0.8, name
        assert float(u['scale'].detach().min()) > 0       # p is increasing in y: pool winners follow y


@pytest.mark.parametrize('name', U.CHAINS)
@pytest.mark.parametrize('bar', sorted(set(U.BARS.values())))
def test_seed_caps(name, bar):
    """At most 2 % of any seed gradient is zeroed, at either per-kernel bar; a first-unit output loses nothing."""
    c = U.chain(name)
    for out, (g, zeroed) in c.seeds(bar).items():
        print('%s %s bar %.0e: %.3f %% of the seed zeroed' % (name, out, bar, 100 * zeroed))
        assert zeroed <= U.SEED_CAP, (out, zeroed)
        assert c.outs[out][1] is not None or zeroed == 0.0
        assert float(g.abs().max()) > 0


def test_fp16_chain_preconditions():
    """R10: y_A is an fp16 number element for element (A's decisions do not depend on the storage type); the stored forward
    stays within the fp16-output bar of the unrounded one; the seed margin zeroes at most 2 %; the seed is made of fp16 numbers;
    and storage rounding really moves the gradients (the two references differ by more than the fp32-output bar somewhere --
    which is why the device is held to the one that rounds where the engine stores)."""
    import exact
    r, c = U.r3_f16(), U.chain('r3')
    yA = c.units['A']['y'].detach()
    assert exact.n_inexact(yA) == 0 and float(yA.abs().max()) < 65504
    assert torch.equal(r['A']['y'].detach(), yA)
    for tag in 'AB':
        for name in ('y', 'z'):
            got, want = r[tag][name].detach(), c.units[tag][name].detach()
            assert torch.equal(got, got.half().double())
            assert float((got - want).abs().max() / want.abs().max()) < U.F16_BARS[0]
    print('fp16 chain: %.3f %% of the seed zeroed' % (100 * r['zeroed']))
    assert 0 < r['zeroed'] <= U.SEED_CAP
    assert torch.equal(r['seed'], r['seed'].half().double())
    assert 0.2 < float((r['B']['p'] > 0).double().mean()) < 0.8
    assert set(r['grads']) == set(r['plain']) == {'wA', 'gammaA', 'betaA', 'wB', 'gammaB', 'betaB'}
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    gaps = {n: rel(r['grads'][n], r['plain'][n]) for n in r['grads']}
    print('fp16 chain: stored vs unrounded reference', {n: '%.2e' % v for n, v in gaps.items()})
    assert max(gaps.values()) > U.F16_BARS[1] and max(gaps.values()) < 4 * U.F16_BARS[0]


def test_keep_masks_mark_exactly_the_undecided():
    """keep_relu / keep_pool on a hand-made tensor: the margin is 16 * bar * max |p|; a window is kept only with a clear positive
    winner or with every value clearly negative."""
    p = torch.tensor([[-4.0, 0.5, -0.5, 3.0, 2.0, -3.0, -1.0, 1.0]], dtype=U.F64).view(1, 1, 1, 1, 8)
    bar = 1.0 / 64                    # m = 16 * bar * 4 = 1
    assert U.keep_relu(p, bar).flatten().tolist() == [1, 0, 0, 1, 1, 1, 1, 1]
    pool = ((1, 1, 2), (1, 1, 2), (0, 0, 0))
    # windows (-4, .5): winner below m; (-.5, 3): clear; (2, -3): clear; (-1, 1): winner == m, gap 2: kept
    assert U.keep_pool(p, pool, bar).flatten().tolist() == [0, 1, 1, 1]
    q = torch.tensor([[3.0, 2.5, -2.0, -1.0, -0.5, -3.0]], dtype=U.F64).view(1, 1, 1, 1, 6)
    # (3, 2.5): the runner-up is closer than m = 0.75; (-2, -1): all clearly negative; (-.5, -3): a value within m of zero
    assert U.keep_pool(q, pool, bar).flatten().tolist() == [0, 1, 0]


def test_unit_reference_is_batch_norm():
    """unit() against torch's own batch_norm in double: output, and the running statistics after one step."""
    c = U.single('k133', True, True)
    u, lv = c.units['A'], c.leaves
    rm, rv = torch.zeros(16, dtype=U.F64), torch.ones(16, dtype=U.F64)
    want = torch.relu(F.batch_norm(u['y'].detach(), rm, rv, lv['gammaA'].detach(), lv['betaA'].detach(), True, U.MOMENTUM, U.EPS) + lv['res'].detach())
    assert float((want - u['z'].detach()).abs().max()) < 1e-12
    assert float((rm - u['running_mean']).abs().max()) < 1e-13 and float((rv - u['running_var']).abs().max()) < 1e-13
    g = c.grads(1e-5)
    assert set(g) == {'x', 'wA', 'gammaA', 'betaA', 'res'} and all(bool(torch.isfinite(t).all()) for t in g.values())


def test_z_interval_is_far_below_the_forward_bar():
    """The per-element interval is derived from operation counts; it must stay a tighter statement than the 1e-5 norm-wise bar."""
    for kn in U.KERNELS:
        u = U.single(kn, True, False).units['A']
        assert float(U.z_interval(u).max() / u['z'].detach().abs().max()) < 1e-5


# ----------------------------------------------------------------------------- host-decidable route selections
@pytest.fixture()
def host(pkg):
    ops = pkg.engine.ops
    default = pkg._hip.lib.gca_get_conv_math()
    yield ops
    pkg._hip.lib.gca_set_conv_math(default)


def resolve(ops, name, mode):
    """The plan of ROUTES[name] under `mode` with its pins, on the host -> (fwd kernel, fwd splits, fwd_ws > 0, wgrad kernel, xf, dzf)."""
    shape, K, (k, s, p), pins, _ = U.ROUTES[name]
    ops.H.lib.gca_set_conv_math(ops.CONV_MATH[mode])
    plan = ops.ConvPlan(*shape, K, k, s, p, torch.device('cpu'))
    plan.tuned = [True, True, True]
    for f, v in pins.items():
        setattr(plan.g, 'tune_' + f, v)
    plan.refresh()
    return (plan.kernel(0), plan.cfg(0)[2], plan.fwd_ws > 0, plan.kernel(2), ops.conv_xf_ok(plan), ops.conv_dzf_ok(plan))


@pytest.mark.parametrize('mode', U.MODES)
@pytest.mark.parametrize('name', sorted(U.ROUTES))
def test_pinned_launch_codes_resolve_to_the_route(host, name, mode):
    assert resolve(host, name, mode) == U.ROUTES[name][4][mode], (name, mode)


def test_unpinned_small_shapes_would_split(host):
    """Why R1 pins one split: under the heuristic launch shapes the R1 / R6 geometries split the reduction with a workspace,
    which is the fused small-BatchNorm route (R2), not the eager one."""
    for name in ('r1_k333', 'r1_k133', 'r6_a'):
        shape, K, (k, s, p), _, _ = U.ROUTES[name]
        plan = host.ConvPlan(*shape, K, k, s, p, torch.device('cpu'))
        assert plan.cfg(0)[2] > 1 and plan.fwd_ws > 0, name


def test_lazy_threshold_of_the_cases():
    """N * SP of every producer the cases call lazy exceeds layers.BN_SMALL_ELEMS, and of every eager one does not."""
    n_sp = lambda sh: sh[0] * sh[2] * sh[3] * sh[4]
    assert n_sp(U.R3_X) == 33280 and n_sp(U.R4_X) == 34816 and n_sp((2, 16, 4, 72, 72)) == 41472
    assert n_sp(U.R1_X) == n_sp(U.R6_X) == 1248
    assert min(n_sp(U.R3_X), n_sp(U.R4_X)) > U.BN_SMALL_ELEMS >= n_sp(U.R1_X)


def test_bn_small_elems_matches_the_engine(pkg):
    assert pkg.engine.layers.BN_SMALL_ELEMS == U.BN_SMALL_ELEMS and pkg.engine.tune.TUNE_HALO == U.HALO
