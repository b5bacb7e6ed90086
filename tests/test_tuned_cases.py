"""CPU checks of tests/tuned_cases.py, the cases tests/test_gpu_tuned.py runs: every entry of profiles/tune_cache.json belongs
to exactly one case; a case that runs as cached adopts its codes from the cache the way the product does; a case that runs
on a shrunken geometry resolves, under its pinned codes, to the launch its key resolves to (plans on torch.device('cpu'):
host logic only); and the operands of every case meet the preconditions of the bit-exact comparison, as tests/test_exact.py
asserts them for tests/test_gpu_exact.py.

Cases whose LDS-halo boxes cannot end ragged on every axis (RELAXED_BOXES): their streaming temporal weight gradient wants
H * W % 16 == 0 while boxes of 2 rows x 8 columns want an odd H and W % 8 != 0; they keep two boxes per axis, ragged along W.
No case had to stay at its key's size for want of a smaller geometry (FORCED_FULL is empty).
"""
import os

import pytest
import torch

import exact
import tuned_cases as tc
from test_tuner import committed_cache

CPU = torch.device('cpu')
ENTRIES = {e.id: e for e in tc.entries()}
RELAXED_BOXES = {'v15c-n4-c192-8x56x56-k192-311-s111-p100', 'v15b-n32-c110-16x56x56-k64-711-s111-p300',
                 'v15c-n32-c110-16x56x56-k64-711-s111-p300'}
FORCED_FULL = set()


@pytest.fixture
def mode(pkg):
    """The library's arithmetic mode restored after a test that sets it per case."""
    H = pkg._hip
    prev = H.lib.gca_get_conv_math()
    yield
    H.lib.gca_set_conv_math(prev)


def test_every_cache_entry_belongs_to_exactly_one_case(pkg, mode):
    cache = committed_cache()
    assert len(cache) == 487 and len(ENTRIES) == 165
    covered = []
    for e in ENTRIES.values():
        for which, code in e.codes:
            covered.append(('%s:%d:%s' % (e.prefix, which, ','.join(str(v) for v in e.geom)), code))
    assert sorted(covered) == cache                                  # every key once, with its own entry
    runs = tc.runs()
    as_cached = [r for r in runs if not r.shrunken]
    assert all(tc.runs_as_cached(r.entry.geom) == (not r.shrunken) for r in runs)
    assert {r.entry.id for r in runs if r.forced_full} == FORCED_FULL
    assert {r.entry.id for r in runs if r.relaxed_boxes} == RELAXED_BOXES
    print('TUNED cases: %d = %d as cached + %d shrunken; %d weight-gradient split counts clamped; %d with relaxed boxes; '
          'largest forward %.2f G multiply-adds' % (len(runs), len(as_cached), len(runs) - len(as_cached),
                                                     sum(r.wgrad_clamped for r in runs), len(RELAXED_BOXES),
                                                     max(tc.macs(r.geom) for r in runs) / 2.0 ** 30))
    assert len(as_cached) + sum(r.shrunken for r in runs) == 165
    # nothing runs at a workload's size unless it is small: the budgets, or at most twice the multiply-adds where no
    # geometry inside them keeps two full column tiles and a ragged one
    assert max(tc.macs(r.geom) for r in runs) <= 2 * tc.MAC_BUDGET


@pytest.mark.parametrize('cid', sorted(ENTRIES))
def test_case_launches_what_its_cache_entries_launch(pkg, mode, cid):
    ops = pkg.engine.ops
    e = ENTRIES[cid]
    run = tc.build(e)
    tc.set_mode(e)
    codes = tc.codes_of(e)
    if not run.shrunken:
        # as cached: the key's geometry, and the tuner adopts the entry (no measurement: the timer must not be asked)
        assert run.geom == e.geom and run.codes == codes
        saved = (dict(ops._TUNE_CACHE), ops._TUNE_DIRTY[0])
        try:
            ops._TUNE_CACHE.clear()
            ops.load_tune_cache(os.path.join(tc_root(), 'profiles', 'tune_cache.json'))
            plan = tc.make_plan(e.geom, e.f16, CPU)
            plan.tuned = [False] * 3
            for which, code in codes.items():
                assert plan.tune_key(which) == '%s:%d:%s' % (e.prefix, which, ','.join(str(v) for v in e.geom))
                plan.search(which, lambda: pytest.fail('measured instead of adopting the entry'), lambda: None)
                assert plan.tuned[which]
                got = [getattr(plan.g, 'tune_%s_%s' % (ops.tune.PASSES[which], f)) for f in code._fields]
                assert got == list(code), (which, got, code)
        finally:
            ops._TUNE_CACHE.clear()
            ops._TUNE_CACHE.update(saved[0])
            ops._TUNE_DIRTY[0] = saved[1]
        return
    g0, g = e.geom, run.geom
    # what stays: channels, kernel, stride, padding, storage, "x is a channel slice of a wider batch"
    assert g[1] == g0[1] and g[5:15] == g0[5:15] and (g[15] != 0) == (g0[15] != 0)
    assert g[15] in (0, 2 * g[1] * g[2] * g[3] * g[4])
    assert all(a <= b for a, b in zip((g[0], g[2], g[3], g[4]), (g0[0], g0[2], g0[3], g0[4]))) and tc.macs(g) < tc.macs(g0)
    full, small = tc.make_plan(g0, e.f16, CPU, codes), tc.make_plan(g, e.f16, CPU, run.codes)
    for which, code in codes.items():
        pinned = run.codes[which]
        assert small.kernel(which) == full.kernel(which), which
        cf, cs = full.cfg(which), small.cfg(which)
        assert cs[:2] == cf[:2], (which, cs, cf)                     # tile rows and columns
        assert cs[3] == cf[3], (which, cs, cf)                       # classes, mask kind, float4 flags, arithmetic, kernel bits
        if which == 2:
            assert pinned == code
            if run.wgrad_clamped:
                assert cs[2] < cf[2] and (cs[2] >= 2 or cf[2] < 2), (cs, cf)
            else:
                assert cs[2] in (cf[2], code.splits), (cs, cf, code)
            continue
        assert cs[2] == cf[2], (which, cs, cf)                       # splits
        assert pinned._replace(tail=0) == code._replace(tail=0)      # rows, splits, arithmetic pin, box: as cached
        tf, ts = tc.tail_in_force(full, g0, which, code), tc.tail_in_force(small, g, which, pinned)
        assert ts[0] == tf[0] == (pinned.tail & 255) * 32 * bool(tf[0])
        if tf[0]:
            tiles = -(-tc.first_class_positions(g, which) // 128)
            assert ts[1] == tiles // 2 and 0 < ts[1] < tiles
        if full.kernel(which) in ('gather', 'pw'):                   # two full column tiles and a ragged one
            cols = g[2] * g[3] * g[4] if full.kernel(which) == 'pw' else tc.first_class_positions(g, which)
            assert cols > 2 * cf[1] and cols % cf[1] != 0, (which, cols, cf)
    desc = lambda plan, geom, cc: tc.describe(plan, geom, cc)
    assert tc.violations(g0, desc(full, g0, codes), g, desc(small, g, run.codes), codes, run.codes,
                         wgrad_exact=not run.wgrad_clamped, ragged_boxes=not run.relaxed_boxes) == []


def tc_root():
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('cid', sorted(ENTRIES))
def test_case_operands_meet_the_preconditions(pkg, mode, cid):
    """Dyadic operands: every sum the GPU test asserts bit for bit stays inside fp32's integer range in any order (the weight
    gradient also when accumulated twice), the operands have at most 6 significant bits, and an fp16 case really holds
    outputs fp16 must round.  Float operands of an fp16 case are fp16 numbers."""
    e = ENTRIES[cid]
    run = tc.build(e)
    main, stats = tc.pick_sets(run)
    c = tc.dyadic_case(run.geom, main)
    b = c['budgets']
    print('TUNED %-52s %-6s y %.2e dx %.2e dw %.2e sum|y| %.2e sum y^2 %.2e%s' % (
        cid, main, b['y'], b['dx'], b['dw'], b['sy'], b['sq'], '' if stats == main else ' (statistics on %s)' % stats))
    assert b['y'] < 1 and b['dx'] < 1 and 2 * b['dw'] < 1
    if stats == main:
        assert b['sy'] < 1
    else:
        b2 = tc.dyadic_case(run.geom, stats)['budgets']
        assert b2['y'] < 1 and b2['sy'] < 1
    for t in (c['x'], c['w'], c['dy']):
        assert torch.equal(t.bfloat16().double(), t) and torch.equal(t.half().double(), t)
    if e.f16:
        y, dx = c['ref']['y'], c['ref']['dx']
        assert exact.n_inexact(y) > 0
        assert bool(torch.isfinite(exact.to_f16(y)).all()) and bool(torch.isfinite(exact.to_f16(dx)).all())
        for t in tc.float_operands(run.geom, True):
            assert torch.equal(t.half().double(), t)


def test_tap_reference_is_atens_convolution():
    """tuned_cases.conv_sums (one matrix product per tap plane) against exact.conv_ref (ATen in double) on a padded, strided case:
    on dyadic operands both are exact, hence equal bit for bit."""
    x, w = exact.grid((2, 3, 5, 7, 6), 8, 0.25, 1), exact.grid((4, 3, 3, 2, 3), 8, 0.125, 2)
    s, p = (2, 1, 2), (1, 0, 2)
    dy = exact.grid(torch.nn.functional.conv3d(x, w, None, s, p).shape, 8, 0.25, 3)
    got, want = tc.conv_sums(x, w, s, p, dy), exact.conv_ref(x, w, None, s, p, dy)
    got_abs, want_abs = tc.conv_ref_abs(x, w, s, p, dy)[1], exact.conv_abs(x, w, None, s, p, dy)
    for k in ('y', 'sy', 'sq', 'dx', 'dw'):
        assert torch.equal(got[k], want[k]), k
        assert torch.equal(got_abs[k], want_abs[k]), k


def test_a_corrupted_code_does_not_pass_as_the_cached_launch(pkg, mode):
    """The comparison above is not vacuous: a box with d and h swapped, one more split, 64 rows turned into 96 and a
    streaming weight-gradient tile turned into a gather tile are each reported."""
    by_kernel = {}
    for e in ENTRIES.values():
        run = tc.build(e)
        if run.shrunken:
            by_kernel.setdefault((dict(e.codes)[0][0] & 2048 != 0, dict(e.codes)[2][0] > 10), run)
    run = by_kernel[(True, True)]
    e = run.entry
    tc.set_mode(e)
    codes = tc.codes_of(e)
    full = tc.describe(tc.make_plan(e.geom, e.f16, CPU, codes), e.geom, codes)

    def reported(bad_codes):
        small = tc.describe(tc.make_plan(run.geom, e.f16, CPU, bad_codes), run.geom, bad_codes)
        return tc.violations(e.geom, full, run.geom, small, codes, bad_codes, not run.wgrad_clamped, not run.relaxed_boxes)
    assert reported(run.codes) == []
    d, h, w = tc.box_of(codes[0])
    assert d != h
    swap = lambda which, code: {**run.codes, which: code}
    assert reported(swap(0, codes[0]._replace(box=h | d << 8 | w << 16)))
    assert reported(swap(0, codes[0]._replace(splits=codes[0].splits + 1)))
    assert reported(swap(0, codes[0]._replace(bm=codes[0].bm + 32)))
    assert reported(swap(2, codes[2]._replace(tile=1)))
