"""CPU replay of the conv launch tuner (ConvPlan.search in engine/ops.py, the candidate lists of engine/tune.py) for every key
of profiles/tune_cache.json, against tests/golden/conv_tune_trace.npz.

The fixture was recorded ONCE, from the commit before the tuner moved into engine/tune.py, by driving that commit's
ConvPlan.tune() with the same replay() as below (its timer and its "is the stream capturing" query stubbed); it is never
regenerated from the code under test.  Everything the tuner does besides launching is host arithmetic plus host-only
library queries, so a fake, deterministic measurement fixes its complete behaviour: which configurations it offers to the
timer and in which order, when it re-packs the weights, what it pins, what it writes to the cache, and what each cache-hit
path does."""
import hashlib
import importlib.util
import json
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNE_INTS = tuple('tune_%s_%s' % (p, f) for p in ('fwd', 'dgrad') for f in ('bm', 'splits', 'tail', 'math', 'box')) + (
    'tune_wgrad_tile', 'tune_wgrad_splits', 'tune_wgrad_math')
GEOM_KEY_FIELDS = ('N', 'C', 'D', 'H', 'W', 'K', 'kd', 'kh', 'kw', 'sd', 'sh', 'sw', 'pd', 'ph', 'pw', 'x_batch_stride')
# (what the cache holds for the key before the run, whether the caller can re-pack the weights -- passes 0 and 1 only)
SCENARIOS = (('empty', True), ('empty', False), ('committed', True), ('committed', False), ('refused', True))
REFUSED_MATH = 9            # a tune math code the library refuses: the entry is stale and the key is measured again
NO_ENTRY = -1


def digest(ints):
    """First 8 bytes of the SHA-256 of a (nested) list of ints taken as little-endian int64, as a signed integer."""
    return int.from_bytes(hashlib.sha256(np.asarray(ints, dtype='<i8').tobytes()).digest()[:8], 'little', signed=True)


def fake_ms(key, ints):
    """The "time" of a configuration: 1 + u32(first four bytes, little-endian, of sha256(key:ints)) / 2**32."""
    h = hashlib.sha256(('%s:%s' % (key, ','.join(str(int(v)) for v in ints))).encode()).digest()
    return 1 + int.from_bytes(h[:4], 'little') / 2.0 ** 32


def parse_key(key):
    """'v15c:1:N,C,...' -> (arithmetic mode to set, fp16 storage, pass, the 16 geometry ints of the key)."""
    prefix, which, geom = key.split(':')
    mode = re.fullmatch(r'v\d+([bch]?)', prefix).group(1)
    return {'': 0, 'b': 1, 'c': 2, 'h': 2}[mode], mode == 'h', int(which), [int(v) for v in geom.split(',')]


def committed_cache():
    with open(os.path.join(ROOT, 'profiles', 'tune_cache.json')) as f:
        return sorted((k, tuple(v)) for k, v in json.load(f).items())


def drive(plan, which, key, measure, repack):
    assert plan.tune_key(which) == key
    plan.search(which, measure, repack)


def replay(ops, key, entry, scenario, drive=drive):
    """One tuner run on a fresh CPU plan of `key` under `scenario` -> (the record, the configurations offered to the timer
    with their times).  The caller has set the arithmetic mode of the key."""
    _, f16, which, (N, C, D, Hh, W, K, kd, kh, kw, sd, sh, sw, pd, ph, pw, xbs) = parse_key(key)
    seed, can_repack = scenario
    plan = ops.ConvPlan(N, C, D, Hh, W, K, (kd, kh, kw), (sd, sh, sw), (pd, ph, pw), torch.device('cpu'), xbs, act_f16=f16)
    plan.tuned = [False] * 3
    ops._TUNE_CACHE.clear()
    if seed == 'committed':
        ops._TUNE_CACHE[key] = entry
    elif seed == 'refused':
        ops._TUNE_CACHE[key] = entry[:-1] + (REFUSED_MATH,) if which == 2 else entry[:3] + (REFUSED_MATH,) + entry[4:]
    offered, repacks = [], []

    def measure():
        ints = [int(getattr(plan.g, f)) for f in TUNE_INTS]
        offered.append((fake_ms(key, ints), ints))
        return offered[-1][0]
    drive(plan, which, key, measure, (lambda: repacks.append(len(offered))) if can_repack and which < 2 else None)
    after = ops._TUNE_CACHE.get(key)
    after = [NO_ENTRY] * 6 if after is None else [len(after)] + list(after) + [0] * (5 - len(after))
    record = [digest(list(key.encode())), SCENARIOS.index(scenario), len(offered), digest([c for _, c in offered]), len(repacks),
              digest(repacks)] + [int(getattr(plan.g, f)) for f in TUNE_INTS] + [int(plan.tuned[which])] + after + [
              plan.parts, plan.fwd_ws, plan.dgrad_ws, plan.wgrad_ws]
    return record, offered


def bases_of(which, offered):
    """The launch codes of pass `which` of the two fastest single-launch configurations among `offered` (what the tuner
    builds its two-phase follow-up on), as two rows of five ints; NO_ENTRY rows where there are fewer, or for pass 2."""
    lo = 5 * which
    single = sorted((t, c[lo:lo + 5]) for t, c in offered if which < 2 and c[lo + 2] == 0)
    return [c for _, c in single[:2]] + [[NO_ENTRY] * 5] * (2 - len(single[:2]))


def test_tuner_replay_matches_the_recorded_trace(pkg):
    """Every key of profiles/tune_cache.json, each under every scenario of SCENARIOS (the refused entry included: it must
    fall through to measurement), on a fresh ConvPlan on the CPU with a fake timer: every recorded field is the same."""
    for knob in ('GCA_HALO', 'GCA_PW', 'GCA_STEM'):
        if os.environ.get(knob):
            pytest.skip('%s changes which kernels the library can run, hence what the tuner offers' % knob)
    ops, H = pkg.engine.ops, pkg._hip
    want = np.load(os.path.join(ROOT, 'tests', 'golden', 'conv_tune_trace.npz'))['trace']
    cache = committed_cache()
    assert len(want) == len(cache) * len(SCENARIOS)
    saved = (dict(ops._TUNE_CACHE), ops._TUNE_DIRTY[0], H.lib.gca_get_conv_math())
    bad, row, remeasured = [], 0, set()
    try:
        for key, entry in cache:
            assert H.lib.gca_set_conv_math(parse_key(key)[0]) == 0
            for scenario in SCENARIOS:
                got, offered = replay(ops, key, entry, scenario)
                if got != want[row].tolist():
                    bad.append((key, scenario, got, want[row].tolist()))
                if scenario[0] == 'refused' and offered:
                    remeasured.add(parse_key(key)[2])
                row += 1
    finally:
        ops._TUNE_CACHE.clear()
        ops._TUNE_CACHE.update(saved[0])
        ops._TUNE_DIRTY[0] = saved[1]
        H.lib.gca_set_conv_math(saved[2])
    assert not bad, (len(bad), bad[:3])
    assert remeasured == {0, 1, 2}


def test_candidate_lists_need_no_device_and_match_the_recorded_ones():
    """engine/tune.py alone (loaded from its file: no package import, no library, no torch device), on a plain namespace
    with the geometry fields: the round-one candidate list of every key, and the two-phase follow-up of the two codes the
    recorded run built it on, are the recorded lists."""
    spec = importlib.util.spec_from_file_location('gca_tune_alone', os.path.join(ROOT, 'video-graph-ssl_amd', 'engine', 'tune.py'))
    tune = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tune)
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'conv_tune_trace.npz'))
    cache = committed_cache()
    assert len(z['candidates']) == len(cache)
    bad = []
    for (key, _), want in zip(cache, z['candidates'].tolist()):
        math, f16, which, geom = parse_key(key)
        g = types.SimpleNamespace(act_f16=int(f16), **dict(zip(GEOM_KEY_FIELDS, geom)))
        g.OD, g.OH, g.OW = [(n + 2 * p - k) // s + 1 for n, p, k, s in zip(geom[2:5], geom[12:15], geom[6:9], geom[9:12])]
        first = tune.candidates(which, g, math)
        bases = [want[5 + 5 * i:10 + 5 * i] for i in (0, 1)]
        second = [c for b in bases if b[0] != NO_ENTRY for c in tune.two_phase(which, g, tune.ConvCode(*b))]
        got = [digest(list(key.encode())), len(first), digest(first), len(second), digest(second)] + bases[0] + bases[1]
        if got != want:
            bad.append((key, got, want))
    assert not bad, (len(bad), bad[:3])
