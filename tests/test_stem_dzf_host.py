"""Host side of the fused stem backward (gca_bn_bwd_sums + gca_conv_wgrad_dzf), no kernel launched: the layout of the
constant array, the eligibility predicate gca_conv_dzf_ok, the argument checks of the new entries (every refusal comes before
a launch, so dummy pointers do), and the trainer dropping the queued split-K jobs of a backward pass that raised."""
import ctypes as C

import pytest
import torch


def _geom(H, N, Cin, D, Hh, W, K, k, s, p, f16=0, tile=14, splits=0):
    od, oh, ow = [(d + 2 * pp - kk) // ss + 1 for d, pp, kk, ss in zip((D, Hh, W), p, k, s)]
    g = H.ConvGeom(N, Cin, D, Hh, W, K, *k, *s, *p, od, oh, ow, 0)
    g.act_f16, g.tune_wgrad_tile, g.tune_wgrad_splits = f16, tile, splits
    return g


@pytest.fixture()
def bf16x6(pkg):
    H = pkg._hip
    default = H.lib.gca_get_conv_math()
    H.lib.gca_set_conv_math(2)
    yield H
    H.lib.gca_set_conv_math(default)


def test_constant_array_layout(pkg):
    """7 rows of stride 16 * ceil(C / 16) + 16: the padding of the scale / shift rows ops.bn_finalize hands the _xf entries."""
    elems = pkg._hip.lib.gca_bn_bwd_consts_elems
    for c, cp in ((1, 32), (16, 32), (17, 48), (64, 80), (110, 128), (128, 144)):
        assert elems(c) == 7 * cp, c
        assert cp == -(-c // 16) * 16 + 16
    assert elems(0) < 0 and elems(-3) < 0 and elems(2 ** 31) < 0


def test_dzf_ok_follows_the_stem_kernel(bf16x6):
    """gca_conv_dzf_ok is 1 exactly where the weight gradient runs on the stem kernel under the tune fields in force: the
    three stems of the flagship configs, not with another tile pinned, not on a geometry the stem kernel refuses (OW = 19 and
    OW = 17: not multiples of 8), not on other convs, not under fp32 MFMA."""
    H = bf16x6
    ok = lambda g: H.lib.gca_conv_dzf_ok(C.byref(g))
    out = (C.c_int32 * 4)()

    def kernel(g):
        assert H.lib.gca_conv_wgrad_cfg(C.byref(g), out) == 0
        return out[3] & 255

    stems = [(32, 3, 16, 112, 112, 110, (1, 7, 7), (1, 2, 2), (0, 3, 3), 0),            # R(2+1)D-18
             (32, 3, 16, 224, 224, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3), 0),             # S3D
             (16, 3, 32, 224, 224, 64, (7, 7, 7), (1, 2, 2), (3, 3, 3), 1),             # 3D-ResNet-50, fp16 storage
             (2, 3, 3, 34, 48, 110, (1, 7, 7), (1, 2, 2), (0, 3, 3), 0),                # the shapes of tests/test_gpu_stem_dzf.py
             (2, 3, 3, 34, 48, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3), 0),
             (1, 3, 4, 34, 48, 64, (7, 7, 7), (1, 2, 2), (3, 3, 3), 1),
             (2, 3, 4, 144, 144, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3), 0)]
    for *shape, f16 in stems:
        for splits in (0, 1, 64):
            g = _geom(H, *shape, f16=f16, splits=splits)
            assert kernel(g) == 14 and ok(g) == 1, (shape, splits)
            # same slabs as the plain launch: one workspace size, whichever entry runs
            plain = H.lib.gca_conv_wgrad_ws_bytes(C.byref(g))
            assert plain > 0
        for tile in (0, 1, 4, 8, 11, 13):
            g = _geom(H, *shape, f16=f16, tile=tile)
            assert kernel(g) != 14 and ok(g) == 0, (shape, tile)
    refused = [(2, 3, 3, 34, 38, 110, (1, 7, 7), (1, 2, 2), (0, 3, 3), 0),              # OW = 19
               (1, 3, 4, 34, 34, 64, (7, 7, 7), (1, 2, 2), (3, 3, 3), 1),               # OW = 17
               (2, 64, 4, 16, 16, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), 0),              # a temporal conv
               (2, 64, 4, 16, 16, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), 0)]              # a (1,3,3) conv
    for *shape, f16 in refused:
        g = _geom(H, *shape, f16=f16)
        assert kernel(g) != 14 and ok(g) == 0, shape
    bad = _geom(H, 2, 3, 3, 34, 48, 110, (1, 7, 7), (1, 2, 2), (0, 3, 3))
    bad.OW += 1
    assert ok(bad) == 0                                                                 # not a geometry at all
    H.lib.gca_set_conv_math(0)
    assert ok(_geom(H, *stems[0][:-1])) == 0                                            # fp32 MFMA: no stem kernel


def test_new_entries_refuse_before_launching(bf16x6):
    """GCA_EINVAL (-1) for a non-stem geometry, for a stem geometry with another tile pinned, for a ReLU mode that reads z, for
    missing or misaligned operands; nothing is launched (the operands are dummy addresses)."""
    H = bf16x6
    A = 1 << 20                                        # a 16-byte aligned dummy address
    splits = C.c_int32(0)
    stem = _geom(H, 2, 3, 3, 34, 48, 110, (1, 7, 7), (1, 2, 2), (0, 3, 3))

    def full(g, x=A, dz=A, y=A, consts=A, relu=2, dw=A, ws=A):
        return H.lib.gca_conv_wgrad_dzf(C.byref(g), x, dz, y, consts, relu, None, dw, 1, ws, None)

    def partial(g, x=A, dz=A, y=A, consts=A, relu=2, slabs=A, out=C.addressof(splits)):
        return H.lib.gca_conv_wgrad_dzf_partial(C.byref(g), x, dz, y, consts, relu, None, slabs, out, None)

    for call in (full, partial):
        assert call(_geom(H, 2, 3, 3, 34, 48, 110, (1, 7, 7), (1, 2, 2), (0, 3, 3), tile=8)) == -1      # tile 8 pinned
        assert call(_geom(H, 2, 3, 3, 34, 48, 110, (1, 7, 7), (1, 2, 2), (0, 3, 3), tile=0)) == -1      # heuristic: gather
        assert call(_geom(H, 2, 64, 4, 16, 16, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), tile=11)) == -1      # not a stem conv
        assert call(_geom(H, 2, 3, 3, 34, 38, 110, (1, 7, 7), (1, 2, 2), (0, 3, 3))) == -1               # OW = 19
        assert call(stem, relu=1) == -1 and call(stem, relu=3) == -1 and call(stem, relu=-1) == -1
        for miss in ('x', 'dz', 'y', 'consts'):
            assert call(stem, **{miss: None}) == -1, miss
        assert call(stem, dz=A + 8) == -1 and call(stem, y=A + 4) == -1 and call(stem, x=A + 2) == -1
    assert full(stem, dw=None) == -1 and full(stem, ws=None) == -1
    assert partial(stem, slabs=None) == -1 and partial(stem, out=None) == -1

    sums = lambda **kw: H.lib.gca_bn_bwd_sums(*[kw.get(k, d) for k, d in (
        ('dz', A), ('x', A), ('gamma', A), ('mean', A), ('invstd', A), ('relu', 2), ('N', 2), ('C', 110), ('SP', 1224),
        ('dgamma', A), ('dbeta', A), ('zs', 0), ('scale', A), ('shift', A), ('consts', A), ('ws', A), ('f16', 0), ('stream', None))])
    assert sums(relu=1) == -1 and sums(relu=3) == -1
    assert sums(scale=None) == -1 and sums(shift=None) == -1                            # mode 2 needs the forward's fold
    for miss in ('dz', 'x', 'mean', 'invstd', 'consts', 'ws'):
        assert sums(**{miss: None}) == -1, miss
    assert sums(N=0) == -1 and sums(C=0) == -1 and sums(SP=-1) == -1
    assert sums(zs=110 * 1224 - 1) == -1                                                # a batch stride inside a clip


def test_failed_backward_leaves_no_pending_reductions(pkg, monkeypatch):
    """A closure that raises after weight-gradient jobs were queued: _backward's `finally` empties the trainer's collector, so
    the next step neither folds stale slabs nor sees another job-table signature."""
    ops, trainer, tape = pkg.engine.ops, pkg.engine.trainer, pkg.engine.tape
    monkeypatch.setattr(trainer, 'DEFER_REDUCE', True)
    t = trainer._TrainerBase.__new__(trainer._TrainerBase)
    tp = tape.Tape(True)
    seen = []

    def queues_a_job():
        seen.append(ops.DEFER[0])
        ops.DEFER[0].pending.append((torch.zeros(4), torch.zeros(4), 4, 1, 1))

    def raises():
        raise ValueError('closure failed')
    tp.record(raises)                                  # (closures run in reverse: the job is queued first)
    tp.record(queues_a_job)
    with pytest.raises(ValueError, match='closure failed'):
        t._backward(tp, 0)
    assert seen == [t._deferred] and t._deferred.pending == [] and ops.DEFER[0] is None
    assert t._deferred.launches == 0
