"""A strided dgrad as ONE launch over all of its stride-residue classes (gca_conv_dgrad_ws, conv_igemm_classes_kernel) against
one launch per class: the same bits under pinned launch codes, and both within the dgrad bar (1e-5 of the output's max) of an
fp64 torch reference on the CPU.  The shapes make the classes differ in tap count and column count and put class boundaries
inside the grid; splits = 3 puts the classes' slabs side by side and finishes them in one launch."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0')
VEC = 1024          # engine/tune.py TUNE_VEC: the 256-column float4 variant (convs that are pointwise in space)
TOL = 1e-5          # the per-op bar of the dgrad tests in test_gpu_ops.py (f32 and bf16x6)

# name -> (x shape, K, kernel, stride, pad, (classes, classes with taps, the float4 variant can run them))
CASES = {
    'four_classes_1_2_2_4_taps': ((2, 24, 5, 9, 11), 40, (1, 3, 3), (1, 2, 2), (0, 1, 1), (4, 4, False)),
    'two_classes_temporal': ((3, 20, 7, 6, 6), 33, (3, 1, 1), (2, 1, 1), (1, 0, 0), (2, 2, True)),
    'eight_classes': ((2, 16, 5, 7, 9), 24, (3, 3, 3), (2, 2, 2), (1, 1, 1), (8, 8, False)),
    'seven_empty_classes': ((2, 16, 4, 6, 6), 32, (1, 1, 1), (2, 2, 2), (0, 0, 0), (8, 1, False)),   # (strided in space: no float4 rows)
}
_REF = {}


def reference(name):
    """(w, dy, fp64 dx of the CPU reference, the tensor an accumulating dgrad adds into) of a case, computed once."""
    if name not in _REF:
        shape, K, k, s, p, _ = CASES[name]
        gen = torch.Generator().manual_seed(1234 + len(name))
        x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
        w = torch.randn((K, shape[1]) + k, generator=gen) * 0.1
        y = F.conv3d(x, w.double(), None, s, p)
        dy = torch.randn(y.shape, generator=gen)
        y.backward(dy.double())
        _REF[name] = (w, dy, x.grad.detach(), torch.randn(shape, generator=gen))
    return _REF[name]


def codes(k):
    out = [(bm, sp) for bm in (32, 64) for sp in (1, 3)]
    if k[1] == 1 and k[2] == 1:
        out += [(bm | VEC, sp) for bm in (32, 64) for sp in (1, 3)]
    return out


@pytest.fixture(scope='module')
def ops(pkg):
    return pkg.engine.ops


@pytest.fixture(params=['bf16x6', 'f32'])
def math(request, ops):
    default = ops.get_conv_math()
    ops.set_conv_math(request.param)
    yield request.param
    ops.set_conv_math(default)


def pinned_plan(ops, name, bm, sp):
    shape, K, k, s, p, _ = CASES[name]
    plan = ops.ConvPlan(*shape, K, k, s, p, DEV)
    plan.tuned = [True, True, True]
    plan.g.tune_dgrad_bm, plan.g.tune_dgrad_splits = bm, sp
    plan.refresh()
    return plan


def dgrad(ops, plan, dy, wp, base, merge, ws_bytes=None):
    """conv_dgrad under the given merge setting; base: None, or the tensor the pass accumulates into."""
    was = ops.set_dgrad_merge(merge)
    try:
        if base is None:
            dx = torch.full(plan.in_shape, float('nan'), device=DEV)      # every element must be written
        else:
            dx = base.to(DEV).clone()
        ops._conv_dgrad_launch(plan, dy, wp, dx, base is not None, ws_bytes)
        torch.cuda.synchronize()
        return dx
    finally:
        ops.set_dgrad_merge(was)


@pytest.mark.gpu
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('name', list(CASES))
def test_merged_launch_has_the_bits_of_the_per_class_launches(pkg, ops, math, name, accumulate):
    H = pkg._hip
    shape, K, k, s, p, (nall, nclasses, vec_ok) = CASES[name]
    w, dy, ref, base = reference(name)
    want = ref + base.double() if accumulate else ref
    dyd, wd = dy.to(DEV), w.to(DEV)
    merged_runs = 0
    for bm, sp in codes(k):
        plan = pinned_plan(ops, name, bm, sp)
        cfg = plan.cfg(1)
        assert cfg[0] == bm & 1023 and cfg[1] == (256 if bm & VEC and vec_ok else 128) and cfg[3] & 255 == nall, cfg
        wp = ops.conv_pack(plan, 1, wd)
        room = max(plan.dgrad_ws, plan.dgrad_ws_merged)
        assert plan.dgrad_ws_merged >= plan.dgrad_ws
        takes_merged = bool(H.lib.gca_conv_dgrad_merged(plan.gp, room))
        assert takes_merged == (nclasses > 1), (name, bm, sp)          # a single class with taps has nothing to merge
        merged_runs += takes_merged
        on = dgrad(ops, plan, dyd, wp, base if accumulate else None, True)
        off = dgrad(ops, plan, dyd, wp, base if accumulate else None, False)
        assert torch.equal(on, off), (name, bm, sp, float((on - off).abs().max()))
        for tag, dx in (('merged', on), ('per class', off)):
            err = rel_err(dx, want)
            print('%s %s bm=%d splits=%d accumulate=%d %s: rel err %.3e' % (name, math, bm, sp, accumulate, tag, err))
            assert err < TOL, (name, bm, sp, tag, err)
    assert merged_runs == (len(codes(k)) if nclasses > 1 else 0)


@pytest.mark.gpu
def test_work_space_of_one_class_falls_back_to_per_class_launches(pkg, ops):
    """Handed only gca_conv_dgrad_ws_bytes (the maximum over classes, what the un-sized entry assumes), the slabs of the
    classes cannot exist side by side: the library launches class by class, with the same bits."""
    H = pkg._hip
    name = 'four_classes_1_2_2_4_taps'
    w, dy, ref, _ = reference(name)
    plan = pinned_plan(ops, name, 32, 3)
    assert plan.cfg(1)[2] == 3 and 0 < plan.dgrad_ws < plan.dgrad_ws_merged
    assert H.lib.gca_conv_dgrad_merged(plan.gp, plan.dgrad_ws_merged) == 1
    assert H.lib.gca_conv_dgrad_merged(plan.gp, plan.dgrad_ws) == 0
    dyd, wp = dy.to(DEV), ops.conv_pack(plan, 1, w.to(DEV))
    full = dgrad(ops, plan, dyd, wp, None, True)
    small = dgrad(ops, plan, dyd, wp, None, True, ws_bytes=plan.dgrad_ws)
    off = dgrad(ops, plan, dyd, wp, None, False)
    # the un-sized entry point: sized by the caller with gca_conv_dgrad_ws_bytes
    old = torch.full(plan.in_shape, float('nan'), device=DEV)
    ws = ops.WS.get(plan.dgrad_ws, DEV)
    H.call('gca_conv_dgrad', plan.gp, dyd.data_ptr(), wp.data_ptr(), plan.table(1).data_ptr(), old.data_ptr(), 0, ws.data_ptr(),
           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(full, small) and torch.equal(full, off) and torch.equal(full, old)
    assert rel_err(small, ref) < TOL


def test_class_block_fits_the_size_the_header_states(pkg):
    """CPU only: the by-value argument block of the merged launch is within GCA_CLASS_BLOCK_BYTES (the static_assert's bound),
    and that bound leaves the rest of a 4 KiB kernel-argument segment to the pointers."""
    hdr = open(os.path.join(ROOT, 'include', 'gca_hip.h')).read()
    bound = int(re.search(r'#define\s+GCA_CLASS_BLOCK_BYTES\s+(\d+)', hdr).group(1))
    size = pkg._hip.lib.gca_conv_class_block_bytes()
    assert 8 * 150 < size <= bound <= 4096 - 5 * 8, (size, bound)


def test_merged_work_space_is_the_sum_over_classes_host_side(pkg):
    """CPU only: gca_conv_dgrad_ws_bytes stays the maximum over classes, gca_conv_dgrad_ws_bytes_merged is the sum; the merge
    switch is a plain setting."""
    H = pkg._hip
    # (2, 24, 5, 9, 11) -> 40, (1,3,3) stride (1,2,2) pad (0,1,1): classes of 5*5*6, 5*5*5, 5*4*6, 5*4*5 positions per image
    g = H.ConvGeom(2, 24, 5, 9, 11, 40, 1, 3, 3, 1, 2, 2, 0, 1, 1, 5, 5, 6, 0)
    g.tune_dgrad_bm, g.tune_dgrad_splits = 32, 3
    cols = [2 * 5 * a * b for a in (5, 4) for b in (6, 5)]
    assert H.lib.gca_conv_dgrad_ws_bytes(C.byref(g)) == 3 * 24 * max(cols) * 4
    assert H.lib.gca_conv_dgrad_ws_bytes_merged(C.byref(g)) == 3 * 24 * sum(cols) * 4
    was = H.lib.gca_set_dgrad_merge(1)
    try:
        assert H.lib.gca_conv_dgrad_merged(C.byref(g), 3 * 24 * sum(cols) * 4) == 1
        assert H.lib.gca_conv_dgrad_merged(C.byref(g), 3 * 24 * sum(cols) * 4 - 1) == 0
        assert H.lib.gca_set_dgrad_merge(0) == 1
        assert H.lib.gca_conv_dgrad_merged(C.byref(g), 1 << 30) == 0
    finally:
        H.lib.gca_set_dgrad_merge(was)
    unit = H.ConvGeom(2, 24, 5, 9, 11, 40, 1, 3, 3, 1, 1, 1, 0, 1, 1, 5, 9, 11, 0)      # one class: nothing to merge
    assert H.lib.gca_conv_dgrad_merged(C.byref(unit), 1 << 30) == 0
    assert H.lib.gca_conv_dgrad_ws_bytes_merged(C.byref(unit)) == H.lib.gca_conv_dgrad_ws_bytes(C.byref(unit))
