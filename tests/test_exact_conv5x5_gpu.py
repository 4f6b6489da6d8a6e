"""Exact tests of the 5x5 stride-1 pad-2 conv kernel (csrc/conv_halo5.hip) through the C ABI -- ssa_conv2d_halo5 itself, so
that the size policy of ssa_conv2d_halo5_supported does not hide the small shapes.

Method of the other exact tests (exact_util): integer operands, so every product and every partial sum of the kernel,
in any order, is an integer fp32 holds exactly (premise asserted on the float64 reference, conv_ref64); the one rounding
left is the store to the 16-bit format, which torch reproduces: the outputs are compared bit for bit and the BatchNorm
partial sums, summed over the replicas, with torch.equal against the float64 sums of the rounded outputs.  Every operand
lives in a guarded buffer (NaN all around, outputs pre-filled with NaN).  Cases: tests/conv5x5_cases.py."""
import ctypes

import pytest
import torch

from util import ACT_DTYPE
from exact_util import assert_bits_equal, assert_guard_intact, guarded, guarded_copy, not_representable
import conv5x5_cases as CC

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _lib():
    from semseg_amd import hip_backend as hb
    from semseg_amd._lib import ConvDesc, check
    return hb, hb.lib(), check, ConvDesc


def _desc(D, B, H, W, Cin, Cout, ldx=None, ldy=None, k=5, stride=1, pad=2, dil=1):
    return D(B, H, W, Cin, ldx or Cin, H, W, Cout, ldy or Cout, k, k, stride, pad, dil, 0, 0, 0, -1)


def test_conv5x5_case_regimes():
    """The regime each case is listed for, on a mirror of the launch geometry (not on the kernel)."""
    by = {c[0]: c for c in CC.CASES}

    def geom(name):
        _, (B, H, W), Cin, Cout, _, _, _, _ = by[name]
        ck = 64 if Cin % 64 == 0 else 48
        assert Cin % ck == 0
        nb = -(-Cout // 32)
        return dict(ck=ck, chunks=Cin // ck, tiles_x=-(-W // 32), tiles_y=-(-H // 4), last_rows=H - (-(-H // 4) - 1) * 4,
                    last_cols=W - (-(-W // 32) - 1) * 32, nb=nb, groups=-(-nb // 8), last_group=nb - (-(-nb // 8) - 1) * 8)
    g = geom("c64")
    assert (g["chunks"], g["tiles_x"], g["tiles_y"], g["last_rows"], g["last_cols"]) == (1, 2, 3, 1, 5)
    assert geom("c128")["chunks"] == 2 and geom("c96")["ck"] == 48 and geom("c96")["chunks"] == 2
    assert geom("c320")["chunks"] == 5 and (geom("c288")["ck"], geom("c288")["chunks"]) == (48, 6)
    assert (geom("d320")["nb"], geom("d320")["groups"], geom("d320")["last_group"]) == (10, 2, 2)
    assert (geom("d288")["nb"], geom("d288")["last_group"]) == (9, 1)
    assert geom("n40")["nb"] == 2 and 40 % 32 == 8
    assert by["sliced"][6] == (128, 280) and by["n40bias"][4] and by["d320"][5] and by["d288"][5]
    assert "c320" not in CC.EMU_IDS and "c288" not in CC.EMU_IDS and "d320" in CC.EMU_IDS and "c96" in CC.EMU_IDS


def test_conv5x5_cases_need_rounding():
    """bf16 (8 significant bits): outputs beyond 256 that the format cannot hold occur in the cases, so the rounding mode
    decides results.  fp16 holds every integer up to 2048, more than the premise on the squares allows: nothing to round."""
    n = sum(not_representable(CC.case_ref(c)["y64"]) for c in CC.CASES if c[0] in ("c64", "n40", "d320"))
    print("[exact conv5x5] %d outputs not representable in %s" % (n, ACT_DTYPE))
    if ACT_DTYPE == torch.bfloat16:
        assert n > 0


@pytest.mark.parametrize("case", CC.CASES, ids=CC.IDS)
def test_exact_conv5x5(case):
    """Output bits (every element written: the buffer starts as NaN), the statistics of the rounded outputs, the guards
    around x, y and the statistics; for the smallest case the same launch without statistics as well."""
    hb, L, check, D = _lib()
    name, (B, H, W), Cin, Cout, bias, dgrad, ld, _ = case
    r = CC.case_ref(case)
    ldx, ldy = ld if ld else (None, None)
    hb.clear_pack_cache()
    xg = guarded_copy(r["x"].to(ACT_DTYPE), DEV, ldx)
    wsrc, mode = r["pack"]
    wd = wsrc.to(DEV)
    wp = hb._packed_filter(wd, mode, Cin if mode == 2 else 0, Cin if mode == 3 else 0)[0]
    assert tuple(wp.shape) == (-(-Cout // 32) * 32, 25 * Cin) and wp.data_ptr() % 16 == 0
    d = _desc(D, B, H, W, Cin, Cout, ldx, ldy)
    bd = r["b"].to(DEV) if r["b"] is not None else None
    nrep = hb.stat_replicas()
    for with_stats in ((True, False) if name == "n40" else (True,)):
        yg = guarded((B, H, W, Cout), ACT_DTYPE, DEV, ldy)
        sg = None
        if with_stats:
            sg = guarded((nrep, 2, Cout), torch.float64, DEV)
            sg.view.zero_()
        check(L.ssa_conv2d_halo5(ctypes.byref(d), hb._p(xg.view), hb._p(wp), hb._p(bd), hb._p(yg.view),
                                 hb._p(sg.view) if sg else None, hb._s()), "ssa_conv2d_halo5")
        torch.cuda.synchronize()
        tag = "conv5x5 %s%s" % (name, "" if with_stats else " (no stats)")
        assert_bits_equal(tag, yg.view.cpu(), r["y"])
        if sg is not None:
            got = sg.view.cpu().sum(0)
            for row, what in ((0, "sums"), (1, "sums of squares")):
                bad = got[row] != r["sums"][row]
                assert not bool(bad.any()), "%s %s differ in %d channels; first: channel %d got %r want %r" % (
                    tag, what, int(bad.sum()), int(bad.nonzero()[0]), float(got[row][bad][0]), float(r["sums"][row][bad][0]))
        assert_guard_intact(tag, xg, yg, *([sg] if sg else []))
    hb.clear_pack_cache()


def test_conv5x5_argument_checks():
    """Rejections return the error code and launch nothing: a NULL operand and an operand off its 16-byte boundary -1; a
    filter that is not 5x5 stride 1 pad 2 dilation 1, a Cin no chunk width divides, an fp32 output, pixel strides that are
    no multiple of 8 or below the channel count -2."""
    hb, L, check, D = _lib()
    t = torch.zeros(1 << 16, dtype=ACT_DTYPE, device=DEV)
    dd = torch.zeros(4096, dtype=torch.float64, device=DEV)
    p, pd = hb._p(t), hb._p(dd)
    assert p.value % 16 == 0
    off = lambda q, nbytes: ctypes.c_void_p(q.value + nbytes)  # noqa: E731
    good = _desc(D, 1, 4, 8, 64, 32)

    def run(d, x=p, w=p, y=p):
        return L.ssa_conv2d_halo5(ctypes.byref(d), x, w, None, y, pd, hb._s())
    L.ssa_launch_count(1)
    assert run(good, x=None) == -1 and run(good, w=None) == -1 and run(good, y=None) == -1
    assert L.ssa_conv2d_halo5(None, p, p, None, p, pd, hb._s()) == -1
    assert run(good, x=off(p, 2)) == -1 and run(good, y=off(p, 8)) == -1 and run(good, w=off(p, 4)) == -1
    bad = [_desc(D, 1, 4, 8, 64, 32, stride=2), _desc(D, 1, 4, 8, 64, 32, dil=2), _desc(D, 1, 4, 8, 64, 32, pad=1),
           _desc(D, 1, 4, 8, 64, 32, k=3, pad=1), _desc(D, 1, 4, 8, 72, 32), _desc(D, 1, 4, 8, 0, 32), _desc(D, 1, 4, 8, -64, 32), _desc(D, 1, 4, 8, 64, 36),
           _desc(D, 1, 4, 8, 64, 32, ldx=68), _desc(D, 1, 4, 8, 64, 32, ldx=56), _desc(D, 1, 4, 8, 64, 32, ldy=24),
           _desc(D, 1, 4, 8, 64, 32, ldy=36), _desc(D, 0, 4, 8, 64, 32)]
    for d in bad:
        assert run(d) == -2, (d.KH, d.stride, d.pad, d.dil, d.Cin, d.Cout, d.ldx, d.ldy, d.B)
        assert L.ssa_conv2d_halo5_supported(ctypes.byref(d)) == 0
    f32 = _desc(D, 1, 4, 8, 64, 32)
    f32.out_f32 = 1
    assert run(f32) == -2
    tr = _desc(D, 1, 4, 8, 64, 32)
    tr.transposed = 1
    assert run(tr) == -2
    ho = _desc(D, 1, 4, 8, 64, 32)
    ho.Ho = 3
    assert run(ho) == -2
    assert L.ssa_launch_count(0) == 0, "a rejected call launched"
    # the policy: the entry point takes the small problem, the _supported query keeps it on the generic route
    assert L.ssa_conv2d_halo5_supported(ctypes.byref(good)) == 0
    assert L.ssa_conv2d_halo5_supported(ctypes.byref(_desc(D, 1, 128, 128, 320, 256))) == 1
