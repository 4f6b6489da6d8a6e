"""Exact tests of the rectangular-dilation 3x3 conv family (csrc/conv_dil.hip) through the C ABI: ssa_dilconv3x3 (forward
and, on the mode-3 filter, the data gradient), ssa_dilconv3x3_wgrad_plan / ssa_dilconv3x3_wgrad.

Method of the other exact tests (exact_util): integer operands, so every product and every partial sum of the kernels,
in any order, is an integer fp32 holds exactly (premise asserted on the float64 reference); the one rounding left is the
store to the 16-bit format, which torch reproduces: the outputs are compared bit for bit, the BatchNorm partial sums,
summed over the replicas, and the weight gradients with == against float64.  Every operand lives in a guarded buffer
(NaN all around, outputs pre-filled with NaN).  Cases: tests/dilconv_cases.py."""
import ctypes

import pytest
import torch

from util import ACT_DTYPE
from exact_util import assert_bits_equal, assert_guard_intact, guarded, guarded_copy, ints, not_representable
import dilconv_cases as DC

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _lib():
    from semseg_amd import hip_backend as hb
    from semseg_amd._lib import DilConvDesc, check
    return hb, hb.lib(), check, DilConvDesc


def _pack(hb, w, mode):
    """ssa_pack_filter through the pack cache: mode 2 (forward, cin_pad = Cin) or 3 (data gradient, cout_pad = Cout)."""
    Cout, Cin = w.shape[:2]
    wp = hb._packed_filter(w.to(DEV), mode, Cin if mode == 2 else 0, Cout if mode == 3 else 0)[0]
    rows, k = (Cout, Cin) if mode == 2 else (Cin, Cout)
    assert tuple(wp.shape) == (-(-rows // 32) * 32, 9 * k) and wp.data_ptr() % 16 == 0
    return wp


def test_dilconv_case_regimes():
    """The regime each case is listed for, on a mirror of the launch geometry (not on the kernel)."""
    by = {c[0]: c for c in DC.CASES}
    g = {n: DC.geometry(c) for n, c in by.items()}
    assert (g["r2x12"]["tiles"], g["r2x12"]["last"]) == (6, 57) and by["r2x12"][1][0] == 2
    assert (g["r36x30"]["tiles"], g["r36x30"]["last"]) == (32, 16)
    assert g["out"]["tiles"] == 2 and g["edge"]["last"] == 403 - 6 * 64
    assert g["k192"]["chunks"] == 3 and g["k4096"]["chunks"] == 64 and g["k192"]["tiles"] == 2
    assert (g["n256"]["groups"], g["n256"]["last_waves"]) == (1, 4) and (g["n320"]["groups"], g["n320"]["last_waves"]) == (2, 1)
    assert by["dgrad"][5] == "dgrad" and by["dgrad"][2:4] == (256, 64) and by["sliced"][5] == "sliced"
    p = {c[0]: DC.wg_plan(c) for c in DC.WG_CASES}
    assert (p["wg_r2x12"]["stages_img"], p["wg_r2x12"]["nsplit"], p["wg_r2x12"]["per"]) == (6, 12, 1)
    assert (p["wg_out"]["total"], p["wg_out"]["nsplit"]) == (2, 2)
    assert (p["wg_split"]["ntile"], p["wg_split"]["total"], p["wg_split"]["nsplit"], p["wg_split"]["per"]) == (18, 32, 16, 2)
    assert p["wg_r36x30"]["nsplit"] == 16 and p["wg_r36x30"]["per"] == 2


def test_dilconv_cases_need_rounding():
    """bf16 (8 significant bits): outputs beyond 256 that the format cannot hold occur in the cases, so the rounding mode
    decides results.  fp16 holds every integer up to 2048, more than the premise on the squares allows."""
    n = sum(not_representable(DC.case_ref(c)["y64"]) for c in DC.CASES if c[0] in ("r2x12", "sq", "dgrad"))
    print("[exact dilconv] %d outputs not representable in %s" % (n, ACT_DTYPE))
    if ACT_DTYPE == torch.bfloat16:
        assert n > 0


def _forward(hb, L, check, D, x_view, ldx, wp, y_view, ldy, stats, shape, Cin, Cout, dil):
    B, H, W = shape
    d = D(B, H, W, Cin, ldx, Cout, ldy, dil[0], dil[1])
    assert L.ssa_dilconv3x3_supported(ctypes.byref(d)) == 1
    check(L.ssa_dilconv3x3(ctypes.byref(d), hb._p(x_view), hb._p(wp), hb._p(y_view), hb._p(stats), hb._s()), "ssa_dilconv3x3")


def _check_sums(tag, sg, prefill, want):
    got = sg.view.cpu().sum(0) - prefill.sum(0)
    for row, what in ((0, "sums"), (1, "sums of squares")):
        bad = got[row] != want[row]
        assert not bool(bad.any()), "%s %s differ in %d channels; first: channel %d got %r want %r" % (
            tag, what, int(bad.sum()), int(bad.nonzero()[0]), float(got[row][bad][0]), float(want[row][bad][0]))


@pytest.mark.parametrize("case", DC.CASES, ids=DC.IDS)
def test_exact_dilconv(case):
    """Output bits (every element written: the buffer starts as NaN), the statistics of the rounded outputs ADDED to a
    pre-filled replica buffer, the guards around x, y and the statistics; for the smallest case the same launch without
    statistics as well.  The data-gradient case runs without statistics (its contract)."""
    hb, L, check, D = _lib()
    name, shape, Cin, Cout, dil, kind, _ = case
    B, H, W = shape
    r = DC.case_ref(case)
    hb.clear_pack_cache()
    wsrc, mode = r["pack"]
    wp = _pack(hb, wsrc, mode)
    nrep = hb.stat_replicas()
    for with_stats in ((True, False) if name == "out" else ((False,) if kind == "dgrad" else (True,))):
        tag = "dilconv %s%s" % (name, "" if with_stats else " (no stats)")
        if kind == "sliced":
            # x = channels [0, 64), y = channels [64, 128) of ONE [B,H,W,320] buffer; the rest keeps its sentinel
            buf = guarded((B, H, W, DC.SLICED_LD), ACT_DTYPE, DEV)
            buf.view.fill_(7.0)
            buf.view[..., :Cin].copy_(r["x"].to(ACT_DTYPE))
            xv, yv, ldx, ldy = buf.view[..., :Cin], buf.view[..., Cin:Cin + Cout], DC.SLICED_LD, DC.SLICED_LD
            held = [buf]
        else:
            xg = guarded_copy(r["x"].to(ACT_DTYPE), DEV)
            yg = guarded((B, H, W, Cout), ACT_DTYPE, DEV)
            xv, yv, ldx, ldy = xg.view, yg.view, Cin, Cout
            held = [xg, yg]
        sg = prefill = None
        if with_stats:
            sg = guarded((nrep, 2, Cout), torch.float64, DEV)
            prefill = ints((nrep, 2, Cout), -1000, 1000, 77).double()
            sg.view.copy_(prefill)
            held.append(sg)
        _forward(hb, L, check, D, xv, ldx, wp, yv, ldy, sg.view if sg else None, shape, Cin, Cout, dil)
        torch.cuda.synchronize()
        assert_bits_equal(tag, yv.cpu().contiguous(), r["y"])
        if kind == "sliced":
            rest = buf.view.cpu()
            assert torch.equal(rest[..., :Cin], r["x"].to(ACT_DTYPE)), "%s: x was written" % tag
            assert bool((rest[..., Cin + Cout:] == 7.0).all()), "%s: channels outside y's slice were written" % tag
        if sg is not None:
            _check_sums(tag, sg, prefill, r["sums"])
        assert_guard_intact(tag, *held)
    hb.clear_pack_cache()


def test_exact_dilconv_grouped():
    """Three problems of one shape on one input with three rate pairs (b, c, d of the cell) issued inside ONE group bracket
    equal their single launches bit for bit, and the float64 references; one launch for the three."""
    hb, L, check, D = _lib()
    probs = DC.grouped_refs()
    hb.clear_pack_cache()
    B, H, W, Cin = probs[0]["x"].shape
    xg = guarded_copy(probs[0]["x"].to(ACT_DTYPE), DEV)
    wps = [_pack(hb, p["w"], 2) for p in probs]
    Cout = probs[0]["w"].shape[0]

    def run(grouped):
        ys = [guarded((B, H, W, Cout), ACT_DTYPE, DEV) for _ in probs]
        L.ssa_launch_count(1)
        if grouped:
            with hb.group():
                for p, wp, y in zip(probs, wps, ys):
                    _forward(hb, L, check, D, xg.view, Cin, wp, y.view, Cout, None, (B, H, W), Cin, Cout, p["dil"])
        else:
            for p, wp, y in zip(probs, wps, ys):
                _forward(hb, L, check, D, xg.view, Cin, wp, y.view, Cout, None, (B, H, W), Cin, Cout, p["dil"])
        torch.cuda.synchronize()
        return ys, L.ssa_launch_count(0)
    single, n1 = run(False)
    group, n3 = run(True)
    assert (n1, n3) == (3, 1), "launches: %d single, %d grouped" % (n1, n3)
    for p, s, g in zip(probs, single, group):
        tag = "dilconv grouped %s" % (p["dil"],)
        assert_bits_equal(tag + " against the single launch", g.view.cpu(), s.view.cpu())
        assert_bits_equal(tag, g.view.cpu(), p["y"])
    assert_guard_intact("dilconv grouped", xg, *single, *group)
    hb.clear_pack_cache()


@pytest.mark.parametrize("case", DC.WG_CASES, ids=DC.WG_IDS)
def test_exact_dilconv_wgrad(case):
    """dW == float64 autograd of F.conv2d, overwritten (dW and the workspace start as NaN: every element the contract
    says is written must be) and added to (dW starts as known integers).  The plan's split count is the mirror's: for
    wg_split each split walks two stages of a two-block filter, so the result does not depend on where the pixel axis is cut."""
    hb, L, check, D = _lib()
    name, (B, H, W), Cin, Cout, dil = case
    r = DC.wg_ref(case)
    d = D(B, H, W, Cin, Cin, Cout, Cout, dil[0], dil[1])
    nsplit, nbytes = ctypes.c_int(0), ctypes.c_size_t(0)
    check(L.ssa_dilconv3x3_wgrad_plan(ctypes.byref(d), ctypes.byref(nsplit), ctypes.byref(nbytes)), "ssa_dilconv3x3_wgrad_plan")
    assert nsplit.value == DC.wg_plan(case)["nsplit"] and nbytes.value == nsplit.value * 9 * Cout * Cin * 4
    xg = guarded_copy(r["x"].to(ACT_DTYPE), DEV)
    gg = guarded_copy(r["dy"].to(ACT_DTYPE), DEV)
    base = ints((Cout, Cin, 3, 3), -50, 50, 5)
    for accumulate in (0, 1):
        tag = "dilconv %s accumulate=%d" % (name, accumulate)
        ws = guarded((nbytes.value // 4,), torch.float32, DEV)
        dw = guarded((Cout, Cin, 3, 3), torch.float32, DEV)
        if accumulate:
            dw.view.copy_(base)
        check(L.ssa_dilconv3x3_wgrad(ctypes.byref(d), hb._p(xg.view), hb._p(gg.view), Cout, hb._p(dw.view), accumulate,
                                     hb._p(ws.view), hb._s()), "ssa_dilconv3x3_wgrad")
        torch.cuda.synchronize()
        want = r["dw"] + base if accumulate else r["dw"]
        assert_bits_equal(tag, dw.view.cpu() + 0.0, want + 0.0)          # (+ 0.0: -0.0 and 0.0 are one gradient)
        assert not bool(torch.isnan(ws.view).any()), "%s: a workspace element was not written" % tag
        assert_guard_intact(tag, xg, gg, ws, dw)


def test_dilconv_argument_checks():
    """Rejections return the documented code and launch nothing: a channel count that is no multiple of 64 -2; a NULL or
    misaligned operand, dil < 1, ldx < Cin, ldy < Cout, a stride that is no multiple of 8, B / H / W < 1 -1."""
    hb, L, check, D = _lib()
    t = torch.zeros(1 << 16, dtype=ACT_DTYPE, device=DEV)
    dd = torch.zeros(4096, dtype=torch.float64, device=DEV)
    f = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    p, pd, pf = hb._p(t), hb._p(dd), hb._p(f)
    off = lambda q, nbytes: ctypes.c_void_p(q.value + nbytes)  # noqa: E731

    def desc(B=1, H=4, W=8, Cin=64, ldx=None, Cout=64, ldy=None, dh=2, dw=3):
        return D(B, H, W, Cin, Cin if ldx is None else ldx, Cout, Cout if ldy is None else ldy, dh, dw)

    def run(d, x=p, w=p, y=p):
        return L.ssa_dilconv3x3(ctypes.byref(d), x, w, y, pd, hb._s())

    def wg(d, x=p, dy=p, lddy=64, dw=pf, ws=pf):
        return L.ssa_dilconv3x3_wgrad(ctypes.byref(d), x, dy, lddy, dw, 0, ws, hb._s())
    good = desc()
    L.ssa_launch_count(1)
    assert L.ssa_dilconv3x3_supported(ctypes.byref(good)) == 1 and L.ssa_dilconv3x3_supported(None) == 0
    assert run(good, x=None) == -1 and run(good, w=None) == -1 and run(good, y=None) == -1
    assert L.ssa_dilconv3x3(None, p, p, p, pd, hb._s()) == -1
    assert run(good, x=off(p, 2)) == -1 and run(good, y=off(p, 8)) == -1 and run(good, w=off(p, 4)) == -1
    ns, nb = ctypes.c_int(0), ctypes.c_size_t(0)
    for d in (desc(Cin=72), desc(Cin=32), desc(Cout=96), desc(Cout=8)):
        assert run(d) == -2 and wg(d) == -2 and L.ssa_dilconv3x3_supported(ctypes.byref(d)) == 0, (d.Cin, d.Cout)
        assert L.ssa_dilconv3x3_wgrad_plan(ctypes.byref(d), ctypes.byref(ns), ctypes.byref(nb)) == -2
    for d in (desc(dh=0), desc(dw=0), desc(dh=-1), desc(ldx=56), desc(ldy=32), desc(ldx=68), desc(ldy=132), desc(B=0),
              desc(H=0), desc(W=0), desc(Cin=0), desc(Cout=0)):
        assert run(d) == -1 and wg(d) == -1 and L.ssa_dilconv3x3_supported(ctypes.byref(d)) == 0, \
            (d.B, d.H, d.W, d.Cin, d.ldx, d.Cout, d.ldy, d.dil_h, d.dil_w)
        assert L.ssa_dilconv3x3_wgrad_plan(ctypes.byref(d), ctypes.byref(ns), ctypes.byref(nb)) == -1
    assert wg(good, x=None) == -1 and wg(good, dy=None) == -1 and wg(good, dw=None) == -1 and wg(good, ws=None) == -1
    assert wg(good, lddy=56) == -1 and wg(good, lddy=68) == -1 and wg(good, dy=off(p, 2)) == -1
    assert L.ssa_dilconv3x3_wgrad_plan(ctypes.byref(good), ctypes.byref(ns), None) == -1
    assert L.ssa_launch_count(0) == 0, "a rejected call launched"
