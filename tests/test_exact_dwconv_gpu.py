"""Exact tests of the depthwise 3x3 conv family (csrc/dwconv.hip) through the C ABI:

  ssa_dwconv3x3      y = round16(sum_taps w x); the BatchNorm sums of the stored y; the inference affine epilogue
  ssa_dwconv3x3_bwd  dx (a gather, every pixel written) and dw ([C][9] fp32, written or added to), together and alone

Method of the other exact tests (exact_util): x and dy integers in [-2, 2], w in {-1, 0, 1}, so |y| <= 18, every fp32 step
and every partial sum of the kernels is exact and a float64 host computation with ONE final rounding is the result bit
for bit; every operand in a guarded buffer.  The host reference is written tap by tap over index ranges (no library
convolution), and is itself checked against torch's grouped conv2d and its autograd below."""
import ctypes
import os

import pytest
import torch

from util import ACT_DTYPE
from exact_util import (assert_bits_equal, assert_guard_intact, assert_integers, assert_premise, choice, guarded,
                        guarded_copy, ints, pow2, to_act, to_f32)

pytestmark = pytest.mark.gpu

DEV = "cuda"
_EMU = bool(os.environ.get("SSA_EMU"))

# id, (B, H, W, C), stride, dil, extra pixel stride of (x, y and dy, dx)
CASES = [
    ("1x1c8", (1, 1, 1, 8), 1, 1, (0, 0, 0)),            # only the centre tap is ever in bounds
    ("3x3c8d4", (1, 3, 3, 8), 1, 4, (0, 0, 0)),          # image smaller than the dilation: centre tap only
    ("5x7c24d2", (2, 5, 7, 24), 1, 2, (0, 0, 0)),        # two images; odd W against the per-thread run
    ("9x11c728d4", (1, 9, 11, 728), 1, 4, (0, 0, 0)),    # 91 channel groups; rows with 1, 2 and 3 taps in bounds
    ("7x10c128s2", (2, 7, 10, 128), 2, 1, (8, 16, 8)),   # odd H: the last output row's bottom taps are out of bounds
    ("8x9c64s2", (1, 8, 9, 64), 2, 1, (0, 0, 0)),        # even H, odd W
    ("5x6c16d3", (1, 5, 6, 16), 1, 3, (0, 0, 0)),        # a dilation no instantiation is specialised for
    ("130x256c256", (1, 130, 256, 256), 1, 1, (0, 0, 0)),  # past both workgroup caps: a workgroup walks several units
]
_IDS = [c[0] for c in CASES]
RUN_FWD, RUN_BWD, TILE, FWD_BLOCKS, BWD_BLOCKS = 4, 2, 16, 1024, 512


def _out(n, s):
    return (n - 1) // s + 1


def _plan(shape, s):
    """Mirror of Lane / plan_grid (csrc/dwconv.hip): a workgroup = TW channel groups x RP runs; grid = (gx, tiles)."""
    B, H, W, C = shape
    Ho, Wo = _out(H, s), _out(W, s)
    VC = C // 8
    TW = min(VC, TILE)
    RP, tiles = 256 // TW, -(-VC // TW)
    fr = B * Ho * -(-Wo // RUN_FWD)
    fb = min(-(-fr // RP), max(1, FWD_BLOCKS // tiles))
    br = B * H * -(-W // RUN_BWD)
    bb = min(-(-br // RP), max(1, BWD_BLOCKS // tiles))
    return dict(TW=TW, RP=RP, tiles=tiles, active=RP * TW, last_tile=VC - (tiles - 1) * TW, fwd_blocks=fb,
                fwd_units=-(-fr // (fb * RP)), bwd_blocks=bb, bwd_units=-(-br // (bb * RP)))


def test_exact_dwconv_case_regimes():
    """The regime each case is listed for, on the mirror (not on the kernel)."""
    p = {c[0]: _plan(c[1], c[2]) for c in CASES}
    assert p["1x1c8"]["RP"] == 256 and p["1x1c8"]["fwd_blocks"] == 1
    assert p["5x7c24d2"]["TW"] == 3 and p["5x7c24d2"]["active"] == 255          # one thread of the workgroup has no row
    assert p["9x11c728d4"]["tiles"] == 6 and p["9x11c728d4"]["last_tile"] == 11   # a ragged last channel tile
    assert 7 % RUN_FWD and 7 % RUN_BWD and 11 % RUN_FWD and 9 % RUN_BWD
    big = p["130x256c256"]
    assert big["tiles"] == 2 and big["fwd_blocks"] == FWD_BLOCKS // 2 and big["fwd_units"] == 2
    assert big["bwd_blocks"] == BWD_BLOCKS // 2 and big["bwd_units"] == 5
    for name in _IDS[:-1]:
        assert p[name]["fwd_units"] == 1 and p[name]["bwd_units"] == 1, name


# ---- the host reference: tap by tap over index ranges, float64, NHWC
def _tap(n_out, n_in, s, d, k):
    o = torch.arange(n_out)
    i = o * s - d + k * d
    m = (i >= 0) & (i < n_in)
    return o[m], i[m]


def _pairs(H, W, s, d):
    Ho, Wo = _out(H, s), _out(W, s)
    for kh in range(3):
        oy, iy = _tap(Ho, H, s, d, kh)
        for kw in range(3):
            ox, ix = _tap(Wo, W, s, d, kw)
            if len(oy) and len(ox):
                yield kh, kw, (oy[:, None], ox[None, :]), (iy[:, None], ix[None, :])


def ref_fwd(x, w, s, d):
    B, H, W, C = x.shape
    y = torch.zeros(B, _out(H, s), _out(W, s), C, dtype=torch.float64)
    for kh, kw, o, i in _pairs(H, W, s, d):
        y[:, o[0], o[1]] += x[:, i[0], i[1]] * w[:, kh, kw]
    return y


def ref_bwd(x, dy, w, s, d):
    B, H, W, C = x.shape
    dx = torch.zeros(B, H, W, C, dtype=torch.float64)
    dw = torch.zeros(C, 3, 3, dtype=torch.float64)
    for kh, kw, o, i in _pairs(H, W, s, d):
        g = dy[:, o[0], o[1]]
        dx[:, i[0], i[1]] += g * w[:, kh, kw]
        dw[:, kh, kw] = (x[:, i[0], i[1]] * g).sum((0, 1, 2))
    return dx, dw


@pytest.mark.parametrize("s,d", [(1, 1), (1, 2), (1, 4), (2, 1)])
def test_host_reference_against_torch(s, d):
    """ref_fwd / ref_bwd equal F.conv2d(groups = C) and its autograd in float64 (integers: exactly)."""
    B, H, W, C = 2, 7, 10, 8
    x, w = ints((B, H, W, C), -2, 2, 1).double(), ints((C, 3, 3), -1, 1, 2).double()
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wn = w.view(C, 1, 3, 3).clone().requires_grad_(True)
    y = torch.nn.functional.conv2d(xn, wn, None, s, d, d, C)
    dy = ints(tuple(y.permute(0, 2, 3, 1).shape), -2, 2, 3).double()
    y.backward(dy.permute(0, 3, 1, 2))
    assert torch.equal(ref_fwd(x, w, s, d), y.detach().permute(0, 2, 3, 1))
    dx, dw = ref_bwd(x, dy, w, s, d)
    assert torch.equal(dx, xn.grad.permute(0, 2, 3, 1)) and torch.equal(dw, wn.grad.view(C, 3, 3))


# ---- operands and references of a case, computed once
_REF = {}


def _case(case):
    name, shape, s, d, extra = case
    if name not in _REF:
        B, H, W, C = shape
        x, w = ints(shape, -2, 2, 700), ints((C, 3, 3), -1, 1, 701)
        dy = ints((B, _out(H, s), _out(W, s), C), -2, 2, 702)
        assert_integers("dwconv operands", x, w, dy)
        y64 = ref_fwd(x.double(), w.double(), s, d)
        assert_premise("dwconv y", ref_fwd(x.double().abs(), w.double().abs(), s, d))
        dx64, dw64 = ref_bwd(x.double(), dy.double(), w.double(), s, d)
        adx, adw = ref_bwd(x.double().abs(), dy.double().abs(), w.double().abs(), s, d)
        assert_premise("dwconv dx", adx)
        assert_premise("dwconv dw: sum |x| |dy| over all pixels", adw)
        yi = y64.long().view(-1, C)
        sums = torch.stack([yi.sum(0), (yi * yi).sum(0)]).double()
        assert_premise("sum of y^2 over the pixels", sums[1])
        _REF[name] = dict(x=x, w=w, dy=dy, y64=y64, y=to_act(y64), dx=to_act(dx64), dw=to_f32(dw64.view(C, 9)), sums=sums)
    return _REF[name]


def _lib():
    from semseg_amd import hip_backend as hb
    from semseg_amd._lib import DwConvDesc, check
    return hb, hb.lib(), check, DwConvDesc


def _big(case):
    """The one case a workgroup walks several units in runs every check of the others on the device; 256 fibers per
    workgroup make its 8.5 M elements too slow for the emulation."""
    if _EMU and case[1][0] * case[1][1] * case[1][2] * case[1][3] > 2e6:
        pytest.skip("8.5 M elements: GPU only")


def _desc(D, shape, s, d, extra):
    B, H, W, C = shape
    return D(B, H, W, C, C + extra[0], _out(H, s), _out(W, s), C + extra[1], s, d)


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_exact_dwconv_forward(case):
    """y bit for bit, plain and with stats; the sums equal to the int64 sums of the stored y, into a zeroed table and once
    more accumulating; the coef epilogue with and without ReLU equal to the float64 value and to ssa_bn_apply on the
    stored y."""
    _big(case)
    hb, L, check, D = _lib()
    name, shape, s, d, extra = case
    B, H, W, C = shape
    r = _case(case)
    Ho, Wo = _out(H, s), _out(W, s)
    desc = _desc(D, shape, s, d, extra)
    ldy = C + extra[1]
    xg, wg = guarded_copy(r["x"].to(ACT_DTYPE), DEV, C + extra[0]), guarded_copy(r["w"].reshape(C, 9), DEV)
    nrep = hb.stat_replicas()
    stats = guarded((nrep, 2, C), torch.float64, DEV)
    stats.view.zero_()
    outs, k = [], 0
    for st in (None, stats, stats):
        yg = guarded((B, Ho, Wo, C), ACT_DTYPE, DEV, ldy)
        check(L.ssa_dwconv3x3(ctypes.byref(desc), hb._p(xg.view), hb._p(wg.view), hb._p(yg.view),
                              None if st is None else hb._p(st.view), None, 0, hb._s()), "ssa_dwconv3x3")
        outs.append(yg)
        if st is not None:
            torch.cuda.synchronize()
            got = st.view.cpu().sum(0)
            k += 1
            for row in (0, 1):
                assert torch.equal(got[row], k * r["sums"][row]), "%s stats row %d after %d calls: %d channels differ" % (
                    name, row, k, int((got[row] != k * r["sums"][row]).sum()))
    torch.cuda.synchronize()
    for i, yg in enumerate(outs):
        assert_bits_equal("dwconv %s y (call %d)" % (name, i), yg.view.cpu(), r["y"])
    assert_guard_intact("dwconv fwd %s" % name, xg, wg, stats, *outs)
    coef = torch.stack([pow2((C,), -2, 1, 710, signed=True), choice((C,), [-1.5, -0.5, 0.0, 0.25, 1.0, 2.5], 711),
                        torch.zeros(C), torch.ones(C)])
    cg = guarded_copy(coef, DEV)
    ys = outs[0].view.contiguous()
    for relu in (0, 1):
        zg = guarded((B, Ho, Wo, C), ACT_DTYPE, DEV, ldy)
        check(L.ssa_dwconv3x3(ctypes.byref(desc), hb._p(xg.view), hb._p(wg.view), hb._p(zg.view), None, hb._p(cg.view), relu,
                              hb._s()), "ssa_dwconv3x3 (coef)")
        za = torch.empty_like(ys)
        check(L.ssa_bn_apply(hb._p(ys), C, None, 0, hb._p(za), C, B * Ho * Wo, C, hb._p(cg.view[0]), hb._p(cg.view[1]), relu,
                             None, Ho * Wo, hb._s()), "ssa_bn_apply")
        torch.cuda.synchronize()
        z64 = r["y"].double() * coef[0].double() + coef[1].double()
        z64 = z64.clamp(min=0.0) if relu else z64
        assert_bits_equal("dwconv %s coef relu=%d" % (name, relu), zg.view.cpu(), to_act(z64))
        assert_bits_equal("dwconv %s coef relu=%d against ssa_bn_apply" % (name, relu), zg.view.cpu(), za.cpu())
        assert_guard_intact("dwconv coef %s" % name, zg, cg)


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_exact_dwconv_backward(case):
    """dx bit for bit and dw exactly: both in one call (dw written over NaN), both with dw added onto integers, and each
    alone; the workspace is exactly ssa_dwconv3x3_bwd_plan's bytes inside a guarded buffer."""
    _big(case)
    hb, L, check, D = _lib()
    name, shape, s, d, extra = case
    B, H, W, C = shape
    r = _case(case)
    desc = _desc(D, shape, s, d, extra)
    lddy, lddx = C + extra[1], C + extra[2]
    nbytes = ctypes.c_size_t(0)
    check(L.ssa_dwconv3x3_bwd_plan(ctypes.byref(desc), ctypes.byref(nbytes)), "ssa_dwconv3x3_bwd_plan")
    assert nbytes.value == _plan(shape, s)["bwd_blocks"] * 9 * C * 4
    xg, wg = guarded_copy(r["x"].to(ACT_DTYPE), DEV, C + extra[0]), guarded_copy(r["w"].reshape(C, 9), DEV)
    dyg = guarded_copy(r["dy"].to(ACT_DTYPE), DEV, lddy)
    pre = ints((C, 9), -9, 9, 720)
    forms = [("both", True, True, 0), ("both, accumulate", True, True, 1), ("dx alone", True, False, 0),
             ("dw alone", False, True, 0)]
    for what, want_dx, want_dw, acc in forms:
        dxg = guarded((B, H, W, C), ACT_DTYPE, DEV, lddx)
        dwg = guarded((C, 9), torch.float32, DEV)
        wsg = guarded((nbytes.value // 4,), torch.float32, DEV)
        if acc:
            dwg.view.copy_(pre)
        check(L.ssa_dwconv3x3_bwd(ctypes.byref(desc), hb._p(xg.view), hb._p(dyg.view), lddy, hb._p(wg.view),
                                  hb._p(dxg.view) if want_dx else None, lddx, hb._p(dwg.view) if want_dw else None, acc,
                                  hb._p(wsg.view), hb._s()), "ssa_dwconv3x3_bwd")
        torch.cuda.synchronize()
        tag = "dwconv bwd %s (%s)" % (name, what)
        if want_dx:
            assert_bits_equal(tag + " dx", dxg.view.cpu(), r["dx"])
        if want_dw:
            assert_bits_equal(tag + " dw", dwg.view.cpu(), to_f32(r["dw"].double() + (pre.double() if acc else 0.0)))
        assert_guard_intact(tag, dxg, dwg, wsg, xg, wg, dyg)     # (a result not asked for keeps its NaN fill: view included)
        if not want_dx:
            assert bool(torch.isnan(dxg.view.float()).all()), tag + ": dx written though NULL"
        if not want_dw:
            assert bool(torch.isnan(dwg.view).all()), tag + ": dw written though NULL"


def test_dwconv_argument_checks():
    """Bad descriptors return -1 before the device is touched: C % 8, stride 2 with a dilation, an Ho / Wo that does not
    match, a pixel stride below C, an operand off its 16-byte boundary (the filter is read in 16-byte pieces too); stats and
    coef together -2."""
    hb, L, check, D = _lib()
    t = torch.zeros(4096, dtype=ACT_DTYPE, device=DEV)
    f = torch.zeros(4096, dtype=torch.float32, device=DEV)
    dd = torch.zeros(512, dtype=torch.float64, device=DEV)
    p, pf, pd = hb._p(t), hb._p(f), hb._p(dd)
    n = ctypes.c_size_t(0)

    def all3(desc):
        return (L.ssa_dwconv3x3(ctypes.byref(desc), p, pf, p, None, None, 0, hb._s()),
                L.ssa_dwconv3x3_bwd_plan(ctypes.byref(desc), ctypes.byref(n)),
                L.ssa_dwconv3x3_bwd(ctypes.byref(desc), p, p, desc.C, pf, p, desc.C, pf, 0, pf, hb._s()))
    good = D(1, 4, 6, 16, 16, 4, 6, 16, 1, 1)
    assert L.ssa_dwconv3x3_bwd_plan(ctypes.byref(good), ctypes.byref(n)) == 0 and n.value > 0
    assert all3(D(1, 4, 6, 12, 16, 4, 6, 16, 1, 1)) == (-1, -1, -1)        # C % 8
    assert all3(D(1, 4, 6, 16, 16, 2, 3, 16, 2, 2)) == (-1, -1, -1)        # stride 2 with dilation 2
    assert all3(D(1, 4, 6, 16, 16, 2, 3, 16, 3, 1)) == (-1, -1, -1)        # stride 3
    assert all3(D(1, 4, 6, 16, 16, 3, 6, 16, 1, 1)) == (-1, -1, -1)        # Ho
    assert all3(D(1, 5, 6, 16, 16, 2, 3, 16, 2, 1)) == (-1, -1, -1)        # Ho = (H - 1) / 2 + 1 = 3
    assert all3(D(1, 4, 6, 16, 16, 4, 5, 16, 1, 1)) == (-1, -1, -1)        # Wo
    assert all3(D(1, 4, 6, 16, 8, 4, 6, 16, 1, 1)) == (-1, -1, -1)         # ldx < C
    assert all3(D(1, 4, 6, 16, 16, 4, 6, 8, 1, 1)) == (-1, -1, -1)         # ldy < C
    assert L.ssa_dwconv3x3_bwd(ctypes.byref(good), p, p, 8, pf, p, 16, pf, 0, pf, hb._s()) == -1       # lddy < C
    assert L.ssa_dwconv3x3_bwd(ctypes.byref(good), p, p, 16, pf, p, 8, pf, 0, pf, hb._s()) == -1       # lddx < C
    assert L.ssa_dwconv3x3_bwd(ctypes.byref(good), p, p, 16, pf, None, 16, None, 0, pf, hb._s()) == -1  # nothing asked for
    assert L.ssa_dwconv3x3(ctypes.byref(good), p, pf, p, pd, pf, 0, hb._s()) == -2                     # stats and coef
    off = lambda q, nbytes: ctypes.c_void_p(q.value + nbytes)  # noqa: E731
    assert p.value % 16 == 0 and pf.value % 16 == 0
    assert L.ssa_dwconv3x3(ctypes.byref(good), p, off(pf, 4), p, None, None, 0, hb._s()) == -1          # filter at a 4-byte offset
    assert L.ssa_dwconv3x3(ctypes.byref(good), off(p, 2), pf, p, None, None, 0, hb._s()) == -1          # x
    assert L.ssa_dwconv3x3(ctypes.byref(good), p, pf, off(p, 8), None, None, 0, hb._s()) == -1          # y
    assert L.ssa_dwconv3x3_bwd(ctypes.byref(good), p, p, 16, off(pf, 4), p, 16, pf, 0, pf, hb._s()) == -1     # filter
    assert L.ssa_dwconv3x3_bwd(ctypes.byref(good), p, off(p, 2), 16, pf, p, 16, pf, 0, pf, hb._s()) == -1     # dy
    assert L.ssa_dwconv3x3_bwd(ctypes.byref(good), p, p, 16, pf, off(p, 8), 16, pf, 0, pf, hb._s()) == -1     # dx
