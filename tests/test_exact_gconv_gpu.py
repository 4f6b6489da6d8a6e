"""Exact tests of the grouped 3x3 conv family (csrc/gconv.hip) through the C ABI:

  ssa_gconv3x3      y = round16(sum w x) over the group's Cg input channels and 9 taps; the BatchNorm sums of the stored y
  ssa_gconv3x3_bwd  dx (every pixel written) and dw ([C][Cg][3][3] fp32, written or added to), together and alone

Method of the other exact tests (exact_util): x and dy integers in [-2, 2], w in {-1, 0, 1} (exact in the 16-bit filter
operand), so |y| <= 18 Cg <= 576, every fp32 step and every partial sum of the kernels is exact and a float64 host
computation with ONE final rounding is the result bit for bit; every operand in a guarded buffer.  The host reference is
written tap by tap over index ranges (no library convolution), and is itself checked against torch's grouped conv2d and
its autograd below."""
import ctypes
import os

import pytest
import torch

from util import ACT_DTYPE
from exact_util import (assert_bits_equal, assert_guard_intact, assert_integers, assert_premise, guarded, guarded_copy,
                        ints, to_act, to_f32)

pytestmark = pytest.mark.gpu

DEV = "cuda"
_EMU = bool(os.environ.get("SSA_EMU"))

# id, (B, H, W, C, G), stride, dil, extra pixel stride of (x, y and dy, dx)
CASES = [
    ("1x1c128", (1, 1, 1, 128, 32), 1, 1, (0, 0, 0)),          # only the centre tap is in bounds
    ("3x3c1024d4", (1, 3, 3, 1024, 32), 1, 4, (0, 0, 0)),      # image smaller than the dilation; Cg = 32
    ("5x7c256", (2, 5, 7, 256, 32), 1, 1, (0, 0, 0)),          # plain two-image case; Cg = 8
    ("9x11c512d2", (1, 9, 11, 512, 32), 1, 2, (0, 0, 0)),      # dilation 2; Cg = 16
    ("7x10c256s2", (2, 7, 10, 256, 32), 2, 1, (8, 16, 8)),     # odd H; extra pixel strides
    ("8x9c128s2", (1, 8, 9, 128, 32), 2, 1, (0, 0, 0)),        # stride 2; Cg = 4
    ("5x6c48g6d3", (1, 5, 6, 48, 6), 1, 3, (0, 0, 0)),         # another group count, a ragged channel tile, dilation 3
    ("130x128c128", (1, 130, 128, 128, 32), 1, 1, (0, 0, 0)),  # past the grid caps: a workgroup walks several tiles
]
_IDS = [c[0] for c in CASES]
WAVES, BLOCKS, WG_BLOCKS = 4, 2048, 1024


def _out(n, s):
    return (n - 1) // s + 1


def _plan(shape, s):
    """Mirror of plan_grid / plan_wgrad (csrc/gconv.hip): a wave = one chunk of 16 channels x 16 pixels (forward, data
    gradient) or one 16 x 16 filter tile x 32 pixels (weight gradient); four waves per workgroup."""
    B, H, W, C, G = shape
    Cg = C // G
    Ho, Wo = _out(H, s), _out(W, s)
    chunks = -(-C // 16)
    ny = -(-chunks // WAVES)

    def grid(pixels):
        units = -(-pixels // 16)
        gx = min(units, max(1, BLOCKS // ny))
        return gx, -(-units // gx)
    ntile = chunks * (2 if Cg == 32 else 1)
    wy = -(-ntile // WAVES)
    steps = -(-(B * Ho * Wo) // 32)
    nsplit = min(steps, max(1, WG_BLOCKS // wy))
    return dict(Cg=Cg, chunks=chunks, ny=ny, idle_waves=ny * WAVES - chunks, fwd=grid(B * Ho * Wo), dgrad=grid(B * H * W),
                ntile=ntile, nsplit=nsplit, wg_walks=-(-steps // nsplit))


def test_exact_gconv_case_regimes():
    """The regime each case is listed for, on the mirror (not on the kernel)."""
    p = {c[0]: _plan(c[1], c[2]) for c in CASES}
    assert [p[n]["Cg"] for n in _IDS] == [4, 32, 8, 16, 8, 4, 8, 4]
    assert p["1x1c128"]["fwd"] == (1, 1)
    assert p["5x6c48g6d3"]["chunks"] == 3 and p["5x6c48g6d3"]["idle_waves"] == 1
    assert p["3x3c1024d4"]["ntile"] == 128 and p["9x11c512d2"]["ntile"] == 32
    assert (2 * 5 * 7) % 16 and (2 * 4 * 5) % 32                 # ragged last pixel unit / last k step
    big = p["130x128c128"]
    assert big["ny"] == 2 and big["fwd"] == (BLOCKS // 2, 2) and big["dgrad"] == (BLOCKS // 2, 2)
    assert big["nsplit"] == WG_BLOCKS // 2 and big["wg_walks"] == 2
    for name in _IDS[:-1]:
        assert p[name]["fwd"][1] == 1 and p[name]["dgrad"][1] == 1 and p[name]["wg_walks"] == 1, name


# ---- the host reference: tap by tap over index ranges, float64, NHWC; w [C, Cg, 3, 3]
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


def ref_fwd(x, w, s, d, G):
    B, H, W, C = x.shape
    Cg = C // G
    y = torch.zeros(B, _out(H, s), _out(W, s), C, dtype=torch.float64)
    for kh, kw, o, i in _pairs(H, W, s, d):
        xs = x[:, i[0], i[1]]
        wt = w[:, :, kh, kw].reshape(G, Cg, Cg)                            # [group][oc in group][ic in group]
        y[:, o[0], o[1]] += torch.einsum("byxgi,goi->byxgo", xs.reshape(xs.shape[:3] + (G, Cg)), wt).reshape(xs.shape)
    return y


def ref_bwd(x, dy, w, s, d, G):
    B, H, W, C = x.shape
    Cg = C // G
    dx = torch.zeros(B, H, W, C, dtype=torch.float64)
    dw = torch.zeros(C, Cg, 3, 3, dtype=torch.float64)
    for kh, kw, o, i in _pairs(H, W, s, d):
        g = dy[:, o[0], o[1]]
        g5 = g.reshape(g.shape[:3] + (G, Cg))
        xs = x[:, i[0], i[1]].reshape(g5.shape)
        wt = w[:, :, kh, kw].reshape(G, Cg, Cg)
        dx[:, i[0], i[1]] += torch.einsum("byxgo,goi->byxgi", g5, wt).reshape(g.shape)
        dw[:, :, kh, kw] = torch.einsum("byxgo,byxgi->goi", g5, xs).reshape(C, Cg)
    return dx, dw


@pytest.mark.parametrize("s,d,G", [(1, 1, 4), (1, 2, 2), (1, 4, 4), (2, 1, 2)])
def test_host_reference_against_torch(s, d, G):
    """ref_fwd / ref_bwd equal F.conv2d(groups = G) and its autograd in float64 (integers: exactly)."""
    B, H, W, C = 2, 7, 10, 16
    x, w = ints((B, H, W, C), -2, 2, 1).double(), ints((C, C // G, 3, 3), -1, 1, 2).double()
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wn = w.clone().requires_grad_(True)
    y = torch.nn.functional.conv2d(xn, wn, None, s, d, d, G)
    dy = ints(tuple(y.permute(0, 2, 3, 1).shape), -2, 2, 3).double()
    y.backward(dy.permute(0, 3, 1, 2))
    assert torch.equal(ref_fwd(x, w, s, d, G), y.detach().permute(0, 2, 3, 1))
    dx, dw = ref_bwd(x, dy, w, s, d, G)
    assert torch.equal(dx, xn.grad.permute(0, 2, 3, 1)) and torch.equal(dw, wn.grad)


# ---- operands and references of a case, computed once
_REF = {}


def _case(case):
    name, shape, s, d, extra = case
    if name not in _REF:
        B, H, W, C, G = shape
        Cg = C // G
        x, w = ints((B, H, W, C), -2, 2, 800), ints((C, Cg, 3, 3), -1, 1, 801)
        dy = ints((B, _out(H, s), _out(W, s), C), -2, 2, 802)
        assert_integers("gconv operands", x, w, dy)
        y64 = ref_fwd(x.double(), w.double(), s, d, G)
        assert_premise("gconv y", ref_fwd(x.double().abs(), w.double().abs(), s, d, G))
        dx64, dw64 = ref_bwd(x.double(), dy.double(), w.double(), s, d, G)
        adx, adw = ref_bwd(x.double().abs(), dy.double().abs(), w.double().abs(), s, d, G)
        assert_premise("gconv dx", adx)
        assert_premise("gconv dw: sum |x| |dy| over all pixels", adw)
        yi = to_act(y64).double().long().view(-1, C)                  # the values AS STORED (bf16 holds integers to 256)
        sums = torch.stack([yi.sum(0), (yi * yi).sum(0)]).double()
        # a lane adds the squares of its own pixels in fp32 (one per unit it walks), everything after that is fp64
        assert_premise("a lane's sum of y^2", _plan(shape, s)["fwd"][1] * (yi * yi).max().double().view(1))
        _REF[name] = dict(x=x, w=w, dy=dy, y=to_act(y64), dx=to_act(dx64), dw=to_f32(dw64), sums=sums)
    return _REF[name]


def _lib():
    from semseg_amd import hip_backend as hb
    from semseg_amd._lib import GConvDesc, check
    return hb, hb.lib(), check, GConvDesc


def _big(case):
    """The one case a workgroup walks several tiles in runs every check of the others on the device; 2.1 M elements
    are too slow for the emulation."""
    if _EMU and case[1][0] * case[1][1] * case[1][2] * case[1][3] > 1e6:
        pytest.skip("2.1 M elements: GPU only")


def _desc(D, shape, s, d, extra):
    B, H, W, C, G = shape
    return D(B, H, W, C, G, C + extra[0], _out(H, s), _out(W, s), C + extra[1], s, d)


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_exact_gconv_forward(case):
    """y bit for bit, plain and with stats; the sums equal to the int64 sums of the stored y, into a zeroed table and once
    more accumulating."""
    _big(case)
    hb, L, check, D = _lib()
    name, shape, s, d, extra = case
    B, H, W, C, G = shape
    r = _case(case)
    Ho, Wo = _out(H, s), _out(W, s)
    desc = _desc(D, shape, s, d, extra)
    ldy = C + extra[1]
    xg, wg = guarded_copy(r["x"].to(ACT_DTYPE), DEV, C + extra[0]), guarded_copy(r["w"], DEV)
    nrep = hb.stat_replicas()
    stats = guarded((nrep, 2, C), torch.float64, DEV)
    stats.view.zero_()
    outs, k = [], 0
    for st in (None, stats, stats):
        yg = guarded((B, Ho, Wo, C), ACT_DTYPE, DEV, ldy)
        check(L.ssa_gconv3x3(ctypes.byref(desc), hb._p(xg.view), hb._p(wg.view), hb._p(yg.view),
                             None if st is None else hb._p(st.view), hb._s()), "ssa_gconv3x3")
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
        assert_bits_equal("gconv %s y (call %d)" % (name, i), yg.view.cpu(), r["y"])
    assert_guard_intact("gconv fwd %s" % name, xg, wg, stats, *outs)
    assert float(r["y"].float().abs().max()) > 0


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_exact_gconv_backward(case):
    """dx bit for bit and dw exactly: both in one call (dw written over NaN), both with dw added onto integers, and each
    alone; the workspace is exactly ssa_gconv3x3_bwd_plan's bytes inside a guarded buffer."""
    _big(case)
    hb, L, check, D = _lib()
    name, shape, s, d, extra = case
    B, H, W, C, G = shape
    Cg = C // G
    r = _case(case)
    desc = _desc(D, shape, s, d, extra)
    lddy, lddx = C + extra[1], C + extra[2]
    nbytes = ctypes.c_size_t(0)
    check(L.ssa_gconv3x3_bwd_plan(ctypes.byref(desc), ctypes.byref(nbytes)), "ssa_gconv3x3_bwd_plan")
    pl = _plan(shape, s)
    assert nbytes.value == pl["nsplit"] * pl["ntile"] * 9 * 256 * 4
    xg, wg = guarded_copy(r["x"].to(ACT_DTYPE), DEV, C + extra[0]), guarded_copy(r["w"], DEV)
    dyg = guarded_copy(r["dy"].to(ACT_DTYPE), DEV, lddy)
    pre = ints((C, Cg, 3, 3), -9, 9, 820)
    forms = [("both", True, True, 0), ("both, accumulate", True, True, 1), ("dx alone", True, False, 0),
             ("dw alone", False, True, 0)]
    for what, want_dx, want_dw, acc in forms:
        dxg = guarded((B, H, W, C), ACT_DTYPE, DEV, lddx)
        dwg = guarded((C, Cg, 3, 3), torch.float32, DEV)
        wsg = guarded((nbytes.value // 4,), torch.float32, DEV)
        if acc:
            dwg.view.copy_(pre)
        check(L.ssa_gconv3x3_bwd(ctypes.byref(desc), hb._p(xg.view), hb._p(dyg.view), lddy, hb._p(wg.view),
                                 hb._p(dxg.view) if want_dx else None, lddx, hb._p(dwg.view) if want_dw else None, acc,
                                 hb._p(wsg.view), hb._s()), "ssa_gconv3x3_bwd")
        torch.cuda.synchronize()
        tag = "gconv bwd %s (%s)" % (name, what)
        if want_dx:
            assert_bits_equal(tag + " dx", dxg.view.cpu(), r["dx"])
        if want_dw:
            assert_bits_equal(tag + " dw", dwg.view.cpu(), to_f32(r["dw"].double() + (pre.double() if acc else 0.0)))
        assert_guard_intact(tag, dxg, dwg, wsg, xg, wg, dyg)     # (a result not asked for keeps its NaN fill: view included)
        if not want_dx:
            assert bool(torch.isnan(dxg.view.float()).all()), tag + ": dx written though NULL"
        if not want_dw:
            assert bool(torch.isnan(dwg.view).all()), tag + ": dw written though NULL"


def test_gconv_argument_checks():
    """Bad descriptors return -1 before the device is touched: C % 8, C % G, stride 2 with a dilation, an Ho / Wo that
    does not match, a pixel stride below C, an operand off its 16-byte boundary, neither gradient asked for; a group
    width other than 4, 8, 16, 32 returns -2."""
    hb, L, check, D = _lib()
    t = torch.zeros(8192, dtype=ACT_DTYPE, device=DEV)
    f = torch.zeros(8192, dtype=torch.float32, device=DEV)
    p, pf = hb._p(t), hb._p(f)
    n = ctypes.c_size_t(0)

    def all3(desc):
        return (L.ssa_gconv3x3(ctypes.byref(desc), p, pf, p, None, hb._s()),
                L.ssa_gconv3x3_bwd_plan(ctypes.byref(desc), ctypes.byref(n)),
                L.ssa_gconv3x3_bwd(ctypes.byref(desc), p, p, desc.C, pf, p, desc.C, pf, 0, pf, hb._s()))
    good = D(1, 4, 6, 16, 2, 16, 4, 6, 16, 1, 1)
    assert L.ssa_gconv3x3_bwd_plan(ctypes.byref(good), ctypes.byref(n)) == 0 and n.value == 1 * 1 * 9 * 256 * 4
    assert all3(D(1, 4, 6, 12, 3, 16, 4, 6, 16, 1, 1)) == (-1, -1, -1)        # C % 8
    assert all3(D(1, 4, 6, 16, 3, 16, 4, 6, 16, 1, 1)) == (-1, -1, -1)        # C % G
    assert all3(D(1, 4, 6, 16, 0, 16, 4, 6, 16, 1, 1)) == (-1, -1, -1)        # G
    assert all3(D(1, 4, 6, 16, 2, 16, 2, 3, 16, 2, 2)) == (-1, -1, -1)        # stride 2 with dilation 2
    assert all3(D(1, 4, 6, 16, 2, 16, 2, 3, 16, 3, 1)) == (-1, -1, -1)        # stride 3
    assert all3(D(1, 4, 6, 16, 2, 16, 3, 6, 16, 1, 1)) == (-1, -1, -1)        # Ho
    assert all3(D(1, 4, 6, 16, 2, 16, 4, 5, 16, 1, 1)) == (-1, -1, -1)        # Wo
    assert all3(D(1, 4, 6, 16, 2, 8, 4, 6, 16, 1, 1)) == (-1, -1, -1)         # ldx < C
    assert all3(D(1, 4, 6, 16, 2, 16, 4, 6, 8, 1, 1)) == (-1, -1, -1)         # ldy < C
    assert all3(D(1, 4, 6, 16, 16, 16, 4, 6, 16, 1, 1)) == (-2, -2, -2)       # Cg = 1: the depthwise kernels' case
    assert all3(D(1, 4, 6, 48, 4, 48, 4, 6, 48, 1, 1)) == (-2, -2, -2)        # Cg = 12
    assert all3(D(1, 4, 6, 64, 1, 64, 4, 6, 64, 1, 1)) == (-2, -2, -2)        # Cg = 64
    assert L.ssa_gconv3x3_bwd(ctypes.byref(good), p, p, 8, pf, p, 16, pf, 0, pf, hb._s()) == -1       # lddy < C
    assert L.ssa_gconv3x3_bwd(ctypes.byref(good), p, p, 16, pf, p, 8, pf, 0, pf, hb._s()) == -1       # lddx < C
    assert L.ssa_gconv3x3_bwd(ctypes.byref(good), p, p, 16, pf, None, 16, None, 0, pf, hb._s()) == -1  # nothing asked for
    assert L.ssa_gconv3x3_bwd(ctypes.byref(good), p, p, 16, pf, None, 16, pf, 0, None, hb._s()) == -1  # dw without ws
    off = lambda q, nbytes: ctypes.c_void_p(q.value + nbytes)  # noqa: E731
    assert p.value % 16 == 0
    assert L.ssa_gconv3x3(ctypes.byref(good), off(p, 2), pf, p, None, hb._s()) == -1                    # x
    assert L.ssa_gconv3x3(ctypes.byref(good), p, pf, off(p, 8), None, hb._s()) == -1                    # y
    assert L.ssa_gconv3x3(ctypes.byref(good), p, None, p, None, hb._s()) == -1                          # no filter
    assert L.ssa_gconv3x3_bwd(ctypes.byref(good), p, off(p, 2), 16, pf, p, 16, pf, 0, pf, hb._s()) == -1     # dy
    assert L.ssa_gconv3x3_bwd(ctypes.byref(good), p, p, 16, pf, off(p, 8), 16, pf, 0, pf, hb._s()) == -1     # dx
