"""Exact tests of the squeeze-and-excitation gate (csrc/se.hip) and of the ceil-mode stem pool (csrc/pool_ceil.hip)
through the C ABI:

  ssa_se_squeeze_gate   mean, h bit for bit and s against the float64 sigmoid where HW is a power of two; elsewhere the mean
                        within 1 ulp, h and s within the rounding bound of an fp32 sum
  ssa_se_apply          z = round16(act(s y + r))
  ssa_se_bwd_reduce     ds = sum_p m dz y
  ssa_se_gate_bwd       g, dW1, db1, dW2, db2, written and accumulated
  ssa_se_apply_bwd      dy = round16(s m dz + g), dr = round16(m dz)
  ssa_maxpool3x3s2c_*   values, index bytes and gradient routing

Method of the other exact tests (exact_util): every operand is an integer or a small multiple of a power of two, chosen
so that every product and every partial sum -- in any order -- is exact in fp32 (the premise is asserted on the float64
reference in units of the finest term); a float64 host computation written out index by index, with ONE final rounding,
is then the result bit for bit.  Every operand sits in a guarded buffer, activations with pixel strides other than C."""
import ctypes
import os

import pytest
import torch

from util import ACT_DTYPE
from exact_util import (assert_bits_equal, assert_guard_intact, assert_integers, assert_premise, assert_within_bound,
                        choice, guarded, guarded_copy, ints, to_act, to_f32, ulp_err32)

pytestmark = pytest.mark.gpu

DEV = "cuda"
_EMU = bool(os.environ.get("SSA_EMU"))
NT, TILE, REDUCE_BLOCKS = 256, 32, 512

# id, (B, H, W, C, r), extra pixel stride of (y, r, z / dz, dy / dr)
CASES = [
    ("1x1c256", (2, 1, 1, 256, 16), (0, 0, 0, 0)),         # one pixel: mean = y
    ("4x8c256", (2, 4, 8, 256, 16), (8, 16, 8, 0)),        # HW = 32: four workgroups share an image's squeeze
    ("5x7c256", (2, 5, 7, 256, 16), (0, 8, 0, 16)),        # HW no power of two, ragged last split
    ("4x8c2048", (2, 4, 8, 2048, 16), (0, 0, 8, 8)),       # eight channel tiles
    ("5x7c2048", (2, 5, 7, 2048, 16), (8, 0, 0, 0)),
    ("64x64c256", (2, 64, 64, 256, 16), (0, 0, 0, 0)),     # past the workgroup target: a thread walks two pixels
    ("3x5c24r4", (1, 3, 5, 24, 4), (8, 8, 8, 8)),          # three channel groups: 85 rows, one idle thread
]
_IDS = [c[0] for c in CASES]


def _plan(B, HW, C):
    """Mirror of plan_reduce (csrc/se.hip): a workgroup = TW channel groups x RP pixel rows; grid = (nsplit, tiles, B)."""
    VC = C // 8
    TW = min(VC, TILE)
    RP, tiles = NT // TW, -(-VC // TW)
    nsplit = min(max(REDUCE_BLOCKS // (B * tiles), 1), -(-HW // RP))
    return dict(TW=TW, RP=RP, tiles=tiles, nsplit=nsplit, walks=-(-HW // (nsplit * RP)), active=RP * TW)


def test_exact_se_case_regimes():
    """The regime each case is listed for, on the mirror (not on the kernel)."""
    p = {c[0]: _plan(c[1][0], c[1][1] * c[1][2], c[1][3]) for c in CASES}
    assert p["1x1c256"]["nsplit"] == 1
    assert p["4x8c256"]["nsplit"] == 4 and p["4x8c256"]["tiles"] == 1 and p["4x8c256"]["walks"] == 1
    assert p["5x7c256"]["nsplit"] == 5 and 35 % p["5x7c256"]["RP"]
    assert p["4x8c2048"]["tiles"] == 8 and p["4x8c2048"]["nsplit"] == 4
    assert p["64x64c256"]["nsplit"] == 256 and p["64x64c256"]["walks"] == 2
    assert p["3x5c24r4"]["TW"] == 3 and p["3x5c24r4"]["active"] == 255


def _lib():
    from semseg_amd import hip_backend as hb
    from semseg_amd._lib import check
    return hb, hb.lib(), check


def _big(case):
    if _EMU and case[1][0] * case[1][1] * case[1][2] * case[1][3] > 1e6:
        pytest.skip("2 M elements: GPU only")


def _ws(L, check, B, HW, C, Cr):
    n = ctypes.c_size_t(0)
    check(L.ssa_se_plan(B, HW, C, Cr, ctypes.byref(n)), "ssa_se_plan")
    assert n.value == 4 * max(B * _plan(B, HW, C)["nsplit"] * C, B * (C + Cr))
    return guarded((n.value // 4,), torch.float32, DEV)


def _units(name, mag, unit):
    """Every partial sum is a multiple of `unit` below 2^24 units: exact in fp32."""
    assert_premise(name, mag / unit)


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_exact_se_squeeze_gate(case):
    """mean: bit for bit where HW is a power of two, within 1 ulp of float32(sum / HW) elsewhere.
    HW a power of two: W1 in {-1, 0, 1} / 64 makes W1 mean + b1 exact, so h is bit for bit from the kernel's own mean; W2
    in {-1, 0, 1} / 16 makes W2 h + b2 exact, and s is compared with the float64 sigmoid of it, the bound twice the largest
    error of ssa_sigmoid_fwd (the kernel of the scale-attention head, which predates the gate) on the same arguments,
    measured here; both numbers are printed.
    HW no power of two (the means are not dyadic, the sums round): h and s against a float64 evaluation from the kernel's
    own mean and h.  An fp32 sum of n products in ANY order is within (n + 1) 2^-24 sum |terms| of the exact one (n - 1
    additions, one rounding per product and one for the bias, first order), so |h - h64| <= (C + 2) 2^-24 (|W1| |mean| +
    |b1|) and the argument of the sigmoid is within (Cr + 2) 2^-24 (|W2| h + |b2|); the sigmoid's slope is at most 1/4, and
    its own error is bounded as above by twice ssa_sigmoid_fwd's on the correctly rounded arguments."""
    _big(case)
    hb, L, check = _lib()
    name, (B, H, W, C, r), extra = case
    HW, Cr = H * W, C // r
    pow2 = HW & (HW - 1) == 0
    y = ints((B, H, W, C), -2, 2, 900)
    w1 = choice((Cr, C), [-1.0, 0.0, 0.0, 1.0], 901) / 64
    b1 = ints((Cr,), -2, 2, 902) / 4
    w2 = choice((C, Cr), [-1.0, 0.0, 1.0], 903) / 16
    b2 = ints((C,), -8, 8, 904) / 4
    assert_integers("se y", y)
    sums = y.double().sum((1, 2))                                         # [B, C], exact
    yg = guarded_copy(y.to(ACT_DTYPE), DEV, C + extra[0])
    pg = [guarded_copy(t, DEV) for t in (w1, b1, w2, b2)]
    mg, hg, sg = guarded((B, C), torch.float32, DEV), guarded((B, Cr), torch.float32, DEV), guarded((B, C), torch.float32, DEV)
    wsg = _ws(L, check, B, HW, C, Cr)
    check(L.ssa_se_squeeze_gate(hb._p(yg.view), C + extra[0], B, HW, C, Cr, *[hb._p(g.view) for g in pg], hb._p(mg.view),
                                hb._p(hg.view), hb._p(sg.view), hb._p(wsg.view), hb._s()), "ssa_se_squeeze_gate")
    torch.cuda.synchronize()
    assert_guard_intact("se squeeze_gate %s" % name, yg, mg, hg, sg, wsg, *pg)
    mean, h, s = mg.view.cpu(), hg.view.cpu(), sg.view.cpu()
    if pow2:
        assert_bits_equal("se %s mean" % name, mean, to_f32(sums / HW))
    else:
        err = ulp_err32(mean, sums / HW)
        assert float(err.max()) <= 1.0, "se %s mean: %.3g ulp" % (name, float(err.max()))
    # h from the kernel's own mean, s from the kernel's own h (fp32 values: exact in float64)
    m64, w1d, b1d, w2d, b2d = mean.double(), w1.double(), b1.double(), w2.double(), b2.double()
    h64 = torch.relu(m64 @ w1d.t() + b1d)
    mag1 = m64.abs() @ w1d.abs().t() + b1d.abs()
    v64 = h.double() @ w2d.t() + b2d
    mag2 = h.double() @ w2d.abs().t() + b2d.abs()
    if pow2:
        unit = 1.0 / (64 * HW)
        _units("se h: sum |W1| |mean| + |b1|", mag1, unit)
        assert_bits_equal("se %s h" % name, h, to_f32(h64))
        _units("se s: sum |W2| h + |b2|", mag2, unit / 16)
        dv = torch.zeros_like(v64)
    else:
        assert_within_bound("se %s h" % name, h, h64, (C + 2) * 2.0 ** -24 * mag1)
        dv = (Cr + 2) * 2.0 ** -24 * mag2
    if C >= 256:
        assert float((h64 > 0).double().mean()) > 0.2 and float((h64 == 0).double().mean()) > 0.2
    v = v64.float().to(DEV)                                  # (exact where HW is a power of two, else correctly rounded)
    old = torch.empty_like(v)
    check(L.ssa_sigmoid_fwd(hb._p(v), hb._p(old), v.numel(), hb._s()), "ssa_sigmoid_fwd")
    torch.cuda.synchronize()
    want = 1.0 / (1.0 + torch.exp(-v64))
    e_old = float((old.cpu().double() - 1.0 / (1.0 + torch.exp(-v.cpu().double()))).abs().max())
    e_new = float((s.double() - want).abs().max())
    print("se %s: gate sigmoid error %.3g, ssa_sigmoid_fwd's on the same arguments %.3g (arguments in [%.2f, %.2f])" % (
        name, e_new, e_old, float(v64.min()), float(v64.max())))
    assert e_old > 0
    assert_within_bound("se %s s" % name, s, want, 2 * e_old + 0.25 * dv)
    assert 0.0 < float(s.min()) and float(s.max()) < 1.0


# ---- apply and the three backward entry points, s and h supplied
_REF = {}


def _bwd_case(case):
    name, (B, H, W, C, r), extra = case
    if name not in _REF:
        HW, Cr = H * W, C // r
        y, res, dz = ints((B, H, W, C), -4, 4, 910), ints((B, H, W, C), -4, 4, 911), ints((B, H, W, C), -2, 2, 912)
        s = choice((B, C), [0.25, 0.5, 0.75], 913)
        d = dict(y=y, res=res, dz=dz, s=s)
        s4 = s.double()[:, None, None, :]
        for relu in (0, 1):
            for has_r in (0, 1):
                z64 = s4 * y.double() + (res.double() if has_r else 0.0)
                z64 = z64.clamp(min=0.0) if relu else z64
                z = to_act(z64)
                m = (z.double() > 0).double() if relu else torch.ones_like(z64)
                ds64 = (m * dz.double() * y.double()).sum((1, 2))
                assert_premise("se ds", (dz.double() * y.double()).abs().sum((1, 2)))
                d[(relu, has_r)] = dict(z=z, m=m, ds=to_f32(ds64))
        # gate backward: operands of their own
        ds = ints((B, C), -2, 2, 920)
        h = torch.relu(ints((B, Cr), -2, 3, 921))
        mean = ints((B, C), -16, 16, 922) / 4
        w1, w2 = choice((Cr, C), [-1.0, 0.0, 1.0], 923), choice((C, Cr), [-1.0, 0.0, 1.0], 924)
        assert bool((h == 0).any()) and bool((h > 0).any())
        a2 = ds.double() * (s.double() * (1 - s.double()))                 # multiples of 1/16
        db2, dw2 = a2.sum(0), a2.t() @ h.double()
        dh = a2 @ w2.double()
        _units("se dh", a2.abs() @ w2.double().abs(), 1 / 16)
        a1 = dh * (h.double() > 0)
        db1, dw1 = a1.sum(0), a1.t() @ mean.double()
        _units("se dW1", a1.abs().t() @ mean.double().abs(), 1 / 64)
        dmean = a1 @ w1.double()
        _units("se dmean", a1.abs() @ w1.double().abs(), 1 / 16)
        g = (dmean / HW).float()                                           # correctly rounded: the division is IEEE
        d["gate"] = dict(ds=ds, h=h, mean=mean, w1=w1, w2=w2, g=g, dw1=to_f32(dw1), db1=to_f32(db1), dw2=to_f32(dw2),
                         db2=to_f32(db2))
        d["g_apply"] = ints((B, C), -8, 8, 925) / 8
        _REF[name] = d
    return _REF[name]


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_exact_se_apply_and_backward_passes(case):
    """ssa_se_apply, ssa_se_bwd_reduce and ssa_se_apply_bwd, with and without the ReLU and the residual: z, ds, dy and dr
    bit for bit (s in {1/4, 1/2, 3/4}: s y + r and s m dz + g are exact before the one rounding)."""
    _big(case)
    hb, L, check = _lib()
    name, (B, H, W, C, r), extra = case
    HW, Cr = H * W, C // r
    d = _bwd_case(case)
    ldy, ldr, ldz, ldd = (C + e for e in extra)
    yg, rg = guarded_copy(d["y"].to(ACT_DTYPE), DEV, ldy), guarded_copy(d["res"].to(ACT_DTYPE), DEV, ldr)
    dzg = guarded_copy(d["dz"].to(ACT_DTYPE), DEV, ldz)
    sg, gg = guarded_copy(d["s"], DEV), guarded_copy(d["g_apply"], DEV)
    s4, g4 = d["s"].double()[:, None, None, :], d["g_apply"].double()[:, None, None, :]
    for relu in (0, 1):
        for has_r in (0, 1):
            ref = d[(relu, has_r)]
            tag = "se %s relu=%d residual=%d" % (name, relu, has_r)
            zg = guarded((B, H, W, C), ACT_DTYPE, DEV, ldz)
            check(L.ssa_se_apply(hb._p(yg.view), ldy, hb._p(rg.view) if has_r else None, ldr, hb._p(sg.view), hb._p(zg.view),
                                 ldz, B, HW, C, relu, hb._s()), "ssa_se_apply")
            dsg, wsg = guarded((B, C), torch.float32, DEV), _ws(L, check, B, HW, C, Cr)
            # (without the ReLU z is not read: NULL)
            check(L.ssa_se_bwd_reduce(hb._p(dzg.view), ldz, hb._p(zg.view) if relu else None, ldz, hb._p(yg.view), ldy, B, HW,
                                      C, relu, hb._p(dsg.view), hb._p(wsg.view), hb._s()), "ssa_se_bwd_reduce")
            dyg, drg = guarded((B, H, W, C), ACT_DTYPE, DEV, ldd), guarded((B, H, W, C), ACT_DTYPE, DEV, ldd)
            check(L.ssa_se_apply_bwd(hb._p(dzg.view), ldz, hb._p(zg.view) if relu else None, ldz, hb._p(sg.view), hb._p(gg.view),
                                     B, HW, C, relu, hb._p(dyg.view), ldd, hb._p(drg.view) if has_r else None, ldd, hb._s()),
                  "ssa_se_apply_bwd")
            torch.cuda.synchronize()
            assert_bits_equal(tag + " z", zg.view.cpu(), ref["z"])
            assert_bits_equal(tag + " ds", dsg.view.cpu(), ref["ds"])
            mdz = torch.where(ref["m"] > 0, d["dz"].double(), torch.zeros(()).double())     # (a masked select: +0)
            assert_bits_equal(tag + " dy", dyg.view.cpu(), to_act(s4 * mdz + g4))
            if has_r:
                assert_bits_equal(tag + " dr", drg.view.cpu(), to_act(mdz))
            else:
                assert bool(torch.isnan(drg.view.float()).all()), tag + ": dr written though NULL"
            assert_guard_intact(tag, yg, rg, dzg, sg, gg, zg, dsg, wsg, dyg, drg)
            if relu:
                assert 0.2 < float(ref["m"].mean()) < 0.8


@pytest.mark.parametrize("case", [c for c in CASES if c[0] != "64x64c256"], ids=[i for i in _IDS if i != "64x64c256"])
def test_exact_se_gate_backward(case):
    """g, dW1, db1, dW2, db2 bit for bit with s, h and mean supplied (h with zeros; s (1 - s) in {3/16, 1/4}): written
    over NaN, and added onto integers with accumulate = 1."""
    hb, L, check = _lib()
    name, (B, H, W, C, r), extra = case
    HW, Cr = H * W, C // r
    d = _bwd_case(case)
    q = d["gate"]
    ins = [guarded_copy(t, DEV) for t in (q["ds"], d["s"], q["h"], q["mean"], q["w1"], q["w2"])]
    pre = [ints(s, -9, 9, 930 + i) for i, s in enumerate(((Cr, C), (Cr,), (C, Cr), (C,)))]
    for acc in (0, 1):
        gg = guarded((B, C), torch.float32, DEV)
        outs = [guarded(tuple(p.shape), torch.float32, DEV) for p in pre]
        if acc:
            for o, p in zip(outs, pre):
                o.view.copy_(p)
        wsg = _ws(L, check, B, HW, C, Cr)
        check(L.ssa_se_gate_bwd(*[hb._p(g.view) for g in ins], B, HW, C, Cr, hb._p(gg.view), *[hb._p(o.view) for o in outs],
                                acc, hb._p(wsg.view), hb._s()), "ssa_se_gate_bwd")
        torch.cuda.synchronize()
        tag = "se gate_bwd %s accumulate=%d" % (name, acc)
        assert_bits_equal(tag + " g", gg.view.cpu(), q["g"])
        for what, o, p in zip(("dw1", "db1", "dw2", "db2"), outs, pre):
            assert_bits_equal("%s %s" % (tag, what), o.view.cpu(), to_f32(q[what].double() + (p.double() if acc else 0.0)))
        assert_guard_intact(tag, gg, wsg, *ins, *outs)
    assert float(q["g"].abs().max()) > 0 and float(q["dw1"].abs().max()) > 0


def test_se_argument_checks():
    """Bad arguments return -1, a hidden width the gate is not built for -2, before the device is touched."""
    hb, L, check = _lib()
    t = torch.zeros(8192, dtype=ACT_DTYPE, device=DEV)
    f = torch.zeros(8192, dtype=torch.float32, device=DEV)
    p, pf = hb._p(t), hb._p(f)
    n = ctypes.c_size_t(0)
    off = lambda q, nbytes: ctypes.c_void_p(q.value + nbytes)  # noqa: E731
    assert L.ssa_se_plan(2, 12, 16, 4, ctypes.byref(n)) == 0 and n.value > 0
    assert L.ssa_se_plan(2, 12, 12, 4, ctypes.byref(n)) == -1              # C % 8
    assert L.ssa_se_plan(0, 12, 16, 4, ctypes.byref(n)) == -1              # B
    assert L.ssa_se_plan(2, 0, 16, 4, ctypes.byref(n)) == -1               # HW
    assert L.ssa_se_plan(2, 12, 16, 0, ctypes.byref(n)) == -1              # Cr
    assert L.ssa_se_plan(2, 12, 16, 32, ctypes.byref(n)) == -2             # Cr > C
    assert L.ssa_se_plan(2, 12, 16, 4, None) == -1
    sq = lambda y, ldy, C=16: L.ssa_se_squeeze_gate(y, ldy, 2, 12, C, 4, pf, pf, pf, pf, pf, pf, pf, pf, hb._s())  # noqa: E731
    assert sq(p, 8) == -1 and sq(p, 20) == -1 and sq(off(p, 2), 16) == -1 and sq(None, 16) == -1 and sq(p, 16, 12) == -1
    assert L.ssa_se_squeeze_gate(p, 16, 2, 12, 16, 4, pf, pf, pf, pf, pf, pf, pf, None, hb._s()) == -1     # no workspace
    ap = lambda y, ldy, r, ldr, z, ldz: L.ssa_se_apply(y, ldy, r, ldr, pf, z, ldz, 2, 12, 16, 1, hb._s())  # noqa: E731
    assert ap(p, 8, None, 0, p, 16) == -1 and ap(p, 16, p, 8, p, 16) == -1 and ap(p, 16, None, 0, p, 12) == -1
    assert ap(p, 16, off(p, 8), 16, p, 16) == -1 and ap(p, 16, None, 0, None, 16) == -1
    assert L.ssa_se_apply(p, 16, None, 0, None, p, 16, 2, 12, 16, 1, hb._s()) == -1                         # no gate
    assert L.ssa_se_bwd_reduce(p, 16, None, 16, p, 16, 2, 12, 16, 1, pf, pf, hb._s()) == -1                 # ReLU without z
    assert L.ssa_se_bwd_reduce(p, 8, p, 16, p, 16, 2, 12, 16, 1, pf, pf, hb._s()) == -1
    assert L.ssa_se_bwd_reduce(p, 16, p, 16, p, 16, 2, 12, 16, 1, None, pf, hb._s()) == -1
    assert L.ssa_se_gate_bwd(pf, pf, pf, pf, pf, pf, 2, 12, 16, 4, pf, pf, pf, pf, None, 0, pf, hb._s()) == -1
    assert L.ssa_se_gate_bwd(pf, pf, pf, pf, pf, pf, 2, 12, 16, 32, pf, pf, pf, pf, pf, 0, pf, hb._s()) == -2
    assert L.ssa_se_apply_bwd(p, 16, None, 16, pf, pf, 2, 12, 16, 1, p, 16, None, 0, hb._s()) == -1         # ReLU without z
    assert L.ssa_se_apply_bwd(p, 16, p, 16, pf, pf, 2, 12, 16, 1, p, 8, None, 0, hb._s()) == -1
    assert L.ssa_se_apply_bwd(p, 16, p, 16, pf, pf, 2, 12, 16, 1, p, 16, off(p, 2), 16, hb._s()) == -1


# ---- the ceil-mode pool
def _pool_ref(x):
    """float64 reference written out tap by tap: values and the first-maximum tap index of MaxPool2d(3, 2, ceil_mode=True)
    without padding (taps past the edge never win), NHWC."""
    B, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    best = torch.full((B, Ho, Wo, C), float("-inf"), dtype=x.dtype)
    arg = torch.full((B, Ho, Wo, C), -1, dtype=torch.int64)
    for kh in range(3):
        ny = min(Ho, (H - kh + 1) // 2)                       # outputs oy with 2 oy + kh < H
        for kw in range(3):
            nx = min(Wo, (W - kw + 1) // 2)
            v = x[:, kh:kh + 2 * ny:2, kw:kw + 2 * nx:2][:, :ny, :nx]
            b, a = best[:, :ny, :nx], arg[:, :ny, :nx]
            win = v > b
            b[win] = v[win]
            a[win] = kh * 3 + kw
    return best, arg


def _pool_route(dy, arg, H, W):
    B, Ho, Wo, C = dy.shape
    dx = torch.zeros((B, H, W, C), dtype=dy.dtype)
    for kh in range(3):
        for kw in range(3):
            ny, nx = min(Ho, (H - kh + 1) // 2), min(Wo, (W - kw + 1) // 2)
            if ny <= 0 or nx <= 0:
                continue
            sel = (arg[:, :ny, :nx] == kh * 3 + kw).to(dy.dtype)
            dx[:, kh:kh + 2 * ny:2, kw:kw + 2 * nx:2][:, :ny, :nx] += dy[:, :ny, :nx] * sel
    return dx


POOL = [(2, 16, h, w) for h in (2, 5, 6, 9) for w in (2, 5, 6, 9)] + [(1, 8, 4100, 4098)]


@pytest.mark.parametrize("Bn,C,H,W", POOL, ids=["%dx%d" % (h, w) for _, _, h, w in POOL])
def test_exact_pool_ceil(Bn, C, H, W):
    """Values, index bytes and the gradient bit for bit on post-ReLU integers (half of them zero: ties in nearly every
    window), the host reference anchored to F.max_pool2d(ceil_mode=True) and its autograd; the input a channel slice.
    4100 x 4098: 4.2 M output channel groups, past the 16384 x 256 grid-stride cap of both kernels."""
    if _EMU and H * W > 1e6:
        pytest.skip("134 M elements: GPU only")
    hb, L, check = _lib()
    F = torch.nn.functional
    big = H * W > 1e6
    if big:
        assert Bn * (H // 2) * (W // 2) * (C // 8) > 16384 * 256
    Ho, Wo = H // 2, W // 2
    if big:       # torch alone is the reference (fp32 holds the integers; int8 draws spare a gigabyte of int64)
        gen = torch.Generator().manual_seed(940)
        x = torch.randint(-3, 4, (Bn, H, W, C), generator=gen, dtype=torch.int8).clamp_(min=0).float()
        dy = torch.randint(-16, 17, (Bn, Ho, Wo, C), generator=gen, dtype=torch.int8).float()
    else:
        x = torch.relu(ints((Bn, H, W, C), -3, 3, 940)).double()
        dy = ints((Bn, Ho, Wo, C), -16, 16, 941).double()
    xr = x.permute(0, 3, 1, 2).requires_grad_(True)
    yr, ind = F.max_pool2d(xr, 3, stride=2, ceil_mode=True, return_indices=True)
    assert tuple(yr.shape[2:]) == (Ho, Wo)
    yr.backward(dy.permute(0, 3, 1, 2))
    oy, ox = torch.arange(Ho).view(1, 1, Ho, 1), torch.arange(Wo).view(1, 1, 1, Wo)
    arg = ((ind // W - 2 * oy) * 3 + (ind % W - 2 * ox)).permute(0, 2, 3, 1)
    y_ref, dx_ref = yr.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1)
    assert int(arg.min()) == 0 and int(arg.max()) <= 8
    if not big:
        y_host, arg_host = _pool_ref(x)
        assert torch.equal(y_host, y_ref) and torch.equal(arg_host, arg), "the host reference picks unlike torch"
        assert torch.equal(_pool_route(dy, arg_host, H, W), dx_ref), "the host reference routes unlike torch"
        assert float((x == 0).double().mean()) > 0.4
    xg = guarded_copy(x.to(ACT_DTYPE), DEV, C + 8)
    yg, ig = guarded((Bn, Ho, Wo, C), ACT_DTYPE, DEV), guarded((Bn, Ho, Wo, C), torch.uint8, DEV)
    dyg, dxg = guarded_copy(dy.to(ACT_DTYPE), DEV), guarded((Bn, H, W, C), ACT_DTYPE, DEV)
    check(L.ssa_maxpool3x3s2c_fwd(hb._p(xg.view), C + 8, Bn, H, W, C, hb._p(yg.view), hb._p(ig.view), Ho, Wo, hb._s()),
          "ssa_maxpool3x3s2c_fwd")
    check(L.ssa_maxpool3x3s2c_bwd(hb._p(dyg.view), hb._p(ig.view), Bn, Ho, Wo, C, hb._p(dxg.view), H, W, hb._s()),
          "ssa_maxpool3x3s2c_bwd")
    torch.cuda.synchronize()
    assert_bits_equal("pool_ceil y", yg.view.cpu(), y_ref.float().to(ACT_DTYPE))
    assert_bits_equal("pool_ceil idx", ig.view.cpu(), arg.to(torch.uint8))
    assert_bits_equal("pool_ceil dx", dxg.view.cpu(), dx_ref.float().to(ACT_DTYPE))
    assert_guard_intact("pool_ceil", xg, yg, ig, dyg, dxg)
    if not big:
        xd = xg.view.detach().requires_grad_(True)
        yd = hb.MaxPool3x3s2CeilFn.apply(xd)
        yd.backward(dyg.view)
        torch.cuda.synchronize()
        assert_bits_equal("MaxPool3x3s2CeilFn y", yd.detach().cpu(), y_ref.float().to(ACT_DTYPE))
        assert_bits_equal("MaxPool3x3s2CeilFn dx", xd.grad.cpu(), dx_ref.float().to(ACT_DTYPE))


def test_pool_ceil_argument_checks():
    hb, L, check = _lib()
    t = torch.zeros(8192, dtype=ACT_DTYPE, device=DEV)
    b = torch.zeros(8192, dtype=torch.uint8, device=DEV)
    p, pb = hb._p(t), hb._p(b)
    fwd = lambda ldx, H, W, C, Ho, Wo, x=p: L.ssa_maxpool3x3s2c_fwd(x, ldx, 1, H, W, C, p, pb, Ho, Wo, hb._s())  # noqa: E731
    assert fwd(8, 1, 4, 8, 0, 2) == -1 and fwd(8, 5, 6, 8, 3, 3) == -1 and fwd(8, 5, 6, 8, 2, 2) == -1      # H < 2, Ho, Wo
    assert fwd(8, 5, 6, 12, 2, 3) == -1 and fwd(4, 5, 6, 8, 2, 3) == -1 and fwd(12, 5, 6, 8, 2, 3) == -1    # C % 8, ldx
    assert fwd(8, 5, 6, 8, 2, 3, ctypes.c_void_p(p.value + 2)) == -1 and fwd(8, 5, 6, 8, 2, 3, None) == -1
    assert L.ssa_maxpool3x3s2c_bwd(p, pb, 1, 3, 3, 8, p, 5, 6, hb._s()) == -1                               # Ho
    assert L.ssa_maxpool3x3s2c_bwd(p, None, 1, 2, 3, 8, p, 5, 6, hb._s()) == -1
