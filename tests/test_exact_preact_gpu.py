"""Exact tests of the two passes of a pre-activation block (csrc/bn.hip) through the C ABI:

  ssa_add_bn_stats      s = round16(a + b) stored once, sum s and sum s^2 over the values as stored
  ssa_bn_bwd_apply_add  dx = round16((A g + (Bx x + D)) + dadd), the mask-from-x form of ssa_bn_bwd_apply

Method of the other exact tests (exact_util): integer / dyadic operands, so that every fp32 step of the kernel is exact and
a float64 host computation with ONE final rounding is the result bit for bit; every operand in a guarded buffer.  Cases:
the smallest at which each regime of the launch can go wrong (see CASES)."""
import os

import pytest
import torch

from util import ACT_DTYPE
from exact_util import (assert_bits_equal, assert_guard_intact, assert_integers, assert_premise, choice, guarded,
                        guarded_copy, ints, pow2, split_replicas, to_act, to_f32)

pytestmark = pytest.mark.gpu

DEV = "cuda"
_EMU = bool(os.environ.get("SSA_EMU"))
_BN_TUNING = ("SSA_BN_WIDE_CHUNKS", "SSA_BN_ROWS_APPLY", "SSA_BN_ROWS_BWD", "SSA_BN_ROWS_REDUCE", "SSA_BN_REDUCE_BLOCKS")

# id, P, C, images, extra pixel stride of every operand
CASES = [
    ("p1c8", 1, 8, 1, 0),              # one pixel, one channel group: 255 threads have no valid row
    ("p300c24", 300, 24, 3, 0),        # VC = 3: 255 active threads (one idle), the only chunk ragged
    ("p5000c128", 5000, 128, 2, 8),    # 40 / 79 workgroups, the last one partial; every leading dimension C + 8
    ("p37c2048", 37, 2048, 1, 0),      # RP = 1: one row of threads per pixel
    ("p16411c1032", 16411, 1032, 1, 0),  # past both workgroup caps: a workgroup walks 2 (statistics) / 5 (backward) chunks
]
_IDS = [c[0] for c in CASES]


def _plan(P, C, rows, max_blocks, chunks=1):
    """Mirror of plan_grid (csrc/bn.hip)."""
    VC = C // 8
    RP = ((256 // VC) * VC) // VC
    chunk = RP * rows
    ppb, blocks = chunk, -(-P // chunk)
    if chunks > 1 and blocks > 1024:
        max_blocks = min(max_blocks, max(1024, -(-blocks // chunks)))
    if blocks > max_blocks:
        ppb = -(-(-(-P // max_blocks)) // chunk) * chunk
        blocks = -(-P // ppb)
    return dict(VC=VC, RP=RP, active=RP * VC, chunk=chunk, ppb=ppb, blocks=max(blocks, 1), chunks_per_wg=ppb // chunk,
                last=P - (max(blocks, 1) - 1) * ppb)


def _stats_plan(P, C):
    return _plan(P, C, 8, 2048)


def _bwd_plan(P, C):
    return _plan(P, C, 4, 16384, 6 if C >= 256 else 1)


def test_exact_preact_case_regimes():
    """The regime each case is listed for, on the mirror (not on the kernel)."""
    s = {c[0]: _stats_plan(c[1], c[2]) for c in CASES}
    b = {c[0]: _bwd_plan(c[1], c[2]) for c in CASES}
    assert s["p1c8"]["blocks"] == 1 and s["p1c8"]["RP"] == 256
    assert s["p300c24"]["active"] == 255 and s["p300c24"]["blocks"] == 1 and 300 % s["p300c24"]["RP"]
    assert s["p5000c128"]["blocks"] == 40 and s["p5000c128"]["last"] < s["p5000c128"]["chunk"]
    assert b["p5000c128"]["blocks"] == 79 and b["p5000c128"]["last"] < b["p5000c128"]["chunk"]
    assert s["p37c2048"]["RP"] == 1 and b["p37c2048"]["RP"] == 1
    assert s["p16411c1032"]["chunks_per_wg"] == 2 and s["p16411c1032"]["blocks"] <= 2048
    assert b["p16411c1032"]["chunks_per_wg"] == 5 and b["p16411c1032"]["blocks"] <= 1024


def _guard():
    on = [k for k in _BN_TUNING if k in os.environ]
    if on:
        pytest.skip("%s set: the grid mirror describes the default launch" % ", ".join(on))
    from semseg_amd import hip_backend as hb
    from semseg_amd._lib import check
    return hb, hb.lib(), check


def _big(case):
    if _EMU and case[1] * case[2] > 4e6:
        pytest.skip("17 M elements: GPU only")


def _rows_equal(tag, got, want):
    for row in (0, 1):
        assert torch.equal(got[row], want[row]), "%s row %d: %d channels differ; first %d" % (
            tag, row, int((got[row] != want[row]).sum()), int((got[row] != want[row]).nonzero()[0]))


# ---- ssa_add_bn_stats
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_exact_add_bn_stats(case):
    """s bit for bit and both rows of the sums equal to the int64 sums of s: twice into one zeroed buffer (zero_sums = 0,
    accumulation) and once over NaN (zero_sums = 1)."""
    _big(case)
    hb, L, check = _guard()
    name, P, C, _, extra = case
    a, b = ints((P, C), -2, 2, 500), ints((P, C), -2, 2, 501)
    assert_integers("add_bn_stats operands", a, b)
    si = (a + b).long()
    want = torch.stack([si.sum(0), (si * si).sum(0)]).double()
    assert_premise("sum of s^2 over the pixels", want[1])          # every fp32 partial sum of a workgroup is then exact
    ld = C + extra
    ag, bg = guarded_copy(a.to(ACT_DTYPE), DEV, ld), guarded_copy(b.to(ACT_DTYPE), DEV, ld)
    acc = guarded((2, C), torch.float64, DEV)
    acc.view.zero_()
    fresh = guarded((2, C), torch.float64, DEV)
    outs = [guarded((P, C), ACT_DTYPE, DEV, ld) for _ in range(3)]
    for i, (sums, zero) in enumerate(((acc, 0), (acc, 0), (fresh, 1))):
        check(L.ssa_add_bn_stats(hb._p(ag.view), ld, hb._p(bg.view), ld, hb._p(outs[i].view), ld, P, C, hb._p(sums.view),
                                 zero, hb._s()), "ssa_add_bn_stats")
    torch.cuda.synchronize()
    ref = to_act((a + b).double())
    for i in range(3):
        assert_bits_equal("add_bn_stats %s s (call %d)" % (name, i), outs[i].view.cpu(), ref)
    _rows_equal("add_bn_stats %s zero_sums=1" % name, fresh.view.cpu(), want)
    _rows_equal("add_bn_stats %s accumulated twice" % name, acc.view.cpu(), 2 * want)
    assert_guard_intact("add_bn_stats %s" % name, ag, bg, acc, fresh, *outs)


def test_add_bn_stats_random_operands():
    """Real operands: s equals ssa_sum_act's output (and one rounding of the fp32 sum) bit for bit, and the sums lie within
    gamma_n * sum |terms| of the float64 sums of the STORED s, n = the longest fp32 chain a value passes through: the
    thread's rows (chunks x 8), the workgroup's tree over RP threads in two chains (RP / 2 + 1), plus the rounding of the
    square."""
    hb, L, check = _guard()
    P, C = 3001, 72
    g = torch.Generator().manual_seed(510)
    a = (torch.randn(P, C, generator=g) * 3).to(ACT_DTYPE)
    b = (torch.randn(P, C, generator=g) * 3 + 0.5).to(ACT_DTYPE)
    ag, bg = guarded_copy(a, DEV, C + 16), guarded_copy(b, DEV, C + 8)
    sg = guarded((P, C), ACT_DTYPE, DEV, C + 24)
    sums = guarded((2, C), torch.float64, DEV)
    check(L.ssa_add_bn_stats(hb._p(ag.view), C + 16, hb._p(bg.view), C + 8, hb._p(sg.view), C + 24, P, C, hb._p(sums.view), 1,
                             hb._s()), "ssa_add_bn_stats")
    ad, bd = a.to(DEV).contiguous(), b.to(DEV).contiguous()
    z = torch.empty_like(ad)
    check(L.ssa_sum_act(hb._p(ad), hb._p(bd), None, None, hb._p(z), z.numel(), 0, hb._s()), "ssa_sum_act")
    torch.cuda.synchronize()
    s = sg.view.cpu()
    assert_bits_equal("add_bn_stats s against ssa_sum_act", s, z.cpu())
    assert_bits_equal("add_bn_stats s against one rounding", s, (a.float() + b.float()).to(ACT_DTYPE))
    assert int((s.double() != a.double() + b.double()).sum()) > P * C // 4        # the rounding decides bits
    p = _stats_plan(P, C)
    n = p["chunks_per_wg"] * 8 + p["RP"] // 2 + 1 + 1
    u = 2.0 ** -24
    gamma = n * u / (1 - n * u)
    sd = s.double()
    want = torch.stack([sd.sum(0), (sd * sd).sum(0)])
    mag = torch.stack([sd.abs().sum(0), (sd * sd).sum(0)])
    got = sums.view.cpu()
    err = (got - want).abs()
    print("add_bn_stats random: n = %d, worst error / bound = %.3g" % (n, float((err / (gamma * mag)).max())))
    assert bool((err <= gamma * mag).all()), "sums off by up to %.3g of the bound" % float((err / (gamma * mag)).max())
    assert_guard_intact("add_bn_stats random", ag, bg, sg, sums)


def test_add_bn_stats_argument_checks():
    """The argument checks of ssa_bn_stats: C % 8, leading dimensions % 8 (and >= C), 16-byte alignment, null pointers."""
    hb, L, check = _guard()
    t = torch.zeros(64 * 16 + 8, dtype=ACT_DTYPE, device=DEV)
    sums = torch.zeros(32, dtype=torch.float64, device=DEV)
    p, ps = t.data_ptr(), hb._p(sums)
    assert p % 16 == 0
    ok = lambda *a: L.ssa_add_bn_stats(*a, hb._s())  # noqa: E731
    assert ok(p, 16, p, 16, p, 16, 4, 12, ps, 0) == -1
    assert ok(p, 20, p, 16, p, 16, 4, 16, ps, 0) == -1
    assert ok(p, 16, p, 16, p, 12, 4, 16, ps, 0) == -1
    assert ok(p, 8, p, 16, p, 16, 4, 16, ps, 0) == -1
    assert ok(p + 2, 16, p, 16, p, 16, 4, 16, ps, 0) == -1
    assert ok(p, 16, p, 16, p + 8, 16, 4, 16, ps, 0) == -1
    assert ok(None, 16, p, 16, p, 16, 4, 16, ps, 0) == -1
    assert ok(p, 16, p, 16, p, 16, 4, 16, None, 0) == -1
    assert ok(p, 16, p, 16, p, 16, 0, 16, ps, 0) == -1


# ---- ssa_bn_bwd_apply_add
_POST = [0.0, 0.5, 1.0, 2.0]


def _bwd_operands(P, C, B, seed):
    """The operands of test_exact_bn_bwd_apply (tests/test_kernels_gpu.py): dz, x integers in [-4, 4], integer mean, invstd
    a power of two, post in {0, 0.5, 1, 2}, the mask recomputed as mask_scale * x + mask_shift > 0 with many pre-activations
    exactly zero; dadd integers in [-4, 4]."""
    assert P % B == 0
    o = dict(P=P, C=C, hw=P // B)
    o["x"], o["dz"], o["dadd"] = ints((P, C), -4, 4, seed), ints((P, C), -4, 4, seed + 1), ints((P, C), -4, 4, seed + 7)
    o["mean"], o["invstd"] = ints((C,), -2, 2, seed + 2), pow2((C,), -2, 1, seed + 3)
    o["post"] = choice((B, C), _POST, seed + 4)
    o["msc"], o["msh"] = pow2((C,), -1, 1, seed + 5, signed=True), ints((C,), -3, 3, seed + 6)
    assert_integers("bn_bwd_apply_add operands", o["x"], o["dz"], o["dadd"], o["mean"], o["msh"])
    pre = o["x"] * o["msc"] + o["msh"]
    if P * C >= 2400:
        assert int((pre == 0).sum()) > pre.numel() // 50, "too few pre-activations are exactly zero"
    o["pre_pos"] = pre > 0
    return o


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_exact_bn_bwd_apply_add(case):
    """dx = (A g + (Bx x + D)) + dadd bit for bit, g = post dz where mask_scale x + mask_shift > 0: with and without post,
    dgamma / dbeta written over NaN and added onto a pre-fill, one and ssa_bn_stat_replicas() replicas, gamma given or
    NULL; and with dadd all zeros (-0.0, the additive identity: dx holds -0.0 where g, x and D cancel) the pass equals
    ssa_bn_bwd_apply bit for bit."""
    _big(case)
    hb, L, check = _guard()
    name, P, C, B, extra = case
    o = _bwd_operands(P, C, B, 540)
    count = 1024.0
    c = torch.stack([ints((C,), -12, 12, 547), ints((C,), -12, 12, 548)]).double()
    gamma = choice((C,), [1.0, -1.0, 2.0, -2.0, 0.5], 549)
    cfgs = [dict(post=True, pg="write", nrep=1, gamma=True, zero=False),
            dict(post=False, pg="acc", nrep=hb.stat_replicas(), gamma=True, zero=False),
            dict(post=True, pg="acc", nrep=hb.stat_replicas(), gamma=False, zero=True),
            dict(post=False, pg="write", nrep=1, gamma=True, zero=True)]
    if P * C > 4e6:
        cfgs = cfgs[1:3]
    ld = C + extra
    rounded = 0
    for k, cf in enumerate(cfgs):
        g = o["dz"] * o["post"].repeat_interleave(o["hw"], 0) if cf["post"] else o["dz"].clone()
        g = torch.where(o["pre_pos"], g, torch.zeros(()))
        # (the zero that leaves EVERY value as it is, -0.0 included, is IEEE's additive identity -0.0: -0.0 + +0.0 is +0.0)
        dadd = torch.full_like(o["dadd"], -0.0) if cf["zero"] else o["dadd"]
        gd, xd, mu, inv = g.double(), o["x"].double(), o["mean"].double(), o["invstd"].double()
        A = (gamma.double() if cf["gamma"] else 1.0) * inv
        Bx = -A * c[1] * inv
        D = A * (c[1] * inv * mu - c[0])
        dx64 = (A * gd + (Bx * xd + D)) + dadd.double()
        dx = to_act(dx64)                                           # (asserts that fp32 holds the sum exactly)
        rounded += int((dx.double() != dx64).sum())
        bufs = dict(x=guarded_copy(o["x"].to(ACT_DTYPE), DEV, ld), dz=guarded_copy(o["dz"].to(ACT_DTYPE), DEV, ld),
                    dadd=guarded_copy(dadd.to(ACT_DTYPE), DEV, ld), mean=guarded_copy(o["mean"], DEV),
                    invstd=guarded_copy(o["invstd"], DEV), msc=guarded_copy(o["msc"], DEV), msh=guarded_copy(o["msh"], DEV),
                    sums=guarded_copy(split_replicas(c * count, cf["nrep"], 550 + k), DEV))
        post = guarded_copy(o["post"], DEV) if cf["post"] else None
        gam = guarded_copy(gamma, DEV) if cf["gamma"] else None
        pre = ints((2, C), -9, 9, 560 + k)

        def run(fn, extra_args, what):
            dxg = guarded((P, C), ACT_DTYPE, DEV, ld)
            pgb = guarded((2, C), torch.float32, DEV)
            if cf["pg"] == "acc":
                pgb.view.copy_(pre)
            check(fn(hb._p(bufs["x"].view), ld, hb._p(bufs["dz"].view), ld, None, 0, hb._p(dxg.view), ld, None, 0, P, C,
                     hb._p(gam.view) if gam else None, hb._p(bufs["mean"].view), hb._p(bufs["invstd"].view),
                     hb._p(bufs["sums"].view), cf["nrep"], count, 1, hb._p(post.view) if post else None, o["hw"],
                     hb._p(pgb.view[0]), hb._p(pgb.view[1]), 0.5, hb._p(bufs["msc"].view), hb._p(bufs["msh"].view),
                     int(cf["pg"] == "acc"), None, *extra_args, hb._s()), what)
            return dxg, pgb
        dxg, pgb = run(L.ssa_bn_bwd_apply_add, (hb._p(bufs["dadd"].view), ld), "ssa_bn_bwd_apply_add")
        plain = run(L.ssa_bn_bwd_apply, (), "ssa_bn_bwd_apply") if cf["zero"] else None
        torch.cuda.synchronize()
        tag = "bn_bwd_apply_add %s %s" % (name, " ".join("%s=%s" % kv for kv in sorted(cf.items())))
        assert_bits_equal(tag + " dx", dxg.view.cpu(), dx)
        wantpg = torch.stack([c[1], c[0]]) * count * 0.5 + (pre.double() if cf["pg"] == "acc" else 0.0)
        assert_bits_equal(tag + " dgamma, dbeta", pgb.view.cpu(), to_f32(wantpg))
        if plain is not None:
            assert_bits_equal(tag + " dx against ssa_bn_bwd_apply", dxg.view.cpu(), plain[0].view.cpu())
            assert_bits_equal(tag + " dgamma, dbeta against ssa_bn_bwd_apply", pgb.view.cpu(), plain[1].view.cpu())
            assert_guard_intact(tag, *plain)
        assert_guard_intact(tag, dxg, pgb, *[v for v in list(bufs.values()) + [post, gam] if v is not None])
    if ACT_DTYPE == torch.bfloat16 and C >= 128 and P >= 37:
        assert rounded > 0, "no dx of %s needs rounding" % name


def test_bn_bwd_apply_add_unbuilt_forms():
    """Only the mask-from-x form is built: without a ReLU, or without mask_scale / mask_shift, the entry point answers
    SSA_EUNSUPPORTED (-2), and a null dadd SSA_EINVAL (-1) -- before any launch."""
    hb, L, check = _guard()
    t = torch.zeros(64, dtype=ACT_DTYPE, device=DEV)
    f = torch.zeros(64, dtype=torch.float32, device=DEV)
    d = torch.zeros(64, dtype=torch.float64, device=DEV)
    p, pf, pd = hb._p(t), hb._p(f), hb._p(d)

    def call(relu, msc, dadd):
        return L.ssa_bn_bwd_apply_add(p, 8, p, 8, p, 8, p, 8, None, 0, 4, 8, pf, pf, pf, pd, 1, 4.0, relu, None, 4, None, None,
                                      1.0, msc, msc, 0, None, dadd, 8, hb._s())
    assert call(0, pf, p) == -2
    assert call(1, None, p) == -2
    assert call(1, pf, None) == -1
