"""Exact tests of the OCR head kernels: the fused object attention (csrc/ocr_attn.hip), the HW softmax, the per-pixel
softmax and the pack kernel (csrc/ocr.hip) through the C ABI with every operand in a guarded buffer, and the Python
composition in OcrAttnFn / OcrGatherFn through autograd (which adds the weight-gradient kernel's pixel reductions).

Method of the other exact tests (exact_util): tests/ocr_cases.py builds inputs whose softmax is EXACTLY 1/m on a group of
m regions (attention) or pixels (gather) and 0 elsewhere, by a derived margin, with integer operands around it; every
fp32 partial sum of the kernels is then exact and a float64 reference with one final rounding is the result bit for bit.
A region swapped in the accumulator-row permutation, a padding region that leaks mass, a wrong cross-lane exchange or a
wrong row maximum changes whole units.  Output buffers start as a NaN pattern: an unwritten element fails, and so does a
write past the last pixel (assert_guard_intact)."""
import os

import pytest
import torch

import ocr_cases as OC
from exact_util import (assert_bits_equal, assert_guard_intact, assert_within_bound, guarded, guarded_copy, ints, to_act,
                        to_f32)
from util import ACT_DTYPE

pytestmark = pytest.mark.gpu

DEV = "cuda"
_EMU = bool(os.environ.get("SSA_EMU"))
D = OC.D
SSA_EUNSUPPORTED = -2                 # include/semseg_hip.h

_CACHE = {}


def _cached(kind, fn, *args):
    key = (kind,) + args
    if key not in _CACHE:
        _CACHE[key] = fn(*args)
    return _CACHE[key]


def _tie(K, P, seed=0):
    return _cached("tie", OC.tie_case, K, P, seed)


def _gather(K, HW, C, seed=0):
    return _cached("gather", OC.gather_case, K, HW, C, seed)


def _lib():
    from semseg_amd import hip_backend as hb
    from semseg_amd._lib import check
    return hb, hb.lib(), check


def _act(t):
    return t.to(ACT_DTYPE)


# ---------------------------------------------------------------- the fused attention through the C ABI
def _rows(t, tail):
    """A [P, 256] input in a guarded buffer.  tail: one more, finite row behind pixel P - 1 (a copy of pixel 0).  A kernel that
    took pixel P for a valid one would compute from a NaN guard row there and store NaNs -- which a NaN guard pattern can
    hide (the emulation's arithmetic keeps a NaN's payload); with a finite row it stores finite values into the guard
    of its output."""
    return torch.cat([t, t[:1]]) if tail else t


def _attn_fwd(c, extra=(0, 0, 0, 0), tail=False):
    hb, L, check = _lib()
    P, K = c["P"], c["K"]
    qg = guarded_copy(_rows(_act(c["q"]), tail), DEV, D + extra[0])
    kg, vg = guarded_copy(_act(c["k"]), DEV), guarded_copy(_act(c["v"]), DEV)
    og = guarded((P, D), ACT_DTYPE, DEV, D + extra[1])
    check(L.ssa_ocr_attn_fwd(hb._p(qg.view), D + extra[0], hb._p(kg.view), hb._p(vg.view), P, K, D, OC.SCALE, hb._p(og.view),
                             D + extra[1], hb._s()), "ssa_ocr_attn_fwd")
    torch.cuda.synchronize()
    return og, (qg, kg, vg, og)


def _attn_bwd(c, extra=(0, 0, 0, 0), tail=False):
    hb, L, check = _lib()
    P, K, Kp = c["P"], c["K"], c["Kp"]
    qg = guarded_copy(_rows(_act(c["q"]), tail), DEV, D + extra[0])
    kg, vg = guarded_copy(_act(c["k"]), DEV), guarded_copy(_act(c["v"]), DEV)
    dog = guarded_copy(_rows(_act(c["dout"]), tail), DEV, D + extra[2])
    dqg = guarded((P, D), ACT_DTYPE, DEV, D + extra[3])
    pg, dsg = guarded((P, Kp), ACT_DTYPE, DEV), guarded((P, Kp), ACT_DTYPE, DEV)
    check(L.ssa_ocr_attn_bwd(hb._p(qg.view), D + extra[0], hb._p(kg.view), hb._p(vg.view), hb._p(dog.view), D + extra[2], P, K,
                             D, OC.SCALE, hb._p(dqg.view), D + extra[3], hb._p(pg.view), hb._p(dsg.view), hb._s()),
          "ssa_ocr_attn_bwd")
    torch.cuda.synchronize()
    return dqg, pg, dsg, (qg, kg, vg, dog, dqg, pg, dsg)


@pytest.mark.parametrize("K,P", OC.TIE_KP, ids=["k%d-p%d" % kp for kp in OC.TIE_KP])
def test_exact_ocr_attn_tie(K, P):
    """ssa_ocr_attn_fwd / _bwd on the tie cases: out, dq and the stored probs and dsim matrices (padding columns
    included) bit for bit; the last, ragged 128-pixel tile writes nothing past pixel P - 1 (q and dout carry a finite row
    there, see _rows); four of the cases run with q, out, dout and dq as channel slices of wider rows, a different extra
    stride each."""
    c = _tie(K, P)
    extra = OC.TIE_LD.get((K, P), (0, 0, 0, 0))
    tag = "attn tie K=%d P=%d" % (K, P)
    og, gs = _attn_fwd(c, extra, tail=True)
    assert_bits_equal(tag + " out", og.view.cpu(), c["out"])
    assert_guard_intact(tag + " fwd", *gs)
    dqg, pg, dsg, gs = _attn_bwd(c, extra, tail=True)
    assert_bits_equal(tag + " probs", pg.view.cpu(), c["probs"])
    assert_bits_equal(tag + " dsim", dsg.view.cpu(), c["dsim"])
    assert_bits_equal(tag + " dq", dqg.view.cpu(), c["dq"])
    assert_guard_intact(tag + " bwd", *gs)


def test_exact_ocr_attn_one_region_real_q():
    """K = 1 with a real-valued q: probs = 1 whatever the logit (negative for half the pixels, down to -150 and below, with
    31 padding regions beside it), so out = v[0] bit for bit and dq = +0.0 everywhere."""
    c = _cached("k1real", OC.k1_real_case, 129)
    og, gs = _attn_fwd(c)
    assert_bits_equal("attn K=1 out", og.view.cpu(), c["out"])
    assert_guard_intact("attn K=1 fwd", *gs)
    dqg, pg, dsg, gs = _attn_bwd(c)
    one = torch.zeros(c["P"], 32, dtype=ACT_DTYPE)
    one[:, 0] = 1
    assert_bits_equal("attn K=1 probs", pg.view.cpu(), one)
    assert_bits_equal("attn K=1 dq", dqg.view.cpu(), c["dq"])
    assert float(dsg.view.float().abs().max()) == 0.0
    assert_guard_intact("attn K=1 bwd", *gs)


def test_exact_ocr_attn_unsupported():
    """More than 96 regions or another channel count: refused, the output untouched."""
    hb, L, check = _lib()
    assert L.ssa_ocr_attn_supported(97, 256) == 0 and L.ssa_ocr_attn_supported(19, 128) == 0
    assert L.ssa_ocr_attn_supported(96, 256) == 1 and L.ssa_ocr_attn_supported(1, 256) == 1
    c = _tie(97, 33)
    qg, kg, vg = (guarded_copy(_act(c[n]), DEV) for n in ("q", "k", "v"))
    og = guarded((33, D), ACT_DTYPE, DEV)
    rc = L.ssa_ocr_attn_fwd(hb._p(qg.view), D, hb._p(kg.view), hb._p(vg.view), 33, 97, D, OC.SCALE, hb._p(og.view), D, hb._s())
    torch.cuda.synchronize()
    assert rc == SSA_EUNSUPPORTED
    itype = torch.int16
    assert bool((og.buf.view(itype) == torch.tensor(og.pattern, dtype=itype, device=og.buf.device)).all()), \
        "a refused call wrote to its output"


@pytest.mark.parametrize("K", [19, 65, 96])
def test_exact_ocr_attn_bounded(K):
    """Gaussian operands, one case per region-block count: the stored probabilities within one storage step of
    round16(p_ref), padding columns exactly 0, out within the derived bound of ocr_cases.bounded_case."""
    c = _cached("bounded", OC.bounded_case, K, 300)
    og, gs = _attn_fwd(c)
    dqg, pg, dsg, gs2 = _attn_bwd(c)
    got = pg.view.cpu()
    assert_within_bound("attn bounded K=%d probs" % K, got, c["probs"], c["probs_bound"])
    assert_bits_equal("attn bounded K=%d padding" % K, got[:, K:], torch.zeros(c["P"], c["Kp"] - K, dtype=ACT_DTYPE))
    err = assert_within_bound("attn bounded K=%d out" % K, og.view.cpu(), c["out"], c["out_bound"])
    print("K=%d: largest out error / bound = %.3f" % (K, float((err / c["out_bound"]).max())))
    assert_guard_intact("attn bounded K=%d" % K, *(gs + gs2))


@pytest.mark.skipif(_EMU, reason="131,205 pixels: GPU only")
def test_exact_ocr_attn_grid_stride():
    """P = 131072 + 133 pixels = 1026 tiles on 1024 workgroups: two workgroups take a second tile.  Tie inputs, out bit for
    bit; operands and reference are built per group on the device."""
    hb, L, check = _lib()
    K, P = OC.GRID_STRIDE_KP
    tiles, gx = OC.attn_tiles(P)
    assert tiles == 1026 and gx == 1024
    c = _cached("tie-fwd", OC.tie_case, K, P, 0, False)
    pg = c["pixel_group"].to(DEV)
    qg = guarded((P, D), ACT_DTYPE, DEV)
    qg.view.copy_(_act(8 * c["key"]).to(DEV)[pg])
    kg, vg = guarded_copy(_act(c["k"]), DEV), guarded_copy(_act(c["v"]), DEV)
    og = guarded((P, D), ACT_DTYPE, DEV)
    check(L.ssa_ocr_attn_fwd(hb._p(qg.view), D, hb._p(kg.view), hb._p(vg.view), P, K, D, OC.SCALE, hb._p(og.view), D, hb._s()),
          "ssa_ocr_attn_fwd")
    torch.cuda.synchronize()
    want = c["outG"].to(DEV)[pg]
    bad = og.view.view(torch.int16) != want.view(torch.int16)
    n = int(bad.sum())
    if n:
        p, ch = (int(i) for i in bad.nonzero()[0])
        raise AssertionError("attn grid stride: %d of %d elements differ; first at pixel %d (tile %d) channel %d: got %r ref %r"
                             % (n, bad.numel(), p, p // 128, ch, float(og.view[p, ch]), float(want[p, ch])))
    assert_guard_intact("attn grid stride", qg, kg, vg, og)


# ---------------------------------------------------------------- the three-launch form's softmax and the pack kernel
@pytest.mark.parametrize("K,P", [(1, 129), (19, 300), (97, 33)])
def test_exact_ocr_lastdim_softmax(K, P):
    """ssa_softmax_lastdim_fwd / _bwd on the tie cases' sim (fp32, rows of K + 3): probs and dsim bit for bit, padding
    columns +0.0."""
    hb, L, check = _lib()
    c = _tie(K, P)
    Kp = c["Kp"]
    sg = guarded_copy(c["sim"], DEV, K + 3)
    dpg = guarded_copy(c["dprobs"], DEV, K + 5)
    pg, dsg = guarded((P, Kp), ACT_DTYPE, DEV), guarded((P, Kp), ACT_DTYPE, DEV)
    check(L.ssa_softmax_lastdim_fwd(hb._p(sg.view), K + 3, P, K, OC.SCALE, hb._p(pg.view), Kp, hb._s()), "ssa_softmax_lastdim_fwd")
    check(L.ssa_softmax_lastdim_bwd(hb._p(sg.view), K + 3, P, K, OC.SCALE, hb._p(dpg.view), K + 5, hb._p(dsg.view), Kp, hb._s()),
          "ssa_softmax_lastdim_bwd")
    torch.cuda.synchronize()
    assert_bits_equal("lastdim probs K=%d" % K, pg.view.cpu(), c["probs"])
    want = c["dsim"].clone()
    want[:, K:] = 0                                   # this kernel writes +0.0 to the padding columns
    assert_bits_equal("lastdim dsim K=%d" % K, dsg.view.cpu(), want)
    assert_guard_intact("lastdim K=%d" % K, sg, dpg, pg, dsg)


@pytest.mark.parametrize("f32", [False, True], ids=["src16", "src32"])
@pytest.mark.parametrize("transpose", [0, 1])
def test_exact_ocr_pack_matrix(f32, transpose):
    """ssa_pack_matrix: a [19][45] matrix (rows of 48, a -0.0 among the values) into [rows_out][Kpad], plain and transposed,
    from either source type: every element a copy, the padding +0.0."""
    hb, L, check = _lib()
    R, C, ld = 19, 45, 48
    src = ints((R, C), -100, 100, 77)
    src[3, 7] = -0.0
    sg = guarded_copy(src if f32 else _act(src), DEV, ld)
    rows_out, Kpad = (64, 32) if transpose else (32, 64)
    dg = guarded((rows_out, Kpad), ACT_DTYPE, DEV)
    check(L.ssa_pack_matrix(hb._p(sg.view), int(f32), R, C, ld, transpose, hb._p(dg.view), rows_out, Kpad, hb._s()),
          "ssa_pack_matrix")
    torch.cuda.synchronize()
    want = torch.zeros(rows_out, Kpad, dtype=ACT_DTYPE)
    if transpose:
        want[:C, :R] = _act(src).t()
    else:
        want[:R, :C] = _act(src)
    assert_bits_equal("pack_matrix", dg.view.cpu(), want)
    assert_guard_intact("pack_matrix", sg, dg)


# ---------------------------------------------------------------- the HW softmax through the C ABI
def _hw_softmax(c, pad, accumulate, name):
    hb, L, check = _lib()
    K, HW, C, Kp = c["K"], c["HW"], c["C"], c["Kp"]
    ld = K + pad
    lg = guarded_copy(c["logits"], DEV, ld)
    rs = guarded((K, 2), torch.float32, DEV)
    check(L.ssa_softmax_hw_stats(hb._p(lg.view), ld, HW, K, hb._p(rs.view), hb._s()), "ssa_softmax_hw_stats")
    torch.cuda.synchronize()
    got = rs.view.cpu()
    # value equality: which zero the maximum of the +0.0 class is (it holds both) is left to the kernel
    assert torch.equal(got, c["rowstat"]), "%s rowstat: classes %s differ: got %s want %s" % (
        name, (got != c["rowstat"]).any(1).nonzero().flatten().tolist()[:8],
        got[(got != c["rowstat"]).any(1)][:4].tolist(), c["rowstat"][(got != c["rowstat"]).any(1)][:4].tolist())
    pg = guarded((HW, Kp), ACT_DTYPE, DEV)
    check(L.ssa_softmax_hw_probs(hb._p(lg.view), ld, HW, K, hb._p(rs.view), hb._p(pg.view), Kp, hb._s()), "ssa_softmax_hw_probs")
    cg, dg = guarded_copy(c["ctx"], DEV), guarded_copy(c["dctx"], DEV)
    dot = guarded((K,), torch.float32, DEV)
    check(L.ssa_rowdot_f32(hb._p(cg.view), hb._p(dg.view), K, C, hb._p(dot.view), hb._s()), "ssa_rowdot_f32")
    dpg = guarded_copy(c["dprobs"], DEV, K + 2 * pad)
    dl = guarded((HW, K), torch.float32, DEV, K + 3 * pad)
    pre = None
    if accumulate:
        pre = ints((HW, K), -5, 5, 88)
        dl.view.copy_(pre)
    check(L.ssa_softmax_hw_bwd(hb._p(lg.view), ld, HW, K, hb._p(rs.view), hb._p(dpg.view), K + 2 * pad, hb._p(dot.view),
                               hb._p(dl.view), K + 3 * pad, accumulate, hb._s()), "ssa_softmax_hw_bwd")
    torch.cuda.synchronize()
    assert_bits_equal(name + " probs", pg.view.cpu(), c["probs"])
    assert_bits_equal(name + " dot", dot.view.cpu(), c["dot"])
    want = c["dlogits"] if pre is None else to_f32(pre.double() + c["dlogits"].double())
    assert_bits_equal(name + " dlogits", dl.view.cpu(), want)
    assert_guard_intact(name, lg, rs, pg, cg, dg, dot, dpg, dl)


@pytest.mark.parametrize("case", OC.GATHER, ids=[g[0] for g in OC.GATHER])
def test_exact_ocr_hw_softmax(case):
    """ssa_softmax_hw_stats / _probs / _bwd and ssa_rowdot_f32: the row maxima (negative, -0.0, +0.0 and positive tops) and
    sums, the 16-bit probabilities with their padding, the row dots and dlogits, bit for bit; two cases with logits
    rows longer than K (and dprobs / dlogits rows longer still)."""
    name, K, H, W, C, pad = case
    _hw_softmax(_gather(K, H * W, C), pad, 0, "hw softmax " + name)


def test_exact_ocr_hw_softmax_accumulate():
    """accumulate = 1 of ssa_softmax_hw_bwd: dlogits pre-filled with integers."""
    name, K, H, W, C, pad = OC.GATHER[3]
    _hw_softmax(_gather(K, H * W, C), 4, 1, "hw softmax accumulate " + name)


@pytest.mark.skipif(_EMU, reason="16,515 pixels x 256 classes: GPU only")
def test_exact_ocr_hw_softmax_rebalance():
    """K = 256, HW = 16515: more than 1024 workgroups of 16 pixels are re-balanced to 972 of 17."""
    name, K, H, W, C, pad = OC.GATHER_REBALANCE
    c = _gather(K, H * W, C)
    assert c["plan"][1] == 17 and c["plan"][2] > 1
    _hw_softmax(c, pad, 0, "hw softmax " + name)


# ---------------------------------------------------------------- the Python composition, through autograd
@pytest.mark.parametrize("K,fused", [(19, True), (65, True), (96, True), (19, False), (97, True)],
                         ids=["k19", "k65", "k96", "k19-three-launch", "k97-fallback"])
def test_exact_ocr_attn_autograd(K, fused, monkeypatch):
    """OcrAttnFn on two images with different k and v, q a channel slice of a wider NHWC tensor: out, dq, and dk / dv (the
    weight-gradient kernel's pixel reductions, after the cast back to the operand type) bit for bit, on the fused
    kernel, on the three-launch form forced, and on the fallback 97 regions take."""
    hb, L, check = _lib()
    monkeypatch.setattr(hb, "_OCR_ATTN_FUSED", fused)
    B, H, W = 2, 12, 25
    cs = [_tie(K, H * W, b) for b in range(B)]
    qg = guarded((B, H, W, D), ACT_DTYPE, DEV, D + 16)
    qg.view.copy_(torch.stack([_act(c["q"]) for c in cs]).view(B, H, W, D))
    qd = qg.view.detach().requires_grad_(True)
    assert hb._pixels(qd)[1] == D + 16
    kd = torch.stack([_act(c["k"]) for c in cs]).to(DEV).requires_grad_(True)
    vd = torch.stack([_act(c["v"]) for c in cs]).to(DEV).requires_grad_(True)
    od = hb.OcrAttnFn.apply(qd, kd, vd, OC.SCALE)
    od.backward(torch.stack([_act(c["dout"]) for c in cs]).view(B, H, W, D).to(DEV))
    torch.cuda.synchronize()
    tag = "OcrAttnFn K=%d%s" % (K, "" if fused else " three-launch")
    for b, c in enumerate(cs):
        assert_bits_equal("%s image %d out" % (tag, b), od[b].detach().cpu().view(-1, D), c["out"])
        assert_bits_equal("%s image %d dq" % (tag, b), qd.grad[b].cpu().view(-1, D), c["dq"])
        assert_bits_equal("%s image %d dv" % (tag, b), vd.grad[b].cpu(), to_act(c["dv64"]))
        assert_bits_equal("%s image %d dk" % (tag, b), kd.grad[b].cpu(), to_act(c["dk64"]))
    assert_guard_intact(tag, qg)


@pytest.mark.parametrize("case", OC.GATHER, ids=[g[0] for g in OC.GATHER])
def test_exact_ocr_gather_autograd(case):
    """OcrGatherFn on two images with different logits: ctx (fp32), dfeats (16 bit) and dlogits (fp32) bit for bit."""
    hb, L, check = _lib()
    name, K, H, W, C, pad = case
    B = 2
    cs = [_gather(K, H * W, C, b) for b in range(B)]
    fd = torch.stack([_act(c["feats"]) for c in cs]).view(B, H, W, C).to(DEV).requires_grad_(True)
    lg = guarded((B, H, W, K), torch.float32, DEV, K + pad)
    lg.view.copy_(torch.stack([c["logits"] for c in cs]).view(B, H, W, K))
    ld = lg.view.detach().requires_grad_(True)
    out = hb.OcrGatherFn.apply(fd, ld)
    out.backward(torch.stack([c["dctx"] for c in cs]).to(DEV))
    torch.cuda.synchronize()
    for b, c in enumerate(cs):
        tag = "OcrGatherFn %s image %d" % (name, b)
        assert_bits_equal(tag + " ctx", out[b].detach().cpu(), c["ctx"])
        assert_bits_equal(tag + " dfeats", fd.grad[b].cpu().view(-1, C), c["dfeats"])
        assert_bits_equal(tag + " dlogits", ld.grad[b].cpu().view(-1, K), c["dlogits"])
    assert_guard_intact("OcrGatherFn " + name, lg)
