"""Exact (integer-operand, bit-for-bit) tests of the operand gather of ConvIgemm (csrc/conv_igemm.hip).

The gather addresses a 16-byte piece as  base + row offset + tap offset + channel offset  with a tap-validity mask per
row and a tap cursor advanced by additions; the shapes below are the smallest at which each part of that arithmetic can
go wrong: a batch of two with odd extents (rows of a tile in different images, image edges on every side), a tap
boundary inside a K-stage (48 channels against stages of 32 and 64), several taps in one stage (8 channels), a masked
K tail (Kpad a multiple of 32, not of 64), an N tail, a channel-sliced input (ldx > Cin), dilation, the transposed
forms (stride 1: the fast gather; stride 2: the general one), more than 32 taps (7x7: the general gather), the strided
output of the parity data gradient, the fp32 and the inference epilogues.  Every case runs at the tile configurations
4 (64x64, stages of 64) and 0 (128x128, stages of 32); the first at all six.

Tolerance: zero, by the argument of tests/exact_util.py.  Inputs sit in NaN-filled guarded buffers (a stray read that
is not zeroed poisons the output; a wrong offset inside the tensor changes its bits) and the guard bands around every
output are checked."""
import ctypes

import pytest
import torch

from util import nhwc, ACT_DTYPE
from exact_util import (assert_bits_equal, assert_guard_intact, assert_integers, assert_premise, choice, conv_ref64,
                        guarded, guarded_copy, ints, not_representable, to_act, to_f32)
from test_kernels_gpu import _exact_fwd_check, _hb

pytestmark = pytest.mark.gpu

DEV = "cuda"
CFGS = [4, 0]


def _sync():
    if DEV != "cpu":
        torch.cuda.synchronize()


def _stats(hb, Cout):
    sg = guarded((hb.stat_replicas(), 2, Cout), torch.float64, DEV)
    sg.view.zero_()
    return sg


def _fwd(cfg, B, H, W, Cin, Cout, k, stride, pad, dil, stats=True, ldx=None, bias=False, out_f32=False, seed=0):
    """One forward conv through hb._igemm at tile configuration cfg; returns (y, stats, x) guarded and the reference."""
    hb = _hb()
    x, w = ints((B, Cin, H, W), -3, 3, 50 + seed), ints((Cout, Cin, k, k), -2, 2, 60 + seed)
    b = ints((Cout,), -5, 5, 70 + seed) if bias else None
    ref = conv_ref64(x, w, b, stride, pad, dil).permute(0, 2, 3, 1).contiguous()
    Ho, Wo = ref.shape[1], ref.shape[2]
    hb.clear_pack_cache()
    xg = guarded_copy(nhwc(x).to(ACT_DTYPE), DEV, ldx)
    wd = w.to(DEV)
    wp, Kpad = hb._packed_filter(wd, 0, Cin, 0)
    yg = guarded((B, Ho, Wo, Cout), torch.float32 if out_f32 else ACT_DTYPE, DEV)
    sg = _stats(hb, Cout) if stats and not out_f32 else None
    hb._igemm(xg.view, ldx or Cin, (B, H, W, Cin), wp, Kpad, b.to(DEV) if bias else None, (Ho, Wo), Cout, (k, k), stride,
              pad, dil, False, out_f32, cfg=cfg, stats=sg.view if sg else None, out=yg.view)
    _sync()
    hb.clear_pack_cache()
    return yg, sg, xg, ref, Kpad


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
def test_exact_gather_s2_batch_odd_edges(cfg):
    """(a) 3x3 stride 2 pad 1, B = 2, 13 x 11, 48 -> 40 channels, with statistics: K = 432 -> Kpad 448 = 7 stages of 64
    or 14 of 32, the last 16 columns past the taps; a tap ends every 48 channels, i.e. inside a stage.  (448 is a
    multiple of 64: the half-masked last stage of 64 is in (b), (d) and (h), Kpad = 96 and 224.)"""
    yg, sg, xg, ref, Kpad = _fwd(cfg, 2, 13, 11, 48, 40, 3, 2, 1, 1)
    assert Kpad == 448
    print("[exact gather a] %d outputs not representable" % not_representable(ref))
    _exact_fwd_check("gather (a) cfg%d" % cfg, yg, sg, ref, 40)
    assert_guard_intact("gather (a) cfg%d input" % cfg, xg)


@pytest.mark.parametrize("cfg", CFGS)
def test_exact_gather_many_taps_per_stage(cfg):
    """(b) 3x3 stride 2 pad 1 on 9 x 9 with 8 channels: four (eight) taps in one stage of 32 (64); K = 72 -> Kpad 96."""
    yg, sg, xg, ref, Kpad = _fwd(cfg, 1, 9, 9, 8, 24, 3, 2, 1, 1, seed=1)
    assert Kpad == 96 and Kpad % 64 == 32
    _exact_fwd_check("gather (b) cfg%d" % cfg, yg, sg, ref, 24)
    assert_guard_intact("gather (b) cfg%d input" % cfg, xg)


@pytest.mark.parametrize("cfg", CFGS)
def test_exact_gather_1x1_channel_slice(cfg):
    """(c) 1x1 on 37 x 45, 72 -> 88 channels, read from a channel slice of rows of 96 elements (the neighbouring
    channels are NaN)."""
    yg, sg, xg, ref, _ = _fwd(cfg, 1, 37, 45, 72, 88, 1, 1, 0, 1, ldx=96, seed=2)
    _exact_fwd_check("gather (c) cfg%d" % cfg, yg, sg, ref, 88)
    assert_guard_intact("gather (c) cfg%d input" % cfg, xg)


@pytest.mark.parametrize("cfg", CFGS)
def test_exact_gather_dilated(cfg):
    """(d) 3x3 stride 1, dilation 2, pad 2; 24 channels: K = 216 -> Kpad 224, the last stage of 64 half masked."""
    yg, sg, xg, ref, Kpad = _fwd(cfg, 1, 13, 11, 24, 40, 3, 1, 2, 2, seed=3)
    assert Kpad % 64 == 32
    _exact_fwd_check("gather (d) cfg%d" % cfg, yg, sg, ref, 40)
    assert_guard_intact("gather (d) cfg%d input" % cfg, xg)


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("stride", [1, 2])
def test_exact_gather_transposed(stride, cfg):
    """(e) the transposed form (data gradient of a 3x3 pad-1 conv 16 -> 24 on 13 x 11) at stride 1 (fast gather: the
    tap offsets are linear) and stride 2 (general gather: zero-inserted rows and columns).  Reference: the float64
    gradient of the conv with respect to its input."""
    hb = _hb()
    B, H, W, Cin, Cout = 2, 13, 11, 16, 24
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    w, dy = ints((Cout, Cin, 3, 3), -2, 2, 81), ints((B, Cout, Ho, Wo), -3, 3, 82)
    assert_integers("gather (e)", w, dy)
    F = torch.nn.functional

    def dgrad(ww, gg):
        xx = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(xx, ww, None, stride, 1, 1).backward(gg)
        return xx.grad.permute(0, 2, 3, 1).contiguous()
    assert_premise("gather (e)", dgrad(w.double().abs(), dy.double().abs()))
    ref = dgrad(w.double(), dy.double())
    hb.clear_pack_cache()
    wd = w.to(DEV)
    dg = guarded_copy(nhwc(dy).to(ACT_DTYPE), DEV)
    wpt, Kpad = hb._packed_filter(wd, 1, 0, Cout)
    dxg = guarded((B, H, W, Cin), ACT_DTYPE, DEV)
    hb._igemm(dg.view, Cout, (B, Ho, Wo, Cout), wpt, Kpad, None, (H, W), Cin, (3, 3), stride, 1, 1, True, False, cfg=cfg,
              out=dxg.view)
    _sync()
    name = "gather (e) stride %d cfg%d" % (stride, cfg)
    assert_bits_equal(name, dxg.view.cpu(), to_act(ref))
    assert_guard_intact(name, dg, dxg)
    hb.clear_pack_cache()


def test_exact_gather_dgrad_s2_parity_classes():
    """(f) ssa_conv2d_dgrad_s2 on 13 x 11 (48 <- 24 channels, B = 2): the four parity classes are 7 x 6, 7 x 5, 6 x 6 and
    6 x 5 pixels, written through the strided output map.  (The entry point chooses the tile itself.)"""
    from semseg_amd._lib import check
    hb = _hb()
    B, H, W, Cin, Cout = 2, 13, 11, 48, 24
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w, dy = ints((Cout, Cin, 3, 3), -2, 2, 91), ints((B, Cout, Ho, Wo), -3, 3, 92)
    assert_integers("gather (f)", w, dy)
    F = torch.nn.functional

    def dgrad(ww, gg):
        xx = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(xx, ww, None, 2, 1, 1).backward(gg)
        return xx.grad.permute(0, 2, 3, 1).contiguous()
    assert_premise("gather (f)", dgrad(w.double().abs(), dy.double().abs()))
    ref = dgrad(w.double(), dy.double())
    hb.clear_pack_cache()
    wd = w.to(DEV)
    dg = guarded_copy(nhwc(dy).to(ACT_DTYPE), DEV)
    packs = [hb._packed_filter(wd, 4 + c, 0, Cout) for c in range(4)]
    dxg = guarded((B, H, W, Cin), ACT_DTYPE, DEV)
    wp = (ctypes.c_void_p * 4)(*[t.data_ptr() for t, _ in packs])
    kp = (ctypes.c_int * 4)(*[k for _, k in packs])
    check(hb.lib().ssa_conv2d_dgrad_s2(B, H, W, Cin, Cin, Ho, Wo, Cout, Cout, hb._p(dg.view), wp, kp, hb._p(dxg.view),
                                       hb._s()), "ssa_conv2d_dgrad_s2")
    _sync()
    assert_bits_equal("gather (f)", dxg.view.cpu(), to_act(ref))
    assert_guard_intact("gather (f)", dg, dxg)
    hb.clear_pack_cache()


@pytest.mark.parametrize("cfg", CFGS)
def test_exact_gather_7x7_general_form(cfg):
    """(g) 7x7 stride 2 pad 3 with 8 channels: 49 taps, more than a 32-bit tap mask holds -- the general gather."""
    yg, sg, xg, ref, _ = _fwd(cfg, 1, 13, 11, 8, 16, 7, 2, 3, 1, seed=4)
    _exact_fwd_check("gather (g) cfg%d" % cfg, yg, sg, ref, 16)
    assert_guard_intact("gather (g) cfg%d input" % cfg, xg)


@pytest.mark.parametrize("cfg", CFGS)
def test_exact_gather_fp32_out_bias(cfg):
    """(h) fp32 output with bias, 19 output channels (an exact integer: no rounding at all)."""
    yg, _, xg, ref, _ = _fwd(cfg, 1, 13, 11, 24, 19, 3, 1, 1, 1, bias=True, out_f32=True, seed=5)
    assert_bits_equal("gather (h) cfg%d" % cfg, yg.view.cpu(), to_f32(ref))
    assert_guard_intact("gather (h) cfg%d" % cfg, yg, xg)


@pytest.mark.parametrize("cfg", CFGS)
def test_exact_gather_affine_epilogue(cfg):
    """(i) the shape of (a) through ssa_conv2d_igemm_affine with residual and ReLU: z = r16(max(scale * r16(conv) + shift
    + residual, 0)).  Scales are powers of two and shifts / residuals integers, so that every fp32 step between the two
    roundings is exact whichever way it is contracted."""
    hb = _hb()
    B, H, W, Cin, Cout = 2, 13, 11, 48, 40
    x, w = ints((B, Cin, H, W), -3, 3, 50), ints((Cout, Cin, 3, 3), -2, 2, 60)
    ref = conv_ref64(x, w, None, 2, 1, 1).permute(0, 2, 3, 1).contiguous()
    Ho, Wo = ref.shape[1], ref.shape[2]
    scale, shift = choice((Cout,), [1.0, 2.0, -1.0, 0.5, -0.5], 101), ints((Cout,), -5, 5, 102)
    res = ints((B, Ho, Wo, Cout), -20, 20, 103)
    y16 = to_act(ref).double()
    want = to_act(torch.clamp(y16 * scale.double() + shift.double() + res.double(), min=0.0))
    assert int((want != 0).sum()) > 0 and int((want == 0).sum()) > 0
    hb.clear_pack_cache()
    xg = guarded_copy(nhwc(x).to(ACT_DTYPE), DEV)
    rg = guarded_copy(res.to(ACT_DTYPE), DEV, Cout + 8)
    wd = w.to(DEV)
    wp, Kpad = hb._packed_filter(wd, 0, Cin, 0)
    coef = torch.stack([scale, shift]).contiguous().to(DEV)
    yg = guarded((B, Ho, Wo, Cout), ACT_DTYPE, DEV)
    hb._igemm(xg.view, Cin, (B, H, W, Cin), wp, Kpad, None, (Ho, Wo), Cout, (3, 3), 2, 1, 1, False, False, cfg=cfg,
              out=yg.view, affine=(coef, rg.view, Cout + 8, True))
    _sync()
    name = "gather (i) cfg%d" % cfg
    assert_bits_equal(name, yg.view.cpu(), want)
    assert_guard_intact(name, yg, xg, rg)
    hb.clear_pack_cache()
