"""Op-level parity: every HIP kernel (through the C ABI) against the oracle
(oracle/ops.py, CPU fp32/fp64) on identical seeded inputs.

Tolerance (stated once): activations are bf16, accumulation fp32.  Inputs and
weights are rounded to bf16 before BOTH paths, so the only differences are the
fp32 accumulation order and one bf16 rounding of the output (2^-9 relative):
max error <= 1e-2 * max|ref|, mean error <= 4e-3 * mean|ref|.  fp32-out ops
use 2e-3 / 5e-4, fp64 RMI statistics 1e-4.
"""
import math
import os

import pytest
import torch

from util import bf16_round, check_close, report, nhwc, nchw, ACT_DTYPE

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _hb():
    from semseg_amd import hip_backend
    return hip_backend


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return bf16_round(torch.randn(*shape, generator=g) * scale)


# ----------------------------------------------------------------- probes
def test_probe_mfma32(out_dir):
    from semseg_amd._lib import lib, check
    import ctypes
    a = _rand(32, 16, seed=1)
    b = _rand(16, 32, seed=2)       # asymmetric on purpose
    a_d = a.to(DEV).to(ACT_DTYPE).contiguous()
    bt_d = b.t().contiguous().to(DEV).to(ACT_DTYPE)
    c_d = torch.zeros(32, 32, device=DEV)
    check(lib().ssa_probe_mfma32(ctypes.c_void_p(a_d.data_ptr()), ctypes.c_void_p(bt_d.data_ptr()),
                                 ctypes.c_void_p(c_d.data_ptr()), None), "probe")
    torch.cuda.synchronize()
    check_close("mfma32", c_d, a @ b, 1e-5, 1e-5)


def test_probe_mfma16():
    """Lane map of v_mfma_f32_16x16x32 (csrc/common.h ssa_mfma16): A rows / B columns l & 15, k = 8 * (l >> 4) + j;
    accumulator column l & 15, rows 4 * (l >> 4) + j."""
    import ctypes
    from semseg_amd._lib import lib, check
    a = _rand(16, 32, seed=1)
    b = _rand(32, 16, seed=2)       # asymmetric on purpose
    a_d = a.to(DEV).to(ACT_DTYPE).contiguous()
    bt_d = b.t().contiguous().to(DEV).to(ACT_DTYPE)
    c_d = torch.zeros(16, 16, device=DEV)
    check(lib().ssa_probe_mfma16(ctypes.c_void_p(a_d.data_ptr()), ctypes.c_void_p(bt_d.data_ptr()),
                                 ctypes.c_void_p(c_d.data_ptr()), None), "probe")
    torch.cuda.synchronize()
    check_close("mfma16", c_d, a @ b, 1e-5, 1e-5)


def test_probe_swap16():
    """v_permlane16_swap: odd 16-lane rows of the first operand <-> even rows of the second."""
    import ctypes
    from semseg_amd._lib import lib, check
    out = torch.zeros(64, 2, dtype=torch.int32, device=DEV)
    check(lib().ssa_probe_swap16(ctypes.c_void_p(out.data_ptr()), None), "probe")
    torch.cuda.synchronize()
    want = []
    for l in range(64):
        if (l >> 4) & 1 == 0:
            want.append((l, l ^ 16))                  # (own a, partner's a)
        else:
            want.append(((l ^ 16) + 100, l + 100))    # (partner's b, own b)
    assert out.cpu().tolist() == [list(t) for t in want]


def test_probe_tr16(out_dir):
    from semseg_amd._lib import lib, check
    import ctypes
    with open(os.path.join(out_dir, "probe_tr16.txt"), "w") as f:
        for mode in (0, 1, 2):
            out = torch.zeros(256, dtype=torch.int16, device=DEV)
            check(lib().ssa_probe_tr16(ctypes.c_void_p(out.data_ptr()), mode, None), "probe_tr16")
            torch.cuda.synchronize()
            v = out.cpu().view(64, 4).tolist()
            f.write("mode %d\n" % mode)
            for l, row in enumerate(v):
                f.write("lane %2d: %s\n" % (l, row))
    assert True


# ------------------------------------------------------------------- conv
CONV_CASES = [
    # B, H, W, Cin(real), Cout, k, stride, pad, dil, bias, out_f32
    (2, 40, 56, 48, 48, 3, 1, 1, 1, False, False),
    (1, 64, 64, 3, 64, 3, 2, 1, 1, False, False),
    (2, 33, 47, 64, 256, 1, 1, 0, 1, False, False),
    (1, 48, 40, 96, 192, 3, 2, 1, 1, False, False),
    (1, 24, 24, 720, 512, 3, 1, 1, 1, True, False),
    (2, 32, 32, 512, 19, 1, 1, 0, 1, True, True),
    (1, 32, 32, 256, 1, 1, 1, 0, 1, False, True),
    (1, 40, 40, 64, 32, 3, 1, 12, 12, False, False),
    (1, 16, 16, 384, 384, 3, 1, 1, 1, False, False),
    (1, 37, 29, 96, 96, 3, 1, 1, 1, False, False),
    (1, 19, 1, 512, 256, 1, 1, 0, 1, False, False),
    # DeepLabV3+/ResNet-50 shapes: 7x7 stride-2 stem, strided 1x1 downsample, ASPP dilations
    (1, 64, 80, 3, 64, 7, 2, 3, 1, False, False),
    (1, 24, 32, 256, 512, 1, 2, 0, 1, False, False),
    (2, 12, 16, 512, 256, 3, 1, 24, 24, False, False),
    (1, 12, 16, 2048, 256, 1, 1, 0, 1, False, False),
    (1, 20, 28, 128, 128, 3, 1, 2, 2, False, False),
    # halo-tile kernel (conv_tile.hip): every (Cin, n-block, tile-width) dispatch class
    (1, 70, 75, 64, 64, 3, 1, 1, 1, False, False),
    (1, 130, 129, 48, 48, 3, 1, 1, 1, True, False),
    (2, 20, 12, 48, 96, 3, 1, 1, 1, False, False),
    (1, 9, 7, 96, 48, 3, 1, 1, 1, False, False),
    (1, 33, 18, 64, 24, 3, 1, 1, 1, False, False),
    (1, 128, 160, 96, 96, 3, 1, 1, 1, False, False),
    (1, 33, 30, 192, 96, 3, 1, 1, 1, False, False),
    (2, 20, 12, 384, 200, 3, 1, 1, 1, True, False),
    (1, 64, 64, 192, 192, 3, 1, 1, 1, False, False),
    # large-channel head convs (ssa_conv2d_halo): 3x3 on ConvHaloReg3, 1x1 on ConvHaloGemm1; CK 48 / 64, ragged tiles,
    # partial n-blocks
    (1, 130, 131, 192, 200, 3, 1, 1, 1, True, False),
    (1, 128, 129, 240, 128, 3, 1, 1, 1, False, False),
    (2, 96, 100, 256, 72, 1, 1, 0, 1, False, False),
    (1, 140, 128, 336, 64, 1, 1, 0, 1, True, False),
    # 3x3 stride-2 down-convs: data gradient by output parity (ssa_conv2d_dgrad_s2) -- odd / even extents,
    # Cout that is no multiple of 32, one-pixel-wide classes
    (1, 37, 45, 48, 96, 3, 2, 1, 1, False, False),
    (2, 33, 64, 96, 200, 3, 2, 1, 1, True, False),
    (1, 128, 128, 64, 64, 3, 2, 1, 1, False, False),
    (1, 2, 3, 48, 24, 3, 2, 1, 1, False, False),
    (1, 1, 9, 48, 48, 3, 2, 1, 1, False, False),
    # the scale-attention head's last conv (network/utils.py:360: 256 -> 1, fp32 out) at the three pass sizes of a
    # 128 x 192 {0.5, 1, 2} evaluation -- round 4's fp16 end-to-end test pointed at the smallest one
    (1, 16, 24, 256, 1, 1, 1, 0, 1, False, True),
    (1, 32, 48, 256, 1, 1, 1, 0, 1, False, True),
    (1, 64, 96, 256, 1, 1, 1, 0, 1, False, True),
]


def _conv_inputs(case, seed=0):
    B, H, W, Cin, Cout, k, s, p, d, bias, out_f32 = case
    x = _rand(B, Cin, H, W, seed=seed)
    w = _rand(Cout, Cin, k, k, seed=seed + 1, scale=1.0 / math.sqrt(Cin * k * k))
    b = _rand(Cout, seed=seed + 2) if bias else None
    return x, w, b


def _to_dev_nhwc(x, cpad=None):
    t = nhwc(x)
    if cpad is not None and cpad > t.shape[3]:
        t = torch.nn.functional.pad(t, (0, cpad - t.shape[3]))
    return t.to(DEV).to(ACT_DTYPE).contiguous()


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_fwd_bwd(case):
    from oracle import ops as O
    hb = _hb()
    B, H, W, Cin, Cout, k, s, p, d, bias, out_f32 = case
    x, w, b = _conv_inputs(case)
    cin_pad = (Cin + 7) // 8 * 8 if Cin >= 8 else 16
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if b is not None else None
    yr = O.conv2d(xr, wr, br, s, p, d)
    gy = _rand(*yr.shape, seed=7)
    yr.backward(gy)

    xd = _to_dev_nhwc(x, cin_pad).requires_grad_(cin_pad == Cin)
    wd = w.to(DEV).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True) if b is not None else None
    hb.clear_pack_cache()
    yd = hb.Conv2dFn.apply(xd, wd, bd, s, p, d, out_f32)
    torch.cuda.synchronize()
    tol = (2e-3, 5e-4) if out_f32 else (1e-2, 4e-3)
    check_close("conv_fwd %s" % (case,), nchw(yd.float()), yr, *tol)
    gyd = nhwc(gy).to(DEV)
    if not out_f32:
        gyd = gyd.to(ACT_DTYPE)
    yd.backward(gyd)
    torch.cuda.synchronize()
    if cin_pad == Cin:
        check_close("conv_dgrad %s" % (case,), nchw(xd.grad.float()), xr.grad)
    # weight grads: fp32 out, but dy is rounded to bf16 for the fp32 heads
    check_close("conv_wgrad %s" % (case,), wd.grad, wr.grad, 1e-2, 4e-3)
    if b is not None:
        check_close("conv_bgrad %s" % (case,), bd.grad, br.grad, 1e-2, 4e-3)


WIDE_CASES = [
    # B, H, W, Cin, Cout, bias, stats, transposed-pack (the data-gradient form: ssa_pack_filter mode 3)
    (1, 16, 32, 96, 264, False, True, False),      # two pixel tiles x two channel tiles, the second 8 channels wide
    (1, 9, 31, 80, 520, True, True, False),        # ragged pixel tile (279 pixels), Cin = 2.5 stages, three channel tiles
    (2, 16, 16, 64, 256, True, False, False),      # one channel tile, exactly two stages (the ring's clamped prefetches)
    (1, 20, 16, 272, 328, False, True, True),      # data-gradient packing, 8.5 stages (ring wraps twice), n-block tail
]


@pytest.mark.parametrize("case", WIDE_CASES)
def test_gemm_wide_1x1(case):
    """csrc/conv_gemm_wide.hip through its own entry point (ssa_conv2d_halo forwards only the large head problems to
    it): every tile / stage / ring edge at sizes the CPU emulation runs in seconds -- ragged pixel tile, Cin that is no
    multiple of the 32-channel stage, channel-tile and n-block tails, bias, the BatchNorm partial sums of the ROUNDED
    outputs, both filter packings."""
    import ctypes
    from oracle import ops as O
    from semseg_amd._lib import check
    hb = _hb()
    B, H, W, Cin, Cout, bias, stats, tr = case
    x = _rand(B, Cin, H, W, seed=3)
    w = _rand(Cout, Cin, 1, 1, seed=4, scale=1.0 / math.sqrt(Cin))
    b = _rand(Cout, seed=5) if bias else None
    ref = O.conv2d(x, w, b, 1, 0, 1)
    xd = _to_dev_nhwc(x)
    hb.clear_pack_cache()
    if tr:      # the weight of the conv whose DATA gradient this is: [Cin_fwd = Cout here][Cout_fwd = Cin here]
        wt = w[:, :, 0, 0].t().contiguous().view(Cin, Cout, 1, 1).to(xd.device)
        wp, _ = hb._packed_filter(wt, 3, 0, Cin)
    else:
        wp, _ = hb._packed_filter(w.to(xd.device), 2, Cin, 0)
    d = hb._tile_desc(B, H, W, Cin, Cin, Cout, (1, 1), 1, 0, 1, H, W, False)
    L = hb.lib()
    assert L.ssa_conv2d_gemm_wide_supported(ctypes.byref(d)) == 0      # (too small for the dispatcher: direct call)
    y = torch.empty(B, H, W, Cout, dtype=ACT_DTYPE, device=xd.device)
    nrep = hb.stat_replicas()
    st = torch.zeros(nrep, 2, Cout, dtype=torch.float64, device=xd.device) if stats else None
    bd = b.to(xd.device) if b is not None else None
    check(L.ssa_conv2d_gemm_wide(ctypes.byref(d), hb._p(xd), hb._p(wp), hb._p(bd), hb._p(y), hb._p(st), hb._s()), "wide")
    if xd.is_cuda:
        torch.cuda.synchronize()
    check_close("gemm_wide %s" % (case,), nchw(y.float()), ref)
    if stats:
        yr = y.float().view(-1, Cout).double()
        got = st.sum(0).cpu()
        check_close("gemm_wide sums %s" % (case,), got[0], yr.sum(0).cpu(), 1e-4, 1e-4)
        check_close("gemm_wide squares %s" % (case,), got[1], (yr * yr).sum(0).cpu(), 1e-4, 1e-4)


HALO_REG_CASES = [
    # B, H, W, Cin, Cout, bias, stats, transposed-pack (the data-gradient form: ssa_pack_filter mode 3)
    (1, 8, 64, 128, 264, True, True, False),       # 2 x 2 pixel tiles, two 64-channel chunks, two channel tiles (2nd: 8 wide)
    (1, 7, 37, 96, 72, False, True, False),        # ragged tile rows / columns, two 48-channel chunks, n-block tail
    (2, 4, 32, 192, 256, True, False, False),      # batch 2, three 64-channel chunks (odd count), one full channel tile
    (1, 9, 33, 144, 320, False, True, True),       # data-gradient packing, three 48-channel chunks, image edge columns
]


@pytest.mark.parametrize("case", HALO_REG_CASES)
def test_halo_reg_3x3(case):
    """csrc/conv_halo_reg.hip through its own entry point (ssa_conv2d_halo forwards the head's 3x3 problems to it): the
    register-fed filter ring, the masked halo DMA (image borders, ragged tiles, the unused pieces of a 48-channel chunk),
    both chunk widths with even / odd chunk counts, channel-tile and n-block tails, bias, the BatchNorm partial sums of the
    ROUNDED outputs, both filter packings -- at sizes the CPU emulation runs in seconds."""
    import ctypes
    from oracle import ops as O
    from semseg_amd._lib import check
    hb = _hb()
    B, H, W, Cin, Cout, bias, stats, tr = case
    x = _rand(B, Cin, H, W, seed=3)
    w = _rand(Cout, Cin, 3, 3, seed=4, scale=1.0 / math.sqrt(9 * Cin))
    b = _rand(Cout, seed=5) if bias else None
    ref = O.conv2d(x, w, b, 1, 1, 1)
    xd = _to_dev_nhwc(x)
    hb.clear_pack_cache()
    if tr:      # the weight of the conv whose DATA gradient this is: flipped taps, [Cin_fwd = Cout here][Cout_fwd = Cin here]
        wt = w.flip(2, 3).permute(1, 0, 2, 3).contiguous().to(xd.device)
        wp, _ = hb._packed_filter(wt, 3, 0, Cin)
    else:
        wp, _ = hb._packed_filter(w.to(xd.device), 2, Cin, 0)
    d = hb._tile_desc(B, H, W, Cin, Cin, Cout, (3, 3), 1, 1, 1, H, W, False)
    L = hb.lib()
    assert L.ssa_conv2d_halo_reg_supported(ctypes.byref(d)) == 1
    y = torch.empty(B, H, W, Cout, dtype=ACT_DTYPE, device=xd.device)
    nrep = hb.stat_replicas()
    st = torch.zeros(nrep, 2, Cout, dtype=torch.float64, device=xd.device) if stats else None
    bd = b.to(xd.device) if b is not None else None
    check(L.ssa_conv2d_halo_reg(ctypes.byref(d), hb._p(xd), hb._p(wp), hb._p(bd), hb._p(y), hb._p(st), hb._s()), "halo_reg")
    if xd.is_cuda:
        torch.cuda.synchronize()
    check_close("halo_reg %s" % (case,), nchw(y.float()), ref)
    if stats:
        yr = y.float().view(-1, Cout).double()
        got = st.sum(0).cpu()
        check_close("halo_reg sums %s" % (case,), got[0], yr.sum(0).cpu(), 1e-4, 1e-4)
        check_close("halo_reg squares %s" % (case,), got[1], (yr * yr).sum(0).cpu(), 1e-4, 1e-4)


def test_stride2_dgrad_by_parity_matches_zero_inserted():
    """ssa_conv2d_dgrad_s2 (four dense parity classes) against the zero-inserted transposed form it
    replaces: same operands, same bf16 rounding of the result; the two differ only in the order of the
    fp32 accumulation (taps that multiply inserted zeros contribute nothing)."""
    hb = _hb()
    for (B, H, W, Cin, Cout) in [(1, 64, 64, 48, 96), (2, 31, 50, 96, 96), (1, 17, 16, 192, 384)]:
        hb.clear_pack_cache()
        w = _rand(Cout, Cin, 3, 3, seed=11, scale=0.05).to(DEV)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        dy = nhwc(_rand(B, Cout, Ho, Wo, seed=12)).to(DEV).to(ACT_DTYPE).contiguous()
        assert hb._DGRAD_S2
        got = hb._conv_dgrad((B, H, W, Cin), w, dy, Cout, Cout, 2, 1, 1, (Ho, Wo))
        hb._DGRAD_S2 = False
        try:
            want = hb._conv_dgrad((B, H, W, Cin), w, dy, Cout, Cout, 2, 1, 1, (Ho, Wo))
        finally:
            hb._DGRAD_S2 = True
        torch.cuda.synchronize()
        assert got.shape == want.shape == (B, H, W, Cin)
        check_close("dgrad_s2 %s" % ((B, H, W, Cin, Cout),), got.float(), want.float(), 8e-3, 1e-3)
        # inside a group bracket: the four classes leave as one launch per tile instantiation
        hb.lib().ssa_launch_count(1)
        with hb.group():
            got2 = hb._conv_dgrad((B, H, W, Cin), w, dy, Cout, Cout, 2, 1, 1, (Ho, Wo))
        torch.cuda.synchronize()
        assert hb.lib().ssa_launch_count(1) <= (1 if H % 2 == 0 and W % 2 == 0 else 4)
        assert torch.equal(got2.view(torch.int16), got.view(torch.int16))
    hb.clear_pack_cache()


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
def test_conv_all_tile_configs(cfg):
    """Every tile configuration on a shape with ragged M and N tails."""
    import ctypes
    from oracle import ops as O
    hb = _hb()
    B, H, W, Cin, Cout = 1, 37, 45, 72, 88
    x = _rand(B, Cin, H, W, seed=3)
    w = _rand(Cout, Cin, 3, 3, seed=4, scale=0.04)
    yr = O.conv2d(x, w, None, 1, 1, 1)
    xd = _to_dev_nhwc(x)
    wd = w.to(DEV)
    hb.clear_pack_cache()
    wp, Kpad = hb._packed_filter(wd, 0, Cin, 0)
    y = hb._igemm(xd, Cin, (B, H, W, Cin), wp, Kpad, None, (H, W), Cout, (3, 3), 1, 1, 1, False, False, cfg=cfg)
    torch.cuda.synchronize()
    check_close("conv cfg%d" % cfg, nchw(y.float()), yr)


@pytest.mark.parametrize("C,H,W", [(48, 50, 70), (96, 17, 33), (64, 128, 128), (192, 96, 96)])
def test_conv_bn_fused_stats(C, H, W):
    """conv -> BN (training) with the batch statistics accumulated in the conv
    epilogue (HipBackend.conv_bn_act) == oracle conv followed by batch_norm."""
    from oracle import ops as O
    from semseg_amd import ops, nn as snn
    hb = _hb()
    B = 2
    x = _rand(B, C, H, W, seed=11)
    conv = snn.Conv2d(C, C, 3, 1, 1, bias=False)
    bn = snn.BatchNorm2d(C)
    with torch.no_grad():
        conv.weight.copy_(_rand(C, C, 3, 3, seed=12, scale=0.05))
        bn.weight.copy_(torch.rand(C) + 0.5)
        bn.bias.copy_(torch.randn(C) * 0.1)
    rm, rv = torch.zeros(C), torch.ones(C)
    yr = O.conv2d(x, conv.weight.detach(), None, 1, 1, 1)
    zr = torch.relu(O.batch_norm(bf16_round(yr), bn.weight.detach(), bn.bias.detach(), rm, rv, True, 0.1, 1e-5))
    conv, bn = conv.to(DEV), bn.to(DEV).train()
    hb.clear_pack_cache()
    be = ops.HipBackend()
    hb.begin_step(torch.device(DEV))
    z = be.conv_bn_act(conv, bn, _to_dev_nhwc(x), relu=True)
    be.end_forward()
    torch.cuda.synchronize()
    assert not hb._PENDING_STATS                 # consumed by the normalisation
    check_close("fused conv-bn", nchw(z.float()), zr, 2e-2, 6e-3)
    check_close("fused running_mean", bn.running_mean, rm, 2e-3, 2e-3)
    check_close("fused running_var", bn.running_var, rv, 2e-3, 2e-3)
    assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("C,B,H,W", [(48, 1, 37, 45), (64, 2, 20, 33), (96, 1, 64, 64), (192, 1, 21, 40), (384, 1, 9, 33)])
def test_wgrad_tile_kernel(C, B, H, W):
    """Halo-staged weight gradient (conv_wgrad_tile.hip, ds_read_b64_tr_b16 fragments):
    every channel configuration against the oracle, through the C ABI (the host glue routes the
    trunk's 3x3 weight gradients here, grouped: tests/test_group_gpu.py)."""
    import ctypes
    from oracle import ops as O
    from semseg_amd._lib import lib, check, ConvDesc
    x = _rand(B, C, H, W, seed=41)
    gy = _rand(B, C, H, W, seed=42)
    w = torch.zeros(C, C, 3, 3, requires_grad=True)
    O.conv2d(x, w, None, 1, 1, 1).backward(gy)
    xd = _to_dev_nhwc(x)
    gd = nhwc(gy).to(DEV).to(ACT_DTYPE).contiguous()
    d = ConvDesc(B, H, W, C, C, H, W, C, C, 3, 3, 1, 1, 1, 0, 0, 0, -1)
    ns, ws = ctypes.c_int(0), ctypes.c_size_t(0)
    L = lib()
    check(L.ssa_conv2d_wgrad_tile_plan(ctypes.byref(d), C, ctypes.byref(ns), ctypes.byref(ws)), "plan")
    part = torch.empty(ws.value // 4, dtype=torch.float32, device=DEV)
    dw = torch.empty(C, C, 3, 3, dtype=torch.float32, device=DEV)
    P = ctypes.c_void_p
    check(L.ssa_conv2d_wgrad_tile(ctypes.byref(d), P(xd.data_ptr()), P(gd.data_ptr()), C, C, ns.value,
                                  P(part.data_ptr()), None), "ssa_conv2d_wgrad_tile")
    check(L.ssa_conv2d_wgrad_reduce(P(part.data_ptr()), ns.value, C, C, C, C, 3, 3, P(dw.data_ptr()), 0, None),
          "ssa_conv2d_wgrad_reduce")
    torch.cuda.synchronize()
    check_close("wgrad tile C=%d" % C, dw, w.grad, 2e-3, 5e-4)


def test_wgrad_tile_grouped_launch_of_twenty_layers():
    """One grouped launch carries up to 32 weight-gradient problems (csrc/group.h MAXJOBS of ConvWgradTile; 16 for every
    other kernel): twenty 48-channel layers of different sizes inside one bracket -> ONE tile launch, one reduce launch
    per 16 parameters, every layer's gradient against the oracle."""
    import ctypes
    from oracle import ops as O
    from semseg_amd._lib import lib, check, ConvDesc
    hb = _hb()
    C, n = 48, 20
    L = lib()
    P = ctypes.c_void_p
    keep, want = [], []
    plans = []
    for i in range(n):
        H, W = 5 + (i % 4) * 3, 33 + 7 * (i % 3)
        x = _rand(1, C, H, W, seed=300 + i)
        gy = _rand(1, C, H, W, seed=400 + i)
        w = torch.zeros(C, C, 3, 3, requires_grad=True)
        O.conv2d(x, w, None, 1, 1, 1).backward(gy)
        want.append(w.grad)
        xd, gd = _to_dev_nhwc(x), nhwc(gy).to(DEV).to(ACT_DTYPE).contiguous()
        d = ConvDesc(1, H, W, C, C, H, W, C, C, 3, 3, 1, 1, 1, 0, 0, 0, 2)        # strips of 2 tiles: several partials
        ns, ws = ctypes.c_int(0), ctypes.c_size_t(0)
        check(L.ssa_conv2d_wgrad_tile_plan(ctypes.byref(d), C, ctypes.byref(ns), ctypes.byref(ws)), "plan")
        part = torch.empty(ws.value // 4, dtype=torch.float32, device=DEV)
        dw = torch.empty(C, C, 3, 3, dtype=torch.float32, device=DEV)
        keep += [xd, gd, part]
        plans.append((d, xd, gd, ns.value, part, dw))
    L.ssa_launch_count(1)
    with hb.group():
        for d, xd, gd, ns, part, dw in plans:
            check(L.ssa_conv2d_wgrad_tile(ctypes.byref(d), P(xd.data_ptr()), P(gd.data_ptr()), C, C, ns,
                                          P(part.data_ptr()), None), "ssa_conv2d_wgrad_tile")
    n_tile = L.ssa_launch_count(1)
    with hb.group():
        for d, xd, gd, ns, part, dw in plans:
            check(L.ssa_conv2d_wgrad_reduce(P(part.data_ptr()), ns, C, C, C, C, 3, 3, P(dw.data_ptr()), 0, None),
                  "ssa_conv2d_wgrad_reduce")
    n_red = L.ssa_launch_count(1)
    torch.cuda.synchronize()
    assert n_tile == 1 and n_red == 2, (n_tile, n_red)
    for i, (pl, ref) in enumerate(zip(plans, want)):
        check_close("grouped wgrad layer %d" % i, pl[5], ref, 2e-3, 5e-4)


@pytest.mark.parametrize("Cin,Cout,k,stride,H,W", [(48, 96, 3, 2, 50, 70), (64, 256, 1, 1, 33, 47), (96, 48, 1, 1, 20, 24)])
def test_conv_bn_fused_stats_igemm(Cin, Cout, k, stride, H, W):
    """Same as test_conv_bn_fused_stats for the shapes that run on the K-pipelined igemm kernel
    (strided 3x3 and small 1x1 convs of the fuse layers / layer1): statistics from its epilogue."""
    from oracle import ops as O
    from semseg_amd import ops, nn as snn
    hb = _hb()
    B = 2
    x = _rand(B, Cin, H, W, seed=51)
    conv = snn.Conv2d(Cin, Cout, k, stride, k // 2, bias=False)
    bn = snn.BatchNorm2d(Cout)
    with torch.no_grad():
        conv.weight.copy_(_rand(Cout, Cin, k, k, seed=52, scale=0.05))
        bn.weight.copy_(torch.rand(Cout) + 0.5)
        bn.bias.copy_(torch.randn(Cout) * 0.1)
    rm, rv = torch.zeros(Cout), torch.ones(Cout)
    yr = O.conv2d(x, conv.weight.detach(), None, stride, k // 2, 1)
    zr = O.batch_norm(bf16_round(yr), bn.weight.detach(), bn.bias.detach(), rm, rv, True, 0.1, 1e-5)
    conv, bn = conv.to(DEV), bn.to(DEV).train()
    hb.clear_pack_cache()
    be = ops.HipBackend()
    hb.begin_step(torch.device(DEV))
    z = be.conv_bn_act(conv, bn, _to_dev_nhwc(x), relu=False)
    be.end_forward()
    torch.cuda.synchronize()
    assert not hb._PENDING_STATS
    check_close("fused igemm conv-bn", nchw(z.float()), zr, 2e-2, 6e-3)
    check_close("fused igemm running_mean", bn.running_mean, rm, 2e-3, 2e-3)
    check_close("fused igemm running_var", bn.running_var, rv, 2e-3, 2e-3)


def test_batched_filter_repack():
    """refresh_packed_filters (one launch for all stale filters) == per-filter packing."""
    hb = _hb()
    hb.clear_pack_cache()
    ws = [torch.randn(48, 48, 3, 3, device=DEV), torch.randn(19, 512, 1, 1, device=DEV),
          torch.randn(96, 48, 3, 3, device=DEV), torch.randn(64, 3, 3, 3, device=DEV),
          torch.randn(512, 720, 3, 3, device=DEV), torch.randn(40, 300, 1, 1, device=DEV),
          torch.randn(24, 3, 7, 7, device=DEV), torch.randn(384, 192, 3, 3, device=DEV)]
    specs = [(0, 48, 0), (1, 0, 48), (0, 512, 0), (1, 0, 24), (0, 48, 0), (1, 0, 96), (0, 16, 0),
             (2, 48, 0), (3, 0, 48), (2, 512, 0), (2, 48, 0), (3, 0, 96), (2, 16, 0),     # fragment-major forms
             (0, 720, 0), (1, 0, 512), (2, 720, 0), (3, 0, 512), (0, 304, 0), (1, 0, 40), (0, 8, 0), (1, 0, 24),
             (0, 192, 0), (1, 0, 384), (2, 192, 0), (3, 0, 384)]
    owners = [0, 0, 1, 1, 2, 2, 3, 0, 0, 1, 2, 2, 3, 4, 4, 4, 4, 5, 5, 6, 6, 7, 7, 7, 7]
    first = [hb._packed_filter(ws[o], *sp)[0] for o, sp in zip(owners, specs)]
    for w in ws:
        w.mul_(-0.5).add_(0.25)                # in-place update, like an optimizer step
    hb.refresh_packed_filters()
    torch.cuda.synchronize()
    tab, = hb._JOB_TABLES.values()
    assert tab["tiles"] is not None and 300 < tab["ntiles"] < 600   # the tile-balanced kernel ran, ONE tile list per
    # source tensor: the 25 operand forms of the 8 tensors are chained (600+ tiles if every form fetched its own)
    batched = [t.clone() for t in first]       # same persistent buffers, refreshed in place
    saved = [w.clone() for w in ws]
    for w in ws:
        w.mul_(2.0).sub_(0.125)
    hb.refresh_packed_filters()
    torch.cuda.synchronize()
    updated = [t.clone() for t in first]
    for w in ws:
        w.add_(0.0)                                          # version bump only
    hb.refresh_packed_filters()
    torch.cuda.synchronize()
    for o, sp, got, one in zip(owners, specs, updated, first):
        assert torch.equal(got.view(torch.int16), one.view(torch.int16)), ("re-pack of unchanged weights", o, sp)
    assert any(not torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(updated, batched))
    for w, w1 in zip(ws, saved):
        w.copy_(w1)
    hb.refresh_packed_filters()
    torch.cuda.synchronize()
    for got, b0 in zip(first, batched):
        assert torch.equal(got.view(torch.int16), b0.view(torch.int16))
    hb.clear_pack_cache()
    for o, sp, got in zip(owners, specs, batched):
        want = hb._packed_filter(ws[o], *sp)[0]
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (o, sp)
    hb.clear_pack_cache()


def test_conv_channel_slice_input():
    """Input given as a channel slice of a wider NHWC buffer (ld > C)."""
    from oracle import ops as O
    hb = _hb()
    B, H, W = 1, 20, 24
    full = _rand(B, 96, H, W, seed=5)
    w = _rand(64, 48, 3, 3, seed=6, scale=0.05)
    yr = O.conv2d(full[:, 48:96], w, None, 1, 1, 1)
    fd = _to_dev_nhwc(full)
    hb.clear_pack_cache()
    y = hb.Conv2dFn.apply(fd[..., 48:96], w.to(DEV), None, 1, 1, 1, False)
    torch.cuda.synchronize()
    check_close("conv slice", nchw(y.float()), yr)


# --------------------------------------------------------------------- BN
@pytest.mark.parametrize("C,relu,res,post", [(48, True, True, False), (96, True, False, False),
                                             (720, True, False, False), (256, False, False, False),
                                             (512, True, False, True)])
def test_bn_train(C, relu, res, post):
    from oracle import ops as O
    hb = _hb()
    B, H, W = 2, 17, 23
    x = _rand(B, C, H, W, seed=1) * 1.7 + 0.3
    x = bf16_round(x)
    gamma = torch.rand(C) + 0.5
    beta = torch.randn(C) * 0.1
    r = _rand(B, C, H, W, seed=2) if res else None
    pm = None
    if post:
        pm = (torch.rand(B, C) > 0.3).float() / 0.7
    rm, rv = torch.zeros(C), torch.ones(C)
    xr = x.clone().requires_grad_(True)
    gr = gamma.clone().requires_grad_(True)
    br = beta.clone().requires_grad_(True)
    rr = r.clone().requires_grad_(True) if res else None
    y = O.batch_norm(xr, gr, br, rm, rv, True, 0.1, 1e-5)
    if res:
        y = y + rr
    if relu:
        y = torch.relu(y)
    if post:
        y = y * pm[:, :, None, None]
    gy = _rand(B, C, H, W, seed=3)
    y.backward(gy)

    xd = _to_dev_nhwc(x).requires_grad_(True)
    gd = gamma.to(DEV).requires_grad_(True)
    bd = beta.to(DEV).requires_grad_(True)
    rd = _to_dev_nhwc(r).requires_grad_(True) if res else None
    rmd, rvd = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    pmd = pm.to(DEV) if post else None
    nbt = torch.zeros((), dtype=torch.long, device=DEV)
    z = hb.BatchNormActFn.apply(xd, gd, bd, rd, pmd, rmd, rvd, nbt, 0.1, 1e-5, True, relu, False, None)
    z.backward(nhwc(gy).to(DEV).to(ACT_DTYPE))
    torch.cuda.synchronize()
    check_close("bn_fwd", nchw(z.float()), y)
    check_close("bn_running_mean", rmd, rm, 1e-4, 1e-4)
    check_close("bn_running_var", rvd, rv, 1e-4, 1e-4)
    assert int(nbt) == 1
    check_close("bn_dx", nchw(xd.grad.float()), xr.grad, 2e-2, 6e-3)
    check_close("bn_dgamma", gd.grad, gr.grad, 1e-2, 4e-3)
    check_close("bn_dbeta", bd.grad, br.grad, 1e-2, 4e-3)
    if res:
        check_close("bn_dres", nchw(rd.grad.float()), rr.grad)


def test_bn_deferred_running_stats_two_passes():
    """Two training passes over one BatchNorm layer (the 0.5x and the 1.0x pass, problems of one
    grouped launch): the deferred batched update must equal the reference's sequential in-place
    updates, in issue order."""
    from oracle import ops as O
    from semseg_amd import ops, nn as snn
    hb = _hb()
    C = 48
    bn = snn.BatchNorm2d(C, momentum=0.1)
    rm, rv = torch.randn(C) * 0.1, torch.rand(C) + 0.5
    with torch.no_grad():
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    xa, xb = _rand(1, C, 12, 20, seed=21), _rand(2, C, 24, 40, seed=22) * 2.0 + 0.5
    one = torch.ones(C)
    zero = torch.zeros(C)
    O.batch_norm(xa, one, zero, rm, rv, True, 0.1, 1e-5)
    O.batch_norm(xb, one, zero, rm, rv, True, 0.1, 1e-5)
    bn = bn.to(DEV).train()
    be = ops.HipBackend()
    hb.begin_step(torch.device(DEV))
    be.batch_norm_act([_to_dev_nhwc(xa), _to_dev_nhwc(xb)], bn)
    be.end_forward()
    torch.cuda.synchronize()
    check_close("deferred running_mean", bn.running_mean, rm, 1e-4, 1e-4)
    check_close("deferred running_var", bn.running_var, rv, 1e-4, 1e-4)
    assert int(bn.num_batches_tracked) == 2


def test_bn_eval():
    from oracle import ops as O
    hb = _hb()
    B, C, H, W = 1, 64, 9, 11
    x = _rand(B, C, H, W, seed=1)
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C) * 0.1
    rm, rv = torch.randn(C) * 0.2, torch.rand(C) + 0.5
    y = torch.relu(O.batch_norm(x, gamma, beta, rm.clone(), rv.clone(), False))
    z = hb.BatchNormActFn.apply(_to_dev_nhwc(x), gamma.to(DEV), beta.to(DEV), None, None, rm.to(DEV),
                                rv.to(DEV), None, 0.1, 1e-5, False, True, False)
    torch.cuda.synchronize()
    check_close("bn_eval", nchw(z.float()), y)


def test_bn_eval_coefficient_registry():
    """Inference forwards take their BatchNorm coefficients from persistent buffers: computed singly the first time a
    layer is seen, refreshed by ONE batched launch at the next begin_step -- and never stale: running statistics and
    affine parameters changed between two forwards (as a training step does, through raw pointers: no version counter
    moves) reach the next forward; under autograd the registry is not used."""
    from oracle import ops as O
    hb = _hb()
    B, H, W = 1, 7, 9
    layers = []
    for k, C in enumerate((48, 64, 720)):
        g = torch.Generator().manual_seed(40 + k)
        layers.append(dict(C=C, x=_rand(B, C, H, W, seed=50 + k), gamma=torch.rand(C, generator=g) + 0.5,
                           beta=torch.randn(C, generator=g) * 0.1, rm=torch.randn(C, generator=g) * 0.2,
                           rv=torch.rand(C, generator=g) + 0.5))
    for l in layers:
        l["dev"] = {k: l[k].to(DEV) for k in ("gamma", "beta", "rm", "rv")}
        l["xd"] = _to_dev_nhwc(l["x"])

    def forward():
        hb.begin_step()
        with torch.no_grad():
            return [hb.BatchNormActFn.apply(l["xd"], l["dev"]["gamma"], l["dev"]["beta"], None, None, l["dev"]["rm"],
                                            l["dev"]["rv"], None, 0.1, 1e-5, False, True, False) for l in layers]

    def check(zs, tag):
        torch.cuda.synchronize()
        for l, z in zip(layers, zs):
            d = l["dev"]
            want = torch.relu(O.batch_norm(l["x"], d["gamma"].cpu(), d["beta"].cpu(), d["rm"].cpu().clone(), d["rv"].cpu().clone(), False))
            check_close("bn_eval registry %s C=%d" % (tag, l["C"]), nchw(z.float()), want)

    reg = hb._BN_EVAL
    z1 = forward()                                   # first sight: single launches, registered
    check(z1, "first")
    mine = [l["dev"]["rm"] for l in layers]
    assert sum(any(e[0]() is t for t in mine) for e in reg.entries.values()) == 3
    z2 = forward()                                   # the batched refresh
    check(z2, "batched")
    assert reg.table is not None and all(e[5] == reg.gen for e in reg.entries.values())
    for a, b in zip(z1, z2):
        assert torch.equal(a, b)
    for l in layers:                                 # what a training step does to a layer, behind autograd's back
        d = l["dev"]
        d["rm"].data.mul_(1.5).add_(0.1)
        d["rv"].data.mul_(0.5).add_(0.2)
        d["gamma"].data.mul_(-0.75)
    z3 = forward()
    check(z3, "after an update")
    assert not torch.equal(z3[0], z2[0])
    hb.begin_step()                                  # a forward that used no inference BatchNorm (a training forward) ...
    hb.begin_step()
    for l in layers:
        l["dev"]["beta"].data.add_(0.25)
    check(forward(), "after a training forward")    # ... then the single launches again, still current
    # under autograd: fresh coefficients per call, the registry untouched
    uses = reg.uses
    xg = layers[0]["xd"].clone().requires_grad_(True)
    d = layers[0]["dev"]
    z = hb.BatchNormActFn.apply(xg, d["gamma"], d["beta"], None, None, d["rm"], d["rv"], None, 0.1, 1e-5, False, True, False)
    assert z.requires_grad and reg.uses == uses


# ---------------------------------------------------------------- pooling
@pytest.mark.parametrize("B,C,H,W", [(2, 64, 48, 64), (1, 64, 33, 47), (1, 8, 5, 7)])
def test_maxpool3x3s2(B, C, H, W):
    """ResNet stem pooling on post-ReLU data (many exact ties at zero): values and
    the gradient routing must match PyTorch's first-maximum rule."""
    from oracle import ops as O
    hb = _hb()
    x = torch.relu(_rand(B, C, H, W, seed=31))
    xr = x.clone().requires_grad_(True)
    yr = O.max_pool_3x3_s2(xr)
    gy = _rand(*yr.shape, seed=32)
    yr.backward(gy)
    xd = _to_dev_nhwc(x).requires_grad_(True)
    yd = hb.MaxPool3x3s2Fn.apply(xd)
    yd.backward(nhwc(gy).to(DEV).to(ACT_DTYPE))
    torch.cuda.synchronize()
    assert torch.equal(nchw(yd.float()).cpu(), yr.detach())
    check_close("maxpool dx", nchw(xd.grad.float()), xr.grad, 1e-2, 4e-3)


def test_global_avg_pool():
    from oracle import ops as O
    hb = _hb()
    x = _rand(2, 2048, 12, 16, seed=33)
    xr = x.clone().requires_grad_(True)
    yr = O.global_avg_pool(xr)
    gy = _rand(*yr.shape, seed=34)
    yr.backward(gy)
    xd = _to_dev_nhwc(x).requires_grad_(True)
    yd = hb.GlobalAvgPoolFn.apply(xd)
    yd.backward(nhwc(gy).to(DEV).to(ACT_DTYPE))
    torch.cuda.synchronize()
    check_close("gap fwd", nchw(yd.float()), yr)
    check_close("gap dx", nchw(xd.grad.float()), xr.grad)


# --------------------------------------------------------------- bilinear
@pytest.mark.parametrize("C,hi,wi,ho,wo,f32", [(48, 16, 20, 64, 80, False), (96, 15, 9, 30, 18, False),
                                               (19, 32, 32, 128, 128, True), (1, 24, 40, 96, 160, True),
                                               (19, 64, 64, 32, 32, True), (192, 8, 8, 64, 64, False),
                                               (19, 33, 45, 67, 91, True),
                                               # dense few-channel fp32 upsampling: the LDS-staged row pass of the separable
                                               # backward (65 = Mapillary; rows of several segments at 2x and 4x; a ratio that
                                               # is not an integer)
                                               (65, 12, 20, 48, 80, True), (19, 6, 1100, 12, 2200, True),
                                               (19, 5, 400, 20, 1600, True), (19, 8, 12, 21, 31, True)])
def test_bilinear(C, hi, wi, ho, wo, f32):
    from oracle import ops as O
    hb = _hb()
    B = 2
    x = _rand(B, C, hi, wi, seed=1)
    xr = x.clone().requires_grad_(True)
    y = O.bilinear(xr, (ho, wo))
    gy = _rand(B, C, ho, wo, seed=2)
    y.backward(gy)
    xd = nhwc(x).to(DEV)
    gyd = nhwc(gy).to(DEV)
    if not f32:
        xd, gyd = xd.to(ACT_DTYPE), gyd.to(ACT_DTYPE)
    xd.requires_grad_(True)
    yd = hb.BilinearFn.apply(xd, ho, wo, f32)
    yd.backward(gyd)
    torch.cuda.synchronize()
    tol = (1e-5, 1e-5) if f32 else (1e-2, 4e-3)
    check_close("bilinear_fwd", nchw(yd.float()), y, *tol)
    check_close("bilinear_bwd", nchw(xd.grad.float()), xr.grad, *tol)


def test_image_resize():
    from oracle import ops as O
    hb = _hb()
    x = torch.randn(2, 3, 64, 96)
    y = hb.image_to_nhwc(x.to(DEV), None)
    torch.cuda.synchronize()
    check_close("image copy", nchw(y.float())[:, :3], bf16_round(x), 1e-6, 1e-6)
    assert float(y[..., 3:].abs().max()) == 0.0
    y2 = hb.image_to_nhwc(x.to(DEV), (32, 48))
    torch.cuda.synchronize()
    check_close("image resize", nchw(y2.float())[:, :3], O.resize_x(x, 0.5), 1e-2, 4e-3)


def test_sum_act():
    hb = _hb()
    ts = [_rand(2, 12, 10, 48, seed=i) for i in range(3)]
    tr = [t.clone().requires_grad_(True) for t in ts]
    y = torch.relu(tr[0] + tr[1] + tr[2])
    gy = _rand(2, 12, 10, 48, seed=9)
    y.backward(gy)
    td = [t.to(DEV).to(ACT_DTYPE).requires_grad_(True) for t in ts]
    z = hb.SumActFn.apply(True, *td)
    z.backward(gy.to(DEV).to(ACT_DTYPE))
    torch.cuda.synchronize()
    check_close("sum_act", z.float(), y)
    for i in range(3):
        check_close("sum_act_grad%d" % i, td[i].grad.float(), tr[i].grad)


# -------------------------------------------------------------------- OCR
def _ocr_gather_case(K, H, W):
    from oracle import ops as O
    hb = _hb()
    B, C = 2, 512
    feats = _rand(B, C, H, W, seed=1)
    logits = torch.randn(B, K, H, W) * 2.0
    fr = feats.clone().requires_grad_(True)
    lr = logits.clone().requires_grad_(True)
    ctx = O.spatial_gather(fr, lr)            # [B,C,K,1]
    g = torch.randn(B, C, K, 1)
    ctx.backward(g)
    fd = _to_dev_nhwc(feats).requires_grad_(True)
    ld = nhwc(logits).to(DEV).requires_grad_(True)
    out = hb.OcrGatherFn.apply(fd, ld)        # [B,K,C]
    out.backward(g[..., 0].permute(0, 2, 1).contiguous().to(DEV))
    torch.cuda.synchronize()
    check_close("gather_fwd", out.permute(0, 2, 1), ctx[..., 0], 1e-2, 4e-3)
    check_close("gather_dfeats", nchw(fd.grad.float()), fr.grad, 2e-2, 6e-3)
    check_close("gather_dlogits", nchw(ld.grad), lr.grad, 2e-2, 8e-3)


def test_ocr_gather():
    _ocr_gather_case(19, 24, 28)


def test_ocr_gather_65_classes():
    """Mapillary's 65 regions (padded to 96 in the probability operand) over a ragged 13 x 21 = 273 pixels: softmax
    over HW per class, the context product and both gradients (ssa_softmax_hw_* and the row dots)."""
    _ocr_gather_case(65, 13, 21)


@pytest.mark.parametrize("K,H,W,fused", [(19, 20, 24, True), (65, 9, 31, True), (19, 3, 5, True), (96, 8, 16, True),
                                          (19, 20, 24, False), (150, 6, 11, True)])
def test_ocr_attention(K, H, W, fused, monkeypatch):
    """ObjectAttentionBlock's softmax(q k^T / sqrt(256)) v (network/ocr_utils.py:100-113): the fused kernel
    (csrc/ocr_attn.hip; 19 = Cityscapes, 65 = Mapillary -> 3 region blocks, 96 = its limit, pixel counts that are not
    multiples of the 128-pixel workgroup tile) and the three-launch form (forced, and what 150 regions fall back to)."""
    from oracle import ops as O
    hb = _hb()
    monkeypatch.setattr(hb, "_OCR_ATTN_FUSED", fused)
    B, D = 2, 256
    q = _rand(B, H * W, D, seed=1)
    k = _rand(B, K, D, seed=2)
    v = _rand(B, K, D, seed=3)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = O.object_attention(qr, kr.permute(0, 2, 1), vr, D)
    g = _rand(B, H * W, D, seed=4)
    out.backward(g)
    qd = q.view(B, H, W, D).to(DEV).to(ACT_DTYPE).requires_grad_(True)
    kd = k.to(DEV).to(ACT_DTYPE).requires_grad_(True)
    vd = v.to(DEV).to(ACT_DTYPE).requires_grad_(True)
    od = hb.OcrAttnFn.apply(qd, kd, vd, D ** -0.5)
    od.backward(g.view(B, H, W, D).to(DEV).to(ACT_DTYPE))
    torch.cuda.synchronize()
    # one rounding of the output (the probabilities are rounded to 16 bit on both paths before the second product)
    check_close("attn_fwd", od.float().view(B, H * W, D), out, 1e-2, 4e-3)
    check_close("attn_dq", qd.grad.float().view(B, H * W, D), qr.grad, 3e-2, 1.5e-2)
    check_close("attn_dk", kd.grad.float(), kr.grad, 3e-2, 1.5e-2)
    check_close("attn_dv", vd.grad.float(), vr.grad, 2e-2, 8e-3)


# ----------------------------------------------------------------- fusion
@pytest.mark.parametrize("shape", [(2, 16, 20, 19), (1, 5, 7, 19), (1, 9, 30, 3), (1, 4, 70, 65)])
def test_scale_fusion_ops(shape):
    hb = _hb()
    B, H, W, C = shape      # ragged last block of the 256-pixel tile kernel; 65 classes: the wave-per-pixel kernel
    a = torch.rand(B, H, W, 1)
    lo = torch.randn(B, H, W, C)
    hi = torch.randn(B, H, W, C)
    x = torch.randn(B, H, W, 1)
    ar, lor, hir, xr = (t.clone().requires_grad_(True) for t in (a, lo, hi, x))
    s = torch.sigmoid(xr)
    m = ar * lor
    j = m + (1 - s) * hir
    gj = torch.randn(B, H, W, C)
    j.backward(gj)
    ad, lod, hid, xd = (t.to(DEV).requires_grad_(True) for t in (a, lo, hi, x))
    sd = hb.SigmoidFn.apply(xd)
    md = hb.BcastMulFn.apply(ad, lod)
    jd = hb.AttnBlendFn.apply(md, sd, hid)
    jd.backward(gj.to(DEV))
    torch.cuda.synchronize()
    check_close("fusion_fwd", jd, j, 1e-5, 1e-5)
    for n, d, r in (("a", ad, ar), ("lo", lod, lor), ("hi", hid, hir), ("x", xd, xr)):
        check_close("fusion_d" + n, d.grad, r.grad, 1e-4, 1e-4)


# ------------------------------------------------------------------ losses
def _labels(B, H, W, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    blocks = torch.randint(0, C, (B, (H + 7) // 8, (W + 7) // 8), generator=g)
    lab = blocks.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W].clone()
    ign = torch.rand(B, H, W, generator=g) < 0.1
    lab[ign] = 255
    return lab.long()


def test_cross_entropy():
    from oracle import ops as O
    hb = _hb()
    B, C, H, W = 2, 19, 40, 56
    logits = torch.randn(B, C, H, W) * 3
    lab = _labels(B, H, W, C)
    lr = logits.clone().requires_grad_(True)
    loss = O.cross_entropy(lr, lab, 255)
    (loss * 1.7).backward()
    ld = nhwc(logits).to(DEV).requires_grad_(True)
    out = hb.CrossEntropyFn.apply(ld, lab.to(DEV), 255)
    (out * 1.7).backward()
    torch.cuda.synchronize()
    check_close("ce", out.view(1), loss.view(1), 1e-5, 1e-5)
    check_close("ce_grad", nchw(ld.grad), lr.grad, 1e-4, 1e-4)


# (2, 64, 96): dense, element count a multiple of four -- the forward saves no gradient, the backward recomputes it
# (ssa_bce_bwd / inside ssa_rmi_bwd_logits_bce); (1, 65, 97): an odd pixel count -- the saved-gradient path
@pytest.mark.parametrize("shape", [(2, 64, 96), (1, 65, 97)])
@pytest.mark.parametrize("do_rmi", [False, True])
def test_bce_rmi(do_rmi, shape):
    from oracle import ops as O
    hb = _hb()
    C = 19
    B, H, W = shape
    logits = torch.randn(B, C, H, W) * 2
    lab = _labels(B, H, W, C, seed=3)
    lr = logits.clone().requires_grad_(True)
    loss = O.rmi_loss(lr, lab, C, do_rmi=do_rmi)
    (loss * 0.4).backward()
    ld = nhwc(logits).to(DEV).requires_grad_(True)
    out = hb.BceRmiFn.apply(ld, lab.to(DEV), do_rmi, 0.5)
    (out * 0.4).backward()
    torch.cuda.synchronize()
    check_close("bce_rmi(%s)" % do_rmi, out.view(1), loss.view(1), 1e-4, 1e-4)
    check_close("bce_rmi_grad(%s)" % do_rmi, nchw(ld.grad), lr.grad, 2e-3, 1e-3)


# Class counts beyond Cityscapes' 19 (Mapillary: 65 classes, ignore label 65 = C, out of range like 255), label edges,
# saturated logits and the fp16 step's loss-scaled upstream gradient (65536 at the start of apex-style dynamic scaling).
def _label_map(kind, B, H, W, C, ign, seed=0):
    """`blocks8`: random 8 x 8 blocks with 10 % scattered ignore; `blocks`: large blocks (a quarter of the crop's
    height) with an ignored band, as real scenes have; `single`: one class everywhere but a few ignored pixels;
    `ignored`: every pixel ignored."""
    g = torch.Generator().manual_seed(seed)
    if kind == "blocks8":
        lab = _labels(B, H, W, C, seed=seed)
        lab[lab == 255] = ign
        return lab
    if kind == "blocks":
        bs = max(4, H // 4)
        blocks = torch.randint(0, C, (B, (H + bs - 1) // bs, (W + bs - 1) // bs), generator=g)
        lab = blocks.repeat_interleave(bs, 1).repeat_interleave(bs, 2)[:, :H, :W].clone()
        lab[:, :, W // 3:W // 3 + 3] = ign
        return lab.long()
    if kind == "single":
        lab = torch.full((B, H, W), int(torch.randint(0, C, (1,), generator=g)), dtype=torch.long)
        lab[:, 0, :3] = ign
        return lab
    assert kind == "ignored"
    return torch.full((B, H, W), ign, dtype=torch.long)


def _logits_on_device(logits, sliced):
    """NHWC fp32 on the device: dense, or (sliced) channels 2..C+1 of a wider NHWC buffer (ld = C + 5)."""
    x = nhwc(logits)
    if not sliced:
        return x.to(DEV).requires_grad_(True)
    B, H, W, C = x.shape
    wide = torch.randn(B, H, W, C + 5)
    wide[..., 2:2 + C] = x
    return wide.to(DEV).requires_grad_(True)


def _grad_of(ld, C, sliced):
    g = ld.grad[..., 2:2 + C] if sliced else ld.grad
    if sliced:      # nothing outside the slice is touched
        assert float(ld.grad[..., :2].abs().max()) == 0.0 and float(ld.grad[..., 2 + C:].abs().max()) == 0.0
    return nchw(g.contiguous())


def _fwd_input(ld, C, sliced):
    return ld[..., 2:2 + C] if sliced else ld


@pytest.mark.parametrize("scale,up", [(3.0, 1.7), (60.0, 65536.0), (3.0, 65536.0), (60.0, 1.7)])
@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("ign", ["255", "C"])
@pytest.mark.parametrize("C", [19, 65, 128])
def test_cross_entropy_classes(C, ign, sliced, scale, up):
    """ssa_ce_fwd at 19 / 65 / 128 classes (from 65 the [256][C] tile needs the raised LDS limit), ignore label 255 or
    C, B = 2 with 2 x 17 x 23 = 782 pixels (not a multiple of the 256-pixel tile), logits dense or a channel slice of a
    wider NHWC buffer, moderate and saturated logits (logsumexp at |x| ~ 60 x 4), upstream 1.7 or the loss scale."""
    from oracle import ops as O
    hb = _hb()
    B, H, W = 2, 17, 23
    ign = 255 if ign == "255" else C
    g = torch.Generator().manual_seed(C + int(scale))
    logits = torch.randn(B, C, H, W, generator=g) * scale
    lab = _label_map("blocks8", B, H, W, C, ign, seed=C)
    lr = logits.clone().requires_grad_(True)
    loss = O.cross_entropy(lr, lab, ign)
    (loss * up).backward()
    assert torch.isfinite(loss) and torch.isfinite(lr.grad).all()
    ld = _logits_on_device(logits, sliced)
    out = hb.CrossEntropyFn.apply(_fwd_input(ld, C, sliced), lab.to(DEV), ign)
    (out * up).backward()
    torch.cuda.synchronize()
    check_close("ce", out.view(1), loss.view(1), 1e-5, 1e-5)
    check_close("ce_grad", _grad_of(ld, C, sliced), lr.grad, 1e-4, 1e-4)


@pytest.mark.parametrize("C", [19, 65])
def test_cross_entropy_fully_ignored(C):
    """Every label ignored: the reference's nll_loss mean over zero pixels is NaN and its gradient is zero; the
    kernels give the same (not 0 * inf in the gradient)."""
    from oracle import ops as O
    hb = _hb()
    B, H, W = 2, 9, 13
    logits = torch.randn(B, C, H, W) * 3
    lab = _label_map("ignored", B, H, W, C, C)
    lr = logits.clone().requires_grad_(True)
    loss = O.cross_entropy(lr, lab, C)
    (loss * 1.7).backward()
    ld = nhwc(logits).to(DEV).requires_grad_(True)
    out = hb.CrossEntropyFn.apply(ld, lab.to(DEV), C)
    (out * 1.7).backward()
    torch.cuda.synchronize()
    assert torch.isnan(loss) and torch.isnan(out.cpu())
    assert torch.equal(nchw(ld.grad).cpu(), lr.grad), float((nchw(ld.grad).cpu() - lr.grad).abs().max())


def _bce_rmi_case(B, C, H, W, route, ign, kind, scale, up, do_rmi, seed=0):
    """BceRmiFn against oracle.ops.rmi_loss.  route "dense": the forward saves no gradient, the backward recomputes it;
    "slice" (ld != C) and "odd" (P * C % 4 != 0): the forward saves the un-normalised gradient.  The route is asserted."""
    from oracle import ops as O
    hb = _hb()
    sliced = route == "slice"
    if route == "odd":
        assert (B * H * W * C) % 4, (B, H, W, C)
    g = torch.Generator().manual_seed(1000 * seed + C)
    logits = torch.randn(B, C, H, W, generator=g) * scale
    lab = _label_map(kind, B, H, W, C, ign, seed=seed + 3)
    lr = logits.clone().requires_grad_(True)
    loss = O.rmi_loss(lr, lab, C, do_rmi=do_rmi)
    (loss * up).backward()
    # the cases stay where the reference's Cholesky is defined
    assert torch.isfinite(loss) and torch.isfinite(lr.grad).all(), "oracle not finite"
    ld = _logits_on_device(logits, sliced)
    out = hb.BceRmiFn.apply(_fwd_input(ld, C, sliced), lab.to(DEV), do_rmi, 0.5)
    assert out.grad_fn.recompute == (route == "dense"), (route, out.grad_fn.recompute)
    (out * up).backward()
    torch.cuda.synchronize()
    check_close("bce_rmi(%s)" % do_rmi, out.view(1), loss.view(1), 1e-4, 1e-4)
    check_close("bce_rmi_grad(%s)" % do_rmi, _grad_of(ld, C, sliced), lr.grad, 2e-3, 1e-3)


# (C, route): every class count with the dense route and a saved-gradient route; P * C is odd-free at 128 classes
_BCE_ROUTES = [(C, r) for C in (19, 30, 31, 65, 128) for r in ("dense", "slice", "odd") if not (C == 128 and r == "odd")]


@pytest.mark.parametrize("do_rmi", [False, True])
@pytest.mark.parametrize("ign", ["255", "C"])
@pytest.mark.parametrize("C,route", _BCE_ROUTES)
def test_bce_rmi_classes(C, route, ign, do_rmi):
    """19 / 30 classes: one chunk of the RMI pool; 31 / 65 / 128: two, three and five chunks."""
    H, W = (19, 27) if route == "odd" else (20, 28)
    _bce_rmi_case(1, C, H, W, route, 255 if ign == "255" else C, "blocks8", 2.0, 0.4, do_rmi)


# H and W through every remainder mod 4 (the pool pads by 2), the smallest pooled grid (H = 8: Hp = 3), B = 2
@pytest.mark.parametrize("do_rmi", [False, True])
@pytest.mark.parametrize("C", [19, 65])
@pytest.mark.parametrize("B,H,W", [(2, 8, 13), (1, 9, 22), (2, 10, 35), (1, 11, 40), (2, 15, 9), (1, 12, 11)])
def test_bce_rmi_geometry(B, H, W, C, do_rmi):
    route = "dense" if (B * H * W * C) % 4 == 0 else "odd"
    _bce_rmi_case(B, C, H, W, route, C, "blocks8", 2.0, 0.4, do_rmi, seed=H)


@pytest.mark.parametrize("scale,up", [(2.0, 0.4), (30.0, 65536.0), (30.0, 0.4), (2.0, 65536.0)])
@pytest.mark.parametrize("kind", ["blocks8", "blocks", "single", "ignored"])
@pytest.mark.parametrize("C", [19, 65])
def test_bce_rmi_label_maps(C, kind, scale, up):
    """Realistic and degenerate label maps, saturated logits (|x| ~ 30: probabilities at the 1e-6 clip or 1.0, the
    9 x 9 inverse and Cholesky near the 5e-4 I regulariser) and the loss-scaled upstream; B = 2, ignore label C."""
    _bce_rmi_case(2, C, 24, 36, "dense", C, kind, scale, up, True, seed=7)


@pytest.mark.parametrize("do_rmi", [False, True])
def test_bce_rmi_wide_crop(do_rmi):
    """A pooled width of 651 (> ~620): ssa_rmi_gram's raised-LDS branch; the odd pixel count takes the saved route."""
    _bce_rmi_case(1, 19, 9, 2601, "odd", 255, "blocks", 2.0, 0.4, do_rmi)


# The full 1024 x 1024 crop (grid-stride loops, 512 workgroups' same-address fp64 atomics of the dense BCE kernel) against
# the CPU oracle.  Not named like the small loss tests: the emulated selection (test_emu_selected_cpu.py) leaves them out.
@pytest.mark.skipif(bool(os.environ.get("SSA_EMU")), reason="full crop: GPU only")
@pytest.mark.parametrize("B,C,ign", [(1, 19, 255), (2, 65, 65)])
def test_full_crop_losses(B, C, ign):
    from oracle import ops as O
    hb = _hb()
    H = W = 1024
    g = torch.Generator().manual_seed(C)
    logits = torch.randn(B, C, H, W, generator=g) * 2
    lab = _label_map("blocks", B, H, W, C, ign, seed=C)
    lab[torch.rand(B, H, W, generator=g) < 0.05] = ign
    ld = nhwc(logits).to(DEV)
    labd = lab.to(DEV)
    # masked BCE + RMI (dense: the recomputing route), upstream = the loss scale
    lr = logits.clone().requires_grad_(True)
    loss = O.rmi_loss(lr, lab, C, do_rmi=True)
    (loss * 65536.0).backward()
    assert torch.isfinite(loss) and torch.isfinite(lr.grad).all()
    x = ld.clone().requires_grad_(True)
    out = hb.BceRmiFn.apply(x, labd, True, 0.5)
    assert out.grad_fn.recompute
    (out * 65536.0).backward()
    torch.cuda.synchronize()
    check_close("full_bce_rmi", out.view(1), loss.view(1), 1e-4, 1e-4)
    check_close("full_bce_rmi_grad", nchw(x.grad).cpu(), lr.grad, 2e-3, 1e-3)
    del lr, x, out
    # cross entropy
    lr = logits.clone().requires_grad_(True)
    loss = O.cross_entropy(lr, lab, ign)
    (loss * 65536.0).backward()
    x = ld.clone().requires_grad_(True)
    out = hb.CrossEntropyFn.apply(x, labd, ign)
    (out * 65536.0).backward()
    torch.cuda.synchronize()
    check_close("full_ce", out.view(1), loss.view(1), 1e-5, 1e-5)
    check_close("full_ce_grad", nchw(x.grad).cpu(), lr.grad, 1e-4, 1e-4)


# ------------------------------------------------------------ exact tests
# Integer-valued operands: every product is an integer and every partial sum stays below 2^24, so fp32 accumulation is
# exact in any order, on any tile shape, split or ring depth, and the single round-to-nearest-even to the 16-bit output
# is what a float64 reference reproduces BIT FOR BIT (tests/exact_util.py; the premise is asserted on the reference).
# The tolerance of everything below is zero by derivation.  What it pins that check_close cannot see: the rounding mode
# of the epilogues, the tile walk of the persistent kernel over multi-tile strips, every term of every sum, every pixel
# of the fused BatchNorm statistics.
from exact_util import (assert_bits_equal, assert_guard_intact, assert_integers, assert_premise, conv_ref64, guarded, guarded_copy, ints,  # noqa: E402
                        not_representable, to_act, wgrad_ref64)

# ---- ssa_conv2d_tile_p (csrc/conv_tile_p.hip) with explicit strip units
# name, Cin, Cout, B, H, W, units
STRIP_CASES = [
    ("c48u1", 48, 48, 2, 10, 70, 1),        # one tile per strip (what the suite ran before)
    ("c48u3", 48, 48, 2, 10, 70, 3),        # 3 tiles per strip = one tile row: every strip ends in a row wrap
    ("c48u4", 48, 48, 2, 10, 70, 4),        # 4, 4, 4, 4, 2: ragged last strip, strip 2 runs from image 0 into image 1
    ("c48u5", 48, 40, 2, 10, 70, 5),        # 5, 5, 5, 3; Cout = 40: the second n-block is 8 channels wide
    ("c48u64", 48, 48, 2, 10, 70, 64),      # one strip covers the whole problem (18 tiles)
    ("c48w20", 48, 48, 2, 11, 20, 2),       # tiles_x == 1: every advance wraps; 3 tiles per image, strips of 2
    ("c48w16", 48, 24, 1, 5, 16, 64),       # the narrowest supported image, H = 5: one pixel row in the second tile row
    ("c96u6", 96, 96, 2, 9, 33, 6),         # two chunks per tile, 3 tiles per strip, W = 33: a one-pixel tile column
    ("c96u10", 96, 72, 1, 14, 100, 10),     # interior tiles (the fast path of fetch) and border tiles in one strip
    ("c96u5", 96, 40, 1, 14, 100, 5),       # strips of 2 over the same image: (border, interior), (interior, border)
    ("c192u12", 192, 64, 1, 6, 40, 12),     # four chunks per tile, 2 tiles per strip (nstrips rebalances 3 -> 2)
    ("c192u16", 192, 40, 2, 9, 33, 16),     # four chunks, 6 tiles per image, strips of 4: the middle strip crosses the images
    ("c384u4", 384, 40, 1, 5, 33, 4),       # units < nchunk = 8: the tpw < 1 clamp
    ("c384u24", 384, 32, 1, 9, 33, 24),     # eight chunks per tile, 3 tiles per strip
]
_STRIP_IDS = [c[0] for c in STRIP_CASES]


def _strip_plan(case):
    """Mirror of launch_p (csrc/conv_tile_p.hip): the strips of this case as lists of (image, tile row, tile column)."""
    _, Cin, Cout, B, H, W, units = case
    tiles_x, tiles_y = -(-W // 32), -(-H // 4)
    total = B * tiles_x * tiles_y
    nchunk = Cin // 48
    tpw = max(1, min(units, 64) // nchunk)
    nstrips = -(-total // tpw)
    tiles_per_wg = -(-total // nstrips)
    tiles = [(b, ty, tx) for b in range(B) for ty in range(tiles_y) for tx in range(tiles_x)]
    strips = [tiles[i:i + tiles_per_wg] for i in range(0, total, tiles_per_wg)]

    def interior(t):
        x0, y0 = t[2] * 32, t[1] * 4
        return x0 >= 1 and y0 >= 1 and x0 + 33 <= W and y0 + 5 <= H
    return dict(tiles_x=tiles_x, tiles_y=tiles_y, total=total, nchunk=nchunk, units=units, tiles_per_wg=tiles_per_wg,
                per_image=tiles_x * tiles_y, strips=strips, ragged=len(strips[-1]) < tiles_per_wg,
                crosses=any(len({t[0] for t in s}) > 1 for s in strips),
                mixed=any(any(interior(t) for t in s) and not all(interior(t) for t in s) for s in strips))


def _assert_strip_coverage(cases):
    """A condition on the parameter list, not a measurement: a later edit of the list cannot silently drop a regime."""
    plans = [(c, _strip_plan(c)) for c in cases]
    tpws = {p["tiles_per_wg"] for _, p in plans}
    assert {1, 2, 3} <= tpws and max(tpws) >= 5, tpws
    assert any(p["ragged"] for _, p in plans), "no ragged last strip"
    assert any(c[3] == 2 and p["per_image"] % p["tiles_per_wg"] and p["crosses"] for c, p in plans), "no strip crosses an image boundary"
    assert any(c[3] == 2 and p["nchunk"] > 1 and p["per_image"] % p["tiles_per_wg"] and p["crosses"] for c, p in plans), \
        "no multi-chunk strip crosses an image boundary"
    assert any(p["tiles_x"] == 1 and 16 <= c[5] <= 32 and p["tiles_per_wg"] > 1 for c, p in plans), "no tiles_x == 1 case"
    assert any(c[5] % 32 and c[4] % 4 for c, _ in plans), "no case with W % 32 != 0 and H % 4 != 0"
    assert any(c[5] >= 97 and c[4] >= 13 and p["mixed"] for c, p in plans), "no strip mixes interior and border tiles"
    assert any(c[6] == 64 and len(p["strips"]) == 1 and p["total"] > 1 for c, p in plans), "no single strip over a whole problem"
    assert any(c[1] == 384 and c[6] < p["nchunk"] and p["tiles_per_wg"] == 1 for c, p in plans), "no units < nchunk case"
    assert {c[1] for c in cases} == {48, 96, 192, 384}
    for c, p in plans:
        assert c[5] >= 16 and c[2] % 8 == 0 and sum(len(s) for s in p["strips"]) == p["total"], c


_assert_strip_coverage(STRIP_CASES)

# Operand amplitudes (x and w uniform integers in [-a, a]) per input-channel count.
#   narrow: for the cases with statistics.  The kernel sums y and y^2 of the rounded outputs in fp32 over a strip, so the
#     premise there is sum_pixels y^2 < 2^24 per channel (asserted on the reference, over the WHOLE problem: an upper
#     bound of any strip); outputs reach a few hundred -- above 2^8, so the bf16 rounding, ties included, decides bits.
#   wide: for the epilogues without statistics (aux modes 1, 3, 4 and mode 0 without stats).  Outputs reach several
#     thousand -- above 2^11, so the fp16 build rounds too -- and stay far below the fp16 maximum after a scale of 4.
_AMP_NARROW = {48: (4, 2), 96: (3, 2), 192: (2, 2), 384: (2, 1)}
_AMP_WIDE = {48: (15, 15), 96: (12, 12), 192: (10, 10), 384: (8, 8)}


def _strip_operands(case, wide, seed=0):
    _, Cin, Cout, B, H, W, _ = case
    ax, aw = (_AMP_WIDE if wide else _AMP_NARROW)[Cin]
    return ints((B, Cin, H, W), -ax, ax, seed + 100), ints((Cout, Cin, 3, 3), -aw, aw, seed + 101)


def _ref_nhwc(case, x, w):
    """float64 conv [B,H,W,Cout] and how many of its values the 16-bit format cannot hold"""
    ref = conv_ref64(x, w, None, 1, 1, 1).permute(0, 2, 3, 1).contiguous()
    n = not_representable(ref)
    print("[exact %s] max |y| = %d, %d of %d outputs are not representable in %s" % (
        case[0], int(ref.abs().max()), n, ref.numel(), ACT_DTYPE))
    return ref, n


def _pack_for_tile(hb, w, tr):
    """Fragment-order filter of the conv with OIHW weight w: forward packing (ssa_pack_filter mode 2), or the
    data-gradient packing (mode 3) of the forward weight whose data gradient this conv is.  Returns (packed, keep-alive)."""
    if tr:
        wt = w.flip(2, 3).permute(1, 0, 2, 3).contiguous().to(DEV)       # [Cin_fwd = Cout here][Cout_fwd = Cin here], taps flipped
        return hb._packed_filter(wt, 3, 0, w.shape[1])[0], wt
    wd = w.to(DEV)
    return hb._packed_filter(wd, 2, w.shape[1], 0)[0], wd


def _launch_tile_p(case, x, w, mode=0, tr=False, stats=False, aux=None, ldaux=None, coef=None, ldx=None, ldy=None,
                   strip=True, packed=None):
    """One ssa_conv2d_tile_p launch through the C ABI inside ssa_conv_tile_strip(units) ... (0).  Input, output and
    statistics live in guarded buffers (NaN all around, the output pre-filled with NaN)."""
    import ctypes
    from semseg_amd._lib import check
    hb = _hb()
    L = hb.lib()
    _, Cin, Cout, B, H, W, units = case
    xg = guarded_copy(nhwc(x).to(ACT_DTYPE), DEV, ldx)
    wp, keep = packed if packed is not None else _pack_for_tile(hb, w, tr)
    d = hb._tile_desc(B, H, W, Cin, ldx or Cin, Cout, (3, 3), 1, 1, 1, H, W, False)
    d.ldy = ldy or Cout
    assert L.ssa_conv2d_tile_p_supported(ctypes.byref(d)) == 1
    yg = guarded((B, H, W, Cout), ACT_DTYPE, DEV, ldy)
    sg = None
    if stats:
        sg = guarded((hb.stat_replicas(), 2, Cout), torch.float64, DEV)
        sg.view.zero_()
    ag = guarded_copy(aux.to(ACT_DTYPE), DEV, ldaux) if aux is not None else None
    cd = coef.to(DEV).contiguous() if coef is not None else None
    gs = [g for g in (xg, yg, sg, ag) if g is not None]

    def go():
        check(L.ssa_conv2d_tile_p(ctypes.byref(d), hb._p(xg.view), hb._p(wp), None, hb._p(yg.view),
                                  hb._p(sg.view) if sg else None, hb._p(ag.view) if ag else None,
                                  (ldaux or Cout) if ag else 0, hb._p(cd), mode, hb._s()), "ssa_conv2d_tile_p")
    if not strip:           # the caller brackets (a grouped level)
        go()
        return yg, sg, gs + [keep, cd, wp]
    L.ssa_conv_tile_strip(units)
    try:
        go()
    finally:
        L.ssa_conv_tile_strip(0)
    if xg.view.is_cuda:
        torch.cuda.synchronize()
    assert_guard_intact("tile_p %s" % case[0], *gs)
    return yg, sg


def _check_stats(name, sg, want0, want1):
    """Both rows of the summed replicas against float64 sums, with torch.equal: no pixel missing, none counted twice."""
    got = sg.view.sum(0).cpu()
    for row, want, what in ((0, want0, "sums"), (1, want1, "second sums")):
        if not torch.equal(got[row], want):
            c = int((got[row] != want).nonzero()[0])
            raise AssertionError("%s %s differ in %d channels; first: channel %d got %r want %r" % (
                name, what, int((got[row] != want).sum()), c, float(got[row][c]), float(want[c])))


def test_exact_strip_cases_need_rounding():
    """The operands of the strip tests exercise the rounding: for every Cin at least one case has outputs the 16-bit
    format cannot hold (wide operands: both builds; narrow operands, the cases with statistics: bf16, whose mantissa
    ends at 2^8 -- fp16 holds every integer up to 2^11 and sum y^2 < 2^24 leaves no room above that)."""
    for Cin in (48, 96, 192, 384):
        cases = [c for c in STRIP_CASES if c[1] == Cin]
        assert sum(_ref_nhwc(c, *_strip_operands(c, True))[1] for c in cases) > 0, Cin
        if ACT_DTYPE == torch.bfloat16:
            assert sum(_ref_nhwc(c, *_strip_operands(c, False))[1] for c in cases) > 0, Cin


@pytest.mark.parametrize("tr", [False, True], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("case", STRIP_CASES, ids=_STRIP_IDS)
def test_exact_strip_mode0(case, tr):
    """aux_mode 0: the output bit for bit, every element written (the buffer starts as NaN), and the BatchNorm sums of
    the ROUNDED outputs equal to the float64 sums -- one missing or doubled pixel, one wrong channel of one tile fails."""
    hb = _hb()
    hb.clear_pack_cache()
    p = _strip_plan(case)
    x, w = _strip_operands(case, False)
    ref, _ = _ref_nhwc(case, x, w)
    want = to_act(ref)
    r = want.double().view(-1, case[2])
    assert_premise("sum of y^2 over the pixels", (r * r).sum(0))       # the kernel's fp32 strip sums are then exact
    yg, sg = _launch_tile_p(case, x, w, 0, tr, stats=True)
    assert_bits_equal("tile_p mode 0 %s" % case[0], yg.view.cpu(), want, tile=(4, 32, p["tiles_per_wg"]))
    _check_stats("tile_p mode 0 %s" % case[0], sg, r.sum(0), (r * r).sum(0))
    hb.clear_pack_cache()


@pytest.mark.parametrize("case", STRIP_CASES, ids=_STRIP_IDS)
def test_exact_strip_mode0_wide_no_stats(case):
    """aux_mode 0 without statistics on the wide operands: outputs of several thousand, rounded in both builds."""
    hb = _hb()
    hb.clear_pack_cache()
    x, w = _strip_operands(case, True)
    ref, _ = _ref_nhwc(case, x, w)
    yg, _ = _launch_tile_p(case, x, w, 0, False)
    assert_bits_equal("tile_p wide %s" % case[0], yg.view.cpu(), to_act(ref), tile=(4, 32, _strip_plan(case)["tiles_per_wg"]))
    hb.clear_pack_cache()


@pytest.mark.parametrize("tr", [False, True], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("case", STRIP_CASES, ids=_STRIP_IDS)
def test_exact_strip_mode1(case, tr):
    """aux_mode 1: y = r16(r16(conv) + aux), two roundings by specification (include/semseg_hip.h, ssa_conv2d_tile_aux;
    csrc/conv_tile_p.hip `f[j] += xv[j]; o = pack8(f)` on the unpacked 16-bit conv output).  Both are reproduced: the
    intermediate is a 16-bit value, the integer aux tile (pixel stride ldaux > Cout, NaN neighbours) is added exactly."""
    hb = _hb()
    hb.clear_pack_cache()
    _, Cin, Cout, B, H, W, _ = case
    x, w = _strip_operands(case, True)
    ref, _ = _ref_nhwc(case, x, w)
    aux = ints((B, H, W, Cout), -100, 100, 7)
    want = to_act(to_act(ref).double() + aux.double())
    yg, _ = _launch_tile_p(case, x, w, 1, tr, aux=aux, ldaux=Cout + 24)
    assert_bits_equal("tile_p mode 1 %s" % case[0], yg.view.cpu(), want, tile=(4, 32, _strip_plan(case)["tiles_per_wg"]))
    hb.clear_pack_cache()


def _bn_coef(Cout, seed):
    """[4][Cout] coefficient table that keeps the epilogue exact: scale = +-2^k (mixed gamma signs), integer shift,
    integer mean, invstd a power of two."""
    g = torch.Generator().manual_seed(seed)
    scale = 2.0 ** torch.randint(-2, 3, (Cout,), generator=g).float() * (torch.randint(0, 2, (Cout,), generator=g).float() * 2 - 1)
    assert (scale > 0).any() and (scale < 0).any()
    shift = torch.randint(-2, 3, (Cout,), generator=g).float()
    mean = torch.randint(-2, 3, (Cout,), generator=g).float()
    invstd = 2.0 ** torch.randint(-2, 2, (Cout,), generator=g).float()
    return torch.stack([scale, shift, mean, invstd])


@pytest.mark.parametrize("case", STRIP_CASES, ids=_STRIP_IDS)
def test_exact_strip_mode2(case):
    """aux_mode 2 (the data-gradient packing, as the product uses it): y = dz untouched, and the BatchNorm backward sums
    sum(m dz), sum(m dz xhat) with m = [scale x + shift > 0] exactly -- gamma signs mixed, many pre-activations exactly
    0 (the comparison is strict), the integer x tile at ldaux > Cout."""
    hb = _hb()
    hb.clear_pack_cache()
    _, Cin, Cout, B, H, W, _ = case
    x, w = _strip_operands(case, False)
    ref, _ = _ref_nhwc(case, x, w)
    dz = to_act(ref)
    a = ints((B, H, W, Cout), -3, 3, 8)
    coef = _bn_coef(Cout, 9)
    c = coef.double()
    pre = a.double() * c[0] + c[1]
    assert int((pre == 0).sum()) > a.numel() // 50, "too few pre-activations are exactly zero"
    m = (pre > 0).double()
    dzd = dz.double()
    assert_premise("sum |dz| |x|", (dzd.abs() * a.double().abs()).view(-1, Cout).sum(0))
    want0 = (m * dzd).view(-1, Cout).sum(0)
    want1 = (m * dzd * (a.double() - c[2]) * c[3]).view(-1, Cout).sum(0)
    yg, sg = _launch_tile_p(case, x, w, 2, True, stats=True, aux=a, ldaux=Cout + 8, coef=coef)
    assert_bits_equal("tile_p mode 2 %s" % case[0], yg.view.cpu(), dz, tile=(4, 32, _strip_plan(case)["tiles_per_wg"]))
    _check_stats("tile_p mode 2 %s" % case[0], sg, want0, want1)
    hb.clear_pack_cache()


@pytest.mark.parametrize("relu", [False, True], ids=["mode3", "mode4relu"])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("case", STRIP_CASES, ids=_STRIP_IDS)
def test_exact_strip_affine(case, res, relu):
    """aux_mode 3 / 4 (inference): z = r16(act(scale * r16(conv) + shift [+ residual])) -- the conv output is rounded to 16
    bits FIRST, as the header specifies; scales +-2^k and integer shifts keep the affine step exact."""
    hb = _hb()
    hb.clear_pack_cache()
    _, Cin, Cout, B, H, W, _ = case
    x, w = _strip_operands(case, True)
    ref, _ = _ref_nhwc(case, x, w)
    coef = _bn_coef(Cout, 10)
    coef[1] = ints((Cout,), -50, 50, 11)
    coef[2:] = 0
    c = coef.double()
    z = to_act(ref).double() * c[0] + c[1]
    r = ints((B, H, W, Cout), -100, 100, 12) if res else None
    if res:
        z = z + r.double()
    if relu:
        z = torch.relu(z)
    assert float(z.abs().max()) < 60000.0            # finite in fp16
    yg, _ = _launch_tile_p(case, x, w, 4 if relu else 3, False, aux=r, ldaux=Cout + 16 if res else None, coef=coef)
    assert_bits_equal("tile_p affine %s" % case[0], yg.view.cpu(), to_act(z), tile=(4, 32, _strip_plan(case)["tiles_per_wg"]))
    hb.clear_pack_cache()


@pytest.mark.parametrize("which", ["ldy", "ldx"])
def test_exact_strip_sliced_buffers(which):
    """ldy > Cout: the output is a channel slice whose neighbouring channels must keep their NaN pattern; ldx > Cin: the
    input is a channel slice whose neighbours ARE NaN -- one stray channel read poisons the output."""
    hb = _hb()
    hb.clear_pack_cache()
    case = dict(zip(_STRIP_IDS, STRIP_CASES))["c48u5" if which == "ldy" else "c96u6"]
    x, w = _strip_operands(case, False)
    ref, _ = _ref_nhwc(case, x, w)
    want = to_act(ref)
    r = want.double().view(-1, case[2])
    kw = dict(ldy=case[2] + 24) if which == "ldy" else dict(ldx=case[1] + 32)
    yg, sg = _launch_tile_p(case, x, w, 0, False, stats=True, **kw)
    assert_bits_equal("tile_p %s %s" % (which, case[0]), yg.view.cpu(), want, tile=(4, 32, _strip_plan(case)["tiles_per_wg"]))
    _check_stats("tile_p %s" % which, sg, r.sum(0), (r * r).sum(0))
    hb.clear_pack_cache()


def test_exact_strip_grouped_level():
    """Problems of different Cin as ONE grouped level under one explicit strip length > 1 (what BasicBlockGroupFn does
    through hb.tile_strip): each equals its exact reference and its own single launch bit for bit, statistics included."""
    hb = _hb()
    L = hb.lib()
    hb.clear_pack_cache()
    units = 8
    level = [("g48", 48, 48, 2, 9, 40, units), ("g96", 96, 40, 1, 6, 33, units), ("g192", 192, 32, 1, 5, 20, units),
             ("g48b", 48, 24, 1, 14, 100, units)]
    assert all(_strip_plan(c)["tiles_per_wg"] > 1 for c in level)
    ops = [_strip_operands(c, False, seed=10 * i) for i, c in enumerate(level)]
    single = [_launch_tile_p(c, x, w, 0, False, stats=True) for c, (x, w) in zip(level, ops)]
    packs = [_pack_for_tile(hb, w, False) for _, w in ops]          # (the packing launches stay outside the count)
    L.ssa_launch_count(1)
    L.ssa_conv_tile_strip(units)
    try:
        with hb.group():
            grouped = [_launch_tile_p(c, x, w, 0, False, stats=True, strip=False, packed=pk)
                       for c, (x, w), pk in zip(level, ops, packs)]
    finally:
        L.ssa_conv_tile_strip(0)
    if DEV != "cpu":
        torch.cuda.synchronize()
    assert L.ssa_launch_count(1) == 1
    for c, (x, w), (y1, s1), (y2, s2, gs) in zip(level, ops, single, grouped):
        assert_guard_intact("grouped %s" % c[0], *[g for g in gs if hasattr(g, "inside")])
        want = to_act(_ref_nhwc(c, x, w)[0])
        tile = (4, 32, _strip_plan(c)["tiles_per_wg"])
        assert_bits_equal("grouped %s vs reference" % c[0], y2.view.cpu(), want, tile=tile)
        assert_bits_equal("grouped %s vs single launch" % c[0], y2.view.cpu(), y1.view.cpu(), tile=tile)
        r = want.double().view(-1, c[2])
        _check_stats("grouped %s" % c[0], s2, r.sum(0), (r * r).sum(0))
        assert torch.equal(s2.view.sum(0).cpu(), s1.view.sum(0).cpu())
    hb.clear_pack_cache()


# ---- the same exact check on the other convolution entry points (the case lists of the statistical tests above)
def _exact_fwd_check(name, y, st, ref, Cout):
    """Output bits, every element written; the BatchNorm sums of the rounded outputs with torch.equal."""
    want = to_act(ref)
    assert_bits_equal(name, y.view.cpu(), want)
    if st is not None:
        r = want.double().view(-1, Cout)
        assert_premise(name + ": sum of y^2 over the pixels", (r * r).sum(0))
        _check_stats(name, st, r.sum(0), (r * r).sum(0))
    assert_guard_intact(name, *[g for g in (y, st) if g is not None])


def _stats_buf(hb, Cout, on):
    if not on:
        return None
    sg = guarded((hb.stat_replicas(), 2, Cout), torch.float64, DEV)
    sg.view.zero_()
    return sg


@pytest.mark.parametrize("case", HALO_REG_CASES)
def test_exact_halo_reg_3x3(case):
    """ssa_conv2d_halo_reg on the cases of test_halo_reg_3x3, integer operands: bits of the output, sums of the stats."""
    import ctypes
    from semseg_amd._lib import check
    hb = _hb()
    B, H, W, Cin, Cout, bias, stats, tr = case
    x, w = ints((B, Cin, H, W), -2, 2, 3), ints((Cout, Cin, 3, 3), -2, 2, 4)
    b = ints((Cout,), -5, 5, 5) if bias else None
    ref = conv_ref64(x, w, b, 1, 1, 1).permute(0, 2, 3, 1).contiguous()
    print("[exact halo_reg] %d outputs not representable" % not_representable(ref))
    hb.clear_pack_cache()
    xg = guarded_copy(nhwc(x).to(ACT_DTYPE), DEV)
    wp, keep = _pack_for_tile(hb, w, tr)
    d = hb._tile_desc(B, H, W, Cin, Cin, Cout, (3, 3), 1, 1, 1, H, W, False)
    L = hb.lib()
    assert L.ssa_conv2d_halo_reg_supported(ctypes.byref(d)) == 1
    yg, sg = guarded((B, H, W, Cout), ACT_DTYPE, DEV), _stats_buf(hb, Cout, stats)
    bd = b.to(DEV) if b is not None else None
    check(L.ssa_conv2d_halo_reg(ctypes.byref(d), hb._p(xg.view), hb._p(wp), hb._p(bd), hb._p(yg.view),
                                hb._p(sg.view) if sg else None, hb._s()), "halo_reg")
    if DEV != "cpu":
        torch.cuda.synchronize()
    _exact_fwd_check("halo_reg %s" % (case,), yg, sg, ref, Cout)
    hb.clear_pack_cache()


@pytest.mark.parametrize("case", WIDE_CASES)
def test_exact_gemm_wide_1x1(case):
    """ssa_conv2d_gemm_wide on the cases of test_gemm_wide_1x1, integer operands."""
    import ctypes
    from semseg_amd._lib import check
    hb = _hb()
    B, H, W, Cin, Cout, bias, stats, tr = case
    x, w = ints((B, Cin, H, W), -4, 4, 3), ints((Cout, Cin, 1, 1), -4, 4, 4)
    b = ints((Cout,), -5, 5, 5) if bias else None
    ref = conv_ref64(x, w, b, 1, 0, 1).permute(0, 2, 3, 1).contiguous()
    print("[exact gemm_wide] %d outputs not representable" % not_representable(ref))
    hb.clear_pack_cache()
    xg = guarded_copy(nhwc(x).to(ACT_DTYPE), DEV)
    if tr:
        keep = w[:, :, 0, 0].t().contiguous().view(Cin, Cout, 1, 1).to(DEV)
        wp, _ = hb._packed_filter(keep, 3, 0, Cin)
    else:
        keep = w.to(DEV)
        wp, _ = hb._packed_filter(keep, 2, Cin, 0)
    d = hb._tile_desc(B, H, W, Cin, Cin, Cout, (1, 1), 1, 0, 1, H, W, False)
    L = hb.lib()
    yg, sg = guarded((B, H, W, Cout), ACT_DTYPE, DEV), _stats_buf(hb, Cout, stats)
    bd = b.to(DEV) if b is not None else None
    check(L.ssa_conv2d_gemm_wide(ctypes.byref(d), hb._p(xg.view), hb._p(wp), hb._p(bd), hb._p(yg.view),
                                 hb._p(sg.view) if sg else None, hb._s()), "wide")
    if DEV != "cpu":
        torch.cuda.synchronize()
    _exact_fwd_check("gemm_wide %s" % (case,), yg, sg, ref, Cout)
    hb.clear_pack_cache()


HALO_GEMM_EXACT_CASES = [
    # id, B, H, W, Cin, Cout, bias, stats, transposed-pack, |x| <=, |w| <=, fp32 output.  ssa_conv2d_halo keeps a 1x1
    # problem for its own 256 x 128 kernel at Cin >= 192, Cout >= 64, W >= 32, B*H*W >= 16384 unless the wide kernel
    # wants it (Cout > 256): the smallest shapes that pass the dispatcher and still reach the kernel's edges.
    ("A", 1, 130, 127, 192, 72, True, True, False, 1, 2, False),     # CK 64, ragged tile rows and columns, n-block tail
    ("B", 2, 96, 88, 240, 136, False, True, True, 1, 2, False),      # CK 48, second channel tile 8 wide, batch 2, dgrad packing
    ("C", 1, 128, 128, 256, 200, True, False, False, 4, 4, False),   # outputs in the thousands: the rounding decides bits
    ("D", 1, 128, 128, 192, 65, True, False, False, 4, 4, True),     # the fp32 branch of the logit convs, odd channel count
]


@pytest.mark.parametrize("case", HALO_GEMM_EXACT_CASES, ids=[c[0] for c in HALO_GEMM_EXACT_CASES])
def test_exact_halo_gemm_1x1(case):
    """ConvHaloGemm1 (csrc/conv_halo_gemm.hip) through ssa_conv2d_halo, integer operands: bits of the 16-bit output and
    sums of the stats (A, B: sum of y^2 per channel stays below 2^24; C, D carry no stats because theirs does not), and
    the fp32 output of the 64-255-class logit convs, an exact integer, against the fp32 reference (D)."""
    import ctypes
    from semseg_amd._lib import check
    hb = _hb()
    name, B, H, W, Cin, Cout, bias, stats, tr, ax, aw, out_f32 = case
    x, w = ints((B, Cin, H, W), -ax, ax, 3), ints((Cout, Cin, 1, 1), -aw, aw, 4)
    b = ints((Cout,), -5, 5, 5) if bias else None
    ref = conv_ref64(x, w, b, 1, 0, 1).permute(0, 2, 3, 1).contiguous()
    nrep = not_representable(ref)
    print("[exact halo_gemm %s] %d outputs not representable" % (name, nrep))
    if name == "C" and ACT_DTYPE == torch.bfloat16:
        assert nrep > 0
    hb.clear_pack_cache()
    xg = guarded_copy(nhwc(x).to(ACT_DTYPE), DEV)
    if tr:
        keep = w[:, :, 0, 0].t().contiguous().view(Cin, Cout, 1, 1).to(DEV)
        wp, _ = hb._packed_filter(keep, 3, 0, Cin)
    else:
        keep = w.to(DEV)
        wp, _ = hb._packed_filter(keep, 2, Cin, 0)
    d = hb._tile_desc(B, H, W, Cin, Cin, Cout, (1, 1), 1, 0, 1, H, W, out_f32)
    L = hb.lib()
    assert L.ssa_conv2d_halo_supported(ctypes.byref(d)) == 1
    assert L.ssa_conv2d_gemm_wide_supported(ctypes.byref(d)) == 0
    yg, sg = guarded((B, H, W, Cout), torch.float32 if out_f32 else ACT_DTYPE, DEV), _stats_buf(hb, Cout, stats)
    bd = b.to(DEV) if b is not None else None
    check(L.ssa_conv2d_halo(ctypes.byref(d), hb._p(xg.view), hb._p(wp), hb._p(bd), hb._p(yg.view),
                            hb._p(sg.view) if sg else None, hb._s()), "halo")
    if DEV != "cpu":
        torch.cuda.synchronize()
    if out_f32:
        want = ref.float()
        assert torch.equal(want.double(), ref)
        assert_bits_equal("halo_gemm %s fp32" % name, yg.view.cpu(), want)
        assert_guard_intact("halo_gemm %s fp32" % name, yg)
    else:
        _exact_fwd_check("halo_gemm %s" % name, yg, sg, ref, Cout)
    hb.clear_pack_cache()


@pytest.mark.parametrize("out_f32", [False, True], ids=["out16", "out32"])
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
def test_exact_igemm_tile_configs(cfg, out_f32):
    """ssa_conv2d_igemm(_stats): all six tile configurations on the ragged shape of test_conv_all_tile_configs, with
    bias; 16-bit output (+ statistics) and fp32 output (an exact integer: no rounding at all)."""
    hb = _hb()
    B, H, W, Cin, Cout = 1, 37, 45, 72, 88
    x, w, b = ints((B, Cin, H, W), -3, 3, 3), ints((Cout, Cin, 3, 3), -2, 2, 4), ints((Cout,), -5, 5, 5)
    ref = conv_ref64(x, w, b, 1, 1, 1).permute(0, 2, 3, 1).contiguous()
    hb.clear_pack_cache()
    xg = guarded_copy(nhwc(x).to(ACT_DTYPE), DEV)
    wd = w.to(DEV)
    wp, Kpad = hb._packed_filter(wd, 0, Cin, 0)
    yg = guarded((B, H, W, Cout), torch.float32 if out_f32 else ACT_DTYPE, DEV)
    sg = _stats_buf(hb, Cout, not out_f32)
    hb._igemm(xg.view, Cin, (B, H, W, Cin), wp, Kpad, b.to(DEV), (H, W), Cout, (3, 3), 1, 1, 1, False, out_f32, cfg=cfg,
              stats=sg.view if sg else None, out=yg.view)
    if DEV != "cpu":
        torch.cuda.synchronize()
    if out_f32:
        assert_bits_equal("igemm cfg%d fp32" % cfg, yg.view.cpu(), ref.float())
        assert_guard_intact("igemm cfg%d fp32" % cfg, yg)
    else:
        print("[exact igemm] %d outputs not representable" % not_representable(ref))
        _exact_fwd_check("igemm cfg%d" % cfg, yg, sg, ref, Cout)
    hb.clear_pack_cache()


# B, H, W, Cin, Cout: shapes ssa_conv2d_tile_p does not take (64 channels; W < 16)
TILE_EXACT_CASES = [(1, 9, 20, 64, 64), (2, 20, 12, 48, 96), (1, 9, 7, 96, 48), (1, 33, 18, 64, 24)]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("case", TILE_EXACT_CASES)
def test_exact_tile_and_tile_aux(case, mode):
    """ssa_conv2d_tile (mode 0: bias + statistics) and ssa_conv2d_tile_aux (1: r16(r16(conv) + aux), two roundings by
    specification; 2: the BatchNorm backward sums) of csrc/conv_tile.hip on 64-channel and W < 16 shapes."""
    import ctypes
    from semseg_amd._lib import check
    hb = _hb()
    L = hb.lib()
    B, H, W, Cin, Cout = case
    x, w = ints((B, Cin, H, W), -3, 3, 21), ints((Cout, Cin, 3, 3), -2, 2, 22)
    b = ints((Cout,), -5, 5, 23) if mode == 0 else None
    ref = conv_ref64(x, w, b, 1, 1, 1).permute(0, 2, 3, 1).contiguous()
    hb.clear_pack_cache()
    xg = guarded_copy(nhwc(x).to(ACT_DTYPE), DEV)
    wp, keep = _pack_for_tile(hb, w, mode != 0)
    d = hb._tile_desc(B, H, W, Cin, Cin, Cout, (3, 3), 1, 1, 1, H, W, False)
    assert L.ssa_conv2d_tile_supported(ctypes.byref(d)) == 1 and L.ssa_conv2d_tile_p_supported(ctypes.byref(d)) == 0
    yg, sg = guarded((B, H, W, Cout), ACT_DTYPE, DEV), _stats_buf(hb, Cout, mode != 1)
    name = "tile mode %d %s" % (mode, case)
    if mode == 0:
        check(L.ssa_conv2d_tile(ctypes.byref(d), hb._p(xg.view), hb._p(wp), hb._p(b.to(DEV)), hb._p(yg.view), hb._p(sg.view),
                                hb._s()), "ssa_conv2d_tile")
        if DEV != "cpu":
            torch.cuda.synchronize()
        _exact_fwd_check(name, yg, sg, ref, Cout)
    else:
        a = ints((B, H, W, Cout), -100, 100, 24) if mode == 1 else ints((B, H, W, Cout), -3, 3, 24)
        ag = guarded_copy(a.to(ACT_DTYPE), DEV, Cout + 8)
        coef = _bn_coef(Cout, 25)
        cd = coef.to(DEV)
        check(L.ssa_conv2d_tile_aux(ctypes.byref(d), hb._p(xg.view), hb._p(wp), None, hb._p(yg.view),
                                    hb._p(sg.view) if sg else None, hb._p(ag.view), Cout + 8, hb._p(cd) if mode == 2 else None,
                                    mode, hb._s()), "ssa_conv2d_tile_aux")
        if DEV != "cpu":
            torch.cuda.synchronize()
        dz = to_act(ref)
        if mode == 1:
            assert_bits_equal(name, yg.view.cpu(), to_act(dz.double() + a.double()))
        else:
            c = coef.double()
            m = (a.double() * c[0] + c[1] > 0).double()
            dzd = dz.double()
            assert_premise("sum |dz| |x|", (dzd.abs() * a.double().abs()).view(-1, Cout).sum(0))
            assert_bits_equal(name, yg.view.cpu(), dz)
            _check_stats(name, sg, (m * dzd).view(-1, Cout).sum(0), (m * dzd * (a.double() - c[2]) * c[3]).view(-1, Cout).sum(0))
        assert_guard_intact(name, *[g for g in (xg, yg, sg, ag) if g is not None])
    hb.clear_pack_cache()


# B, H, W, Cin, Cout of the forward stride-2 conv: even / odd extents, Cout no multiple of 32, one-pixel classes
DGRAD_S2_EXACT_CASES = [(2, 31, 50, 96, 96), (1, 17, 16, 192, 384), (1, 37, 45, 48, 96), (2, 33, 64, 96, 200),
                        (1, 2, 3, 48, 24), (1, 1, 9, 48, 48), (1, 64, 64, 48, 96)]


@pytest.mark.parametrize("case", DGRAD_S2_EXACT_CASES)
def test_exact_dgrad_s2(case):
    """ssa_conv2d_dgrad_s2 (four parity classes) against the exact transposed reference: the float64 gradient of the
    stride-2 conv with respect to its input."""
    import ctypes
    from semseg_amd._lib import check
    hb = _hb()
    B, H, W, Cin, Cout = case
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w, dy = ints((Cout, Cin, 3, 3), -2, 2, 31), ints((B, Cout, Ho, Wo), -3, 3, 32)
    assert_integers("dgrad_s2", w, dy)
    F = torch.nn.functional

    def dgrad(ww, gg):
        xx = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(xx, ww, None, 2, 1, 1).backward(gg)
        return xx.grad.permute(0, 2, 3, 1).contiguous()
    assert_premise("dgrad_s2", dgrad(w.double().abs(), dy.double().abs()))
    ref = dgrad(w.double(), dy.double())
    print("[exact dgrad_s2] %d outputs not representable" % not_representable(ref))
    hb.clear_pack_cache()
    wd = w.to(DEV)
    dg = guarded_copy(nhwc(dy).to(ACT_DTYPE), DEV)
    packs = [hb._packed_filter(wd, 4 + c, 0, Cout) for c in range(4)]
    dxg = guarded((B, H, W, Cin), ACT_DTYPE, DEV)
    wp = (ctypes.c_void_p * 4)(*[t.data_ptr() for t, _ in packs])
    kp = (ctypes.c_int * 4)(*[k for _, k in packs])
    check(hb.lib().ssa_conv2d_dgrad_s2(B, H, W, Cin, Cin, Ho, Wo, Cout, Cout, hb._p(dg.view), wp, kp, hb._p(dxg.view),
                                       hb._s()), "ssa_conv2d_dgrad_s2")
    if DEV != "cpu":
        torch.cuda.synchronize()
    assert_bits_equal("dgrad_s2 %s" % (case,), dxg.view.cpu(), to_act(ref))
    assert_guard_intact("dgrad_s2 %s" % (case,), dg, dxg)
    hb.clear_pack_cache()


def _exact_wgrad(kind, B, H, W, Cin, Cout, k, stride, pad, cfg, amp=3):
    """One weight-gradient kernel (`kind`: tile / head / wgrad = split-K) + ssa_conv2d_wgrad_reduce through the C ABI:
    the fp32 gradient bit for bit (an exact integer: sum |x| |dy| over all pixels < 2^24, asserted on the reference).
    The fp32 partial buffer starts as NaN: a block no workgroup writes poisons the reduce."""
    import ctypes
    from semseg_amd._lib import check, ConvDesc
    hb = _hb()
    L = hb.lib()
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x, dy = ints((B, Cin, H, W), -amp, amp, 41), ints((B, Cout, Ho, Wo), -amp, amp, 42)
    ref = wgrad_ref64(x, dy, k, stride, pad, 1)
    xg, gg = guarded_copy(nhwc(x).to(ACT_DTYPE), DEV), guarded_copy(nhwc(dy).to(ACT_DTYPE), DEV)
    d = ConvDesc(B, H, W, Cin, Cin, Ho, Wo, Cout, Cout, k, k, stride, pad, 1, 0, 0, 0, cfg)
    ns, ws = ctypes.c_int(0), ctypes.c_size_t(0)
    plan = {"tile": L.ssa_conv2d_wgrad_tile_plan, "head": L.ssa_conv2d_wgrad_head_plan, "wgrad": L.ssa_conv2d_wgrad_plan}[kind]
    fn = {"tile": L.ssa_conv2d_wgrad_tile, "head": L.ssa_conv2d_wgrad_head, "wgrad": L.ssa_conv2d_wgrad}[kind]
    check(plan(ctypes.byref(d), Cout, ctypes.byref(ns), ctypes.byref(ws)), "plan")
    part = guarded((ws.value // 4,), torch.float32, DEV)
    dw = guarded((Cout, Cin, k, k), torch.float32, DEV)
    check(fn(ctypes.byref(d), hb._p(xg.view), hb._p(gg.view), Cout, Cout, ns.value, hb._p(part.view), hb._s()), kind)
    check(L.ssa_conv2d_wgrad_reduce(hb._p(part.view), ns.value, Cout, Cout, Cin, Cin, k, k, hb._p(dw.view), 0, hb._s()),
          "ssa_conv2d_wgrad_reduce")
    if DEV != "cpu":
        torch.cuda.synchronize()
    name = "%s wgrad %s cfg %d (%d splits)" % (kind, (B, H, W, Cin, Cout, k, stride), cfg, ns.value)
    assert_bits_equal(name, dw.view.cpu(), ref.float())
    assert_guard_intact(name, xg, gg, part, dw)
    return ns.value


@pytest.mark.parametrize("cfg", [-1, 1, 2, 3], ids=["default", "strip1", "strip2", "strip3"])
@pytest.mark.parametrize("C,B,H,W", [(48, 1, 37, 45), (64, 2, 20, 33), (96, 1, 21, 40), (192, 1, 9, 40), (384, 1, 9, 33)])
def test_exact_wgrad_tile(C, B, H, W, cfg):
    """ssa_conv2d_wgrad_tile + reduce at the default split and at strips of 1, 2, 3 tiles per workgroup."""
    _exact_wgrad("tile", B, H, W, C, C, 3, 1, 1, cfg)


@pytest.mark.parametrize("cfg", [-1, 1], ids=["default", "strip1"])
@pytest.mark.parametrize("B,H,W,Cin,Cout,k,stride,pad", [(1, 20, 24, 48, 96, 3, 2, 1), (2, 9, 13, 64, 40, 1, 1, 0),
                                                          (1, 12, 16, 72, 88, 3, 1, 1), (1, 19, 1, 128, 64, 1, 1, 0)])
def test_exact_wgrad_splitk(B, H, W, Cin, Cout, k, stride, pad, cfg):
    """The split-K ssa_conv2d_wgrad + reduce (strided 3x3, 1x1, ragged channel counts, a one-pixel-wide image), and the
    bias gradient beside it: ssa_colsum_bf16 of the same dy, fp32, exact."""
    import ctypes
    from semseg_amd._lib import check
    _exact_wgrad("wgrad", B, H, W, Cin, Cout, k, stride, pad, cfg)
    hb = _hb()
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dy = ints((B, Ho, Wo, Cout), -3, 3, 43)
    gg = guarded_copy(dy.to(ACT_DTYPE), DEV, Cout + 8)
    out, scratch = guarded((Cout,), torch.float32, DEV), guarded((2 * Cout,), torch.float64, DEV)
    check(hb.lib().ssa_colsum_bf16(hb._p(gg.view), B * Ho * Wo, Cout, Cout + 8, hb._p(out.view), hb._p(scratch.view), hb._s()),
          "ssa_colsum_bf16")
    if DEV != "cpu":
        torch.cuda.synchronize()
    assert_bits_equal("bias gradient", out.view.cpu(), dy.double().view(-1, Cout).sum(0).float())
    assert_guard_intact("bias gradient", gg, out, scratch)


@pytest.mark.skipif(bool(os.environ.get("SSA_EMU")), reason="16,384 pixels at >= 128 channels: GPU only")
@pytest.mark.parametrize("B,H,W,Cin,Cout,k", [(1, 130, 131, 192, 200, 3), (2, 96, 100, 256, 72, 1), (1, 128, 129, 240, 128, 3)])
def test_exact_wgrad_head(B, H, W, Cin, Cout, k):
    """ssa_conv2d_wgrad_head + reduce (3x3 and 1x1, ragged tiles, channel-tile tails) at the sizes it takes."""
    _exact_wgrad("head", B, H, W, Cin, Cout, k, 1, k // 2, -1)


# ---- the BatchNorm kernels (csrc/bn.hip): ssa_bn_stats / apply / apply_train / bwd_reduce / bwd_apply / param_grads
# through the C ABI, every operand in a guarded buffer, at every grid regime of plan_grid / plan_reduce_grid.
from exact_util import choice, pow2, sign_bytes, split_replicas, split_replicas_real, to_f32, ulp_err32  # noqa: E402

# the switches csrc/bn.hip reads for its grids: with one of them set the mirror below describes another launch
_BN_TUNING = ("SSA_BN_WIDE_CHUNKS", "SSA_BN_ROWS_APPLY", "SSA_BN_ROWS_BWD", "SSA_BN_ROWS_REDUCE", "SSA_BN_REDUCE_BLOCKS")

# id, C, B, H, W
BN_CASES = [
    ("c8", 8, 2, 9, 11),            # VC = 1: one workgroup, P = 198 < RP = 256 -- most threads have no valid row at all
    ("c48", 48, 2, 17, 23),         # 252 of 256 threads active; 5 apply / 3 reduce workgroups, ragged last range
    ("c248", 248, 1, 37, 45),       # VC = 31 (248 active); the last workgroup's range is ONE pixel
    ("c720a", 720, 2, 65, 67),      # 180 active, RP = 2; apply walks 2 chunks (545 workgroups), last range 6 pixels < a chunk
    ("c256", 256, 2, 173, 191),     # RP = 8; apply walks 3 chunks, last range = one full chunk + a partial one
    ("c720b", 720, 2, 129, 131),    # apply walks 5 chunks, last range 4 full chunks + 6 pixels; reduce above its cap: 2 chunks
    ("c1032", 1032, 2, 97, 131),    # 129 of 256 threads active, prologue over C > 256 with idle threads; apply 6, reduce 2 chunks
    ("c2048", 2048, 3, 67, 61),     # RP = 1; apply walks 3 chunks; B = 3 for the per-image `post` index
]
_BN_IDS = [c[0] for c in BN_CASES]
# the full configuration matrices run on these; the others (17-26 M elements) run each kernel's richest configuration once
_BN_SMALL = ("c8", "c48", "c248", "c720a")


def _bn_plan(P, C, rows, max_blocks=16384, chunks=1):
    """Mirror of plan_grid (csrc/bn.hip) with the active-thread layout of the kernels: `rows` pixel rows per thread and
    chunk, at most max_blocks workgroups, `chunks` > 1 = the passes with a per-workgroup coefficient prologue."""
    VC = C // 8
    active = (256 // VC) * VC
    RP = active // VC
    chunk = RP * rows
    ppb = chunk
    blocks = -(-P // ppb)
    if chunks > 1 and blocks > 1024:
        max_blocks = min(max_blocks, max(1024, -(-blocks // chunks)))
    capped = blocks > max_blocks
    if capped:
        ppb = -(-(-(-P // max_blocks)) // chunk) * chunk
        blocks = -(-P // ppb)
    blocks = max(blocks, 1)
    return dict(VC=VC, active=active, RP=RP, chunk=chunk, ppb=ppb, blocks=blocks, chunks_per_wg=ppb // chunk,
                last=P - (blocks - 1) * ppb, capped=capped)


def _bn_plans(case):
    """The three launches of a case with the defaults of csrc/bn.hip: `apply` (ssa_bn_apply: 4 rows, one chunk),
    `train` (ssa_bn_apply_train and ssa_bn_bwd_apply: 4 rows, prologue_chunks = 6 from 256 channels on) and `reduce`
    (ssa_bn_stats and ssa_bn_bwd_reduce: 8 rows, at most 2048 workgroups)."""
    _, C, B, H, W = case
    P = B * H * W
    return dict(P=P, apply=_bn_plan(P, C, 4), train=_bn_plan(P, C, 4, 16384, 6 if C >= 256 else 1),
                reduce=_bn_plan(P, C, 8, 2048))


def _assert_bn_coverage(cases):
    """A condition on the case list (on the mirror, not on the kernel): a later edit cannot silently drop a regime."""
    plans = [(c, _bn_plans(c)) for c in cases]
    assert any(p["train"]["VC"] == 1 for _, p in plans), "no VC = 1 case"
    assert any(p["train"]["RP"] == 1 for _, p in plans), "no RP = 1 case"
    assert any(p["train"]["active"] < 192 for _, p in plans), "no case with fewer than 192 active threads"
    assert any(p["P"] < p["train"]["RP"] for _, p in plans), "no case with P < RP"
    assert any(p["train"]["last"] == 1 and p["train"]["blocks"] > 1 for _, p in plans), "no last range of one pixel"
    counts = {p["train"]["chunks_per_wg"] for _, p in plans}
    assert {1, 2, 3, 6} <= counts, counts
    assert any(p["train"]["chunks_per_wg"] >= 5 and p["train"]["last"] % p["train"]["chunk"] and
               p["train"]["last"] > p["train"]["chunk"] for _, p in plans), "no walk of >= 5 chunks with a partial last chunk"
    assert any(p["reduce"]["capped"] and p["reduce"]["chunks_per_wg"] > 1 for _, p in plans), "no reduce pass above its cap"
    assert any(c[2] >= 3 for c, _ in plans), "no case with B >= 3"
    for c, p in plans:
        assert c[1] % 8 == 0 and c[1] <= 2048 and (c[0] in _BN_SMALL) == (p["P"] * c[1] < 8e6), c


_assert_bn_coverage(BN_CASES)


def _bn_guard():
    """The exact BatchNorm tests describe the default grids: skip when a tuning switch of csrc/bn.hip is set."""
    on = [k for k in _BN_TUNING if k in os.environ]
    if on:
        pytest.skip("%s set: the grid mirror of the exact BatchNorm tests (_bn_plan) describes the default launch" % ", ".join(on))
    from semseg_amd._lib import check
    hb = _hb()
    return hb, hb.lib(), check


def _bn_sync():
    torch.cuda.synchronize()


def _ld(g):
    return g.view.stride(0)


def _pp(t):
    return _hb()._p(t.view) if t is not None else None


def _per_pixel(post, hw):
    """[B, C] per-image factors -> [P, C]"""
    return post.repeat_interleave(hw, 0)


def test_exact_bn_plan_mirror():
    """The regime each case of BN_CASES is listed for, as the mirror computes it."""
    p = {c[0]: _bn_plans(c) for c in BN_CASES}
    assert p["c8"]["train"]["VC"] == 1 and p["c8"]["train"]["blocks"] == 1 and p["c8"]["P"] == 198 < p["c8"]["train"]["RP"] == 256
    assert p["c48"]["train"]["active"] == 252 and (p["c48"]["apply"]["blocks"], p["c48"]["reduce"]["blocks"]) == (5, 3)
    assert p["c48"]["train"]["last"] % p["c48"]["train"]["chunk"] and p["c48"]["reduce"]["last"] % p["c48"]["reduce"]["chunk"]
    assert p["c248"]["train"]["VC"] == 31 and p["c248"]["train"]["active"] == 248 and p["c248"]["train"]["last"] == 1
    assert p["c248"]["reduce"]["last"] == 1
    t = p["c720a"]["train"]
    assert (t["active"], t["RP"], t["chunks_per_wg"], t["blocks"], t["last"]) == (180, 2, 2, 545, 6)
    t = p["c256"]["train"]
    assert t["RP"] == 8 and t["chunks_per_wg"] == 3 and t["chunk"] < t["last"] < 2 * t["chunk"]
    t, r = p["c720b"]["train"], p["c720b"]["reduce"]
    assert t["chunks_per_wg"] == 5 and t["last"] == 4 * t["chunk"] + 6 and r["capped"] and r["chunks_per_wg"] == 2
    t, r = p["c1032"]["train"], p["c1032"]["reduce"]
    assert t["active"] == 129 and t["chunks_per_wg"] == 6 and r["chunks_per_wg"] == 2
    t = p["c2048"]["train"]
    assert t["RP"] == 1 and t["chunks_per_wg"] == 3
    # the evaluation form: 8 channels over 16384 * 1024 + 517 pixels meets the 16,384-workgroup cap at 2 chunks
    e = _bn_plan(_BN_EVAL_P, 8, 4)
    assert e["capped"] and e["chunks_per_wg"] == 2 and e["blocks"] <= 16384


# ---- ssa_bn_stats
@pytest.mark.parametrize("case", BN_CASES, ids=_BN_IDS)
def test_exact_bn_stats(case):
    """Both rows of the sums equal to the int64 sums: no pixel missing, none counted twice, masked rows zeroed.  Twice
    into one buffer with zero_sums = 0 (accumulation) and once with zero_sums = 1 over a NaN-filled buffer; pixel
    stride C and C + 24 (NaN neighbours)."""
    hb, L, check = _bn_guard()
    name, C, B, H, W = case
    P = B * H * W
    x = ints((P, C), -4, 4, 300)
    assert_integers("bn_stats x", x)
    xi = x.long()
    want = torch.stack([xi.sum(0), (xi * xi).sum(0)]).double()
    assert_premise("sum of x^2 over the pixels", want[1])                # the fp32 partial sums of any workgroup are then exact
    for ld in ((C, C + 24) if name in _BN_SMALL else (C + 24,)):
        xg = guarded_copy(x.to(ACT_DTYPE), DEV, ld)
        acc = guarded((2, C), torch.float64, DEV)
        acc.view.zero_()
        fresh = guarded((2, C), torch.float64, DEV)                     # NaN: zero_sums = 1 has to clear it
        for _ in range(2):
            check(L.ssa_bn_stats(hb._p(xg.view), P, C, ld, hb._p(acc.view), 0, hb._s()), "ssa_bn_stats")
        check(L.ssa_bn_stats(hb._p(xg.view), P, C, ld, hb._p(fresh.view), 1, hb._s()), "ssa_bn_stats")
        _bn_sync()
        for what, got, k in (("zero_sums=1", fresh.view.cpu(), 1), ("accumulated twice", acc.view.cpu(), 2)):
            for row in (0, 1):
                assert torch.equal(got[row], k * want[row]), "bn_stats %s ld=%d %s row %d: %d channels differ; first %d" % (
                    name, ld, what, row, int((got[row] != k * want[row]).sum()), int((got[row] != k * want[row]).nonzero()[0]))
        assert_guard_intact("bn_stats %s" % name, xg, acc, fresh)


# ---- ssa_bn_apply
# |x|, |residual| up to this: integers the storage format holds (bf16: 8 bits, fp16: 11 bits), large enough that
# scale * x + shift + residual needs more bits than the format has -- the rounding decides bits in BOTH builds
_BN_AMP = 2000 if ACT_DTYPE == torch.float16 else 200
_BN_POST = [0.0, 0.5, 1.0, 2.0]


def _bn_apply_operands(C, B, P, seed):
    x = ints((P, C), -_BN_AMP, _BN_AMP, seed)
    r = ints((P, C), -_BN_AMP, _BN_AMP, seed + 1)
    scale = pow2((C,), -2, 2, seed + 2, signed=True)
    assert (scale > 0).any() and (scale < 0).any()
    shift = ints((C,), -50, 50, seed + 3)
    post = choice((B, C), _BN_POST, seed + 4)
    return x, r, scale, shift, post


def _bn_apply_ref(x, r, scale, shift, post_pp, relu):
    """z = post * act(scale * x + shift + residual) in float64: every step exact (dyadic operands of a few bits)."""
    f = x.double() * scale.double() + shift.double()
    if r is not None:
        f = f + r.double()
    if relu:
        f = torch.relu(f)
    if post_pp is not None:
        f = f * post_pp.double()
    return f


@pytest.mark.parametrize("case", BN_CASES, ids=_BN_IDS)
def test_exact_bn_apply(case):
    """z bit for bit, every element written (the buffer starts as NaN), nothing around it: relu x residual x post on
    the small cases (dense), and the richest form -- residual + relu + post with ldx, ldr, ldz all different from C --
    on every case.  Part of the outputs is not representable in the storage format: the rounding decides bits."""
    hb, L, check = _bn_guard()
    name, C, B, H, W = case
    P = B * H * W
    x, r, scale, shift, post = _bn_apply_operands(C, B, P, 310)
    assert_integers("bn_apply operands", x, r)
    post_pp = _per_pixel(post, H * W)
    cfgs = [(True, True, True, True)]
    if name in _BN_SMALL:
        cfgs += [(relu, res, pst, False) for relu in (False, True) for res in (False, True) for pst in (False, True)]
    sg, hg, pg = guarded_copy(scale, DEV), guarded_copy(shift, DEV), guarded_copy(post, DEV)
    for relu, res, pst, sliced in cfgs:
        ref = _bn_apply_ref(x, r if res else None, scale, shift, post_pp if pst else None, relu)
        assert float(ref.abs().max()) < 60000.0                         # finite in fp16
        want = to_act(ref)
        assert not_representable(ref) > 0, "no output of this configuration needs rounding"
        ldx, ldr, ldz = (C + 8, C + 16, C + 24) if sliced else (C, C, C)
        xg = guarded_copy(x.to(ACT_DTYPE), DEV, ldx)
        rg = guarded_copy(r.to(ACT_DTYPE), DEV, ldr) if res else None
        zg = guarded((P, C), ACT_DTYPE, DEV, ldz)
        check(L.ssa_bn_apply(hb._p(xg.view), ldx, _pp(rg), ldr if res else 0, hb._p(zg.view), ldz, P, C, hb._p(sg.view),
                             hb._p(hg.view), int(relu), hb._p(pg.view) if pst else None, H * W, hb._s()), "ssa_bn_apply")
        _bn_sync()
        tag = "bn_apply %s relu=%d res=%d post=%d sliced=%d" % (name, relu, res, pst, sliced)
        assert_bits_equal(tag, zg.view.cpu(), want)
        assert_guard_intact(tag, *[g for g in (xg, rg, zg, sg, hg, pg) if g is not None])


_BN_EVAL_P = 16384 * 1024 + 517


@pytest.mark.skipif(bool(os.environ.get("SSA_EMU")), reason="16.8 M pixels: GPU only")
def test_exact_bn_apply_eval_scale():
    """The form large-scale evaluation uses: 8 channels over 16384 * 1024 + 517 pixels -- the 16,384-workgroup cap of
    plan_grid at 2 chunks per workgroup (a ragged last one), pixel offsets beyond 2^24, images of 5,000,011 pixels (the
    last one shorter) for the per-image `post`.  The reference is integer arithmetic on the device: in units of 1/32
    every intermediate is an integer below 2^31, the value a float32 then holds exactly."""
    hb, L, check = _bn_guard()
    C, P, ppi = 8, _BN_EVAL_P, 5000011
    nimg = -(-P // ppi)
    g = torch.Generator(device=DEV).manual_seed(320)
    xi = torch.randint(-_BN_AMP, _BN_AMP + 1, (P, C), generator=g, device=DEV, dtype=torch.int32)
    ri = torch.randint(-_BN_AMP, _BN_AMP + 1, (P, C), generator=g, device=DEV, dtype=torch.int32)
    scale, shift, post = pow2((C,), -2, 2, 321, signed=True), ints((C,), -50, 50, 322), choice((nimg, C), _BN_POST, 323)
    xg, rg = guarded((P, C), ACT_DTYPE, DEV, C + 8), guarded((P, C), ACT_DTYPE, DEV, C + 16)
    xg.view.copy_(xi)
    rg.view.copy_(ri)
    assert torch.equal(xg.view.to(torch.int32), xi) and torch.equal(rg.view.to(torch.int32), ri)      # representable
    sg, hg, pg = guarded_copy(scale, DEV), guarded_copy(shift, DEV), guarded_copy(post, DEV)
    zg = guarded((P, C), ACT_DTYPE, DEV, C + 24)
    check(L.ssa_bn_apply(hb._p(xg.view), C + 8, hb._p(rg.view), C + 16, hb._p(zg.view), C + 24, P, C, hb._p(sg.view),
                         hb._p(hg.view), 1, hb._p(pg.view), ppi, hb._s()), "ssa_bn_apply")
    s4 = (scale * 4).to(torch.int32).to(DEV)                             # scale in quarters, post in halves: integers
    f = xi * s4 + (ri + shift.to(torch.int32).to(DEV)) * 4
    f = torch.clamp_min(f, 0)
    img = torch.div(torch.arange(P, device=DEV), ppi, rounding_mode="floor")
    f = f * (post * 2).to(torch.int32).to(DEV)[img]
    assert int(f.abs().max()) < 2 ** 24
    want = (f.to(torch.float32) / 8).to(ACT_DTYPE)
    assert int((want.float() * 8 != f).sum()) > 0, "no output needs rounding"
    torch.cuda.synchronize()
    if not torch.equal(zg.view.view(torch.int16), want.view(torch.int16)):
        bad = (zg.view.view(torch.int16) != want.view(torch.int16)).nonzero()
        p = int(bad[0][0])
        assert_bits_equal("bn_apply eval scale: %d elements differ, first pixel %d" % (bad.shape[0], p),
                          zg.view[p:p + 1].cpu(), want[p:p + 1].cpu())
    assert_guard_intact("bn_apply eval scale", xg, rg, zg, sg, hg, pg)


# ---- ssa_bn_bwd_reduce / ssa_bn_bwd_apply
def _bn_bwd_operands(case, seed):
    """dz, x integers in [-4, 4]; integer mean, invstd a power of two; post in {0, 0.5, 1, 2}; the forward whose ReLU the
    backward masks with is z = post * relu(mask_scale * x + mask_shift) with mask_scale = +-2^k and an integer
    mask_shift -- exact, many pre-activations exactly 0 (the comparisons are strict), and the same sign whether it is
    recomputed from x (mode 1), read off z (mode 2) or off the sign bytes built from z (mode 0)."""
    name, C, B, H, W = case
    P = B * H * W
    o = dict(P=P, C=C, hw=H * W)
    o["x"], o["dz"] = ints((P, C), -4, 4, seed), ints((P, C), -4, 4, seed + 1)
    o["mean"], o["invstd"] = ints((C,), -2, 2, seed + 2), pow2((C,), -2, 1, seed + 3)
    o["post"] = choice((B, C), _BN_POST, seed + 4)
    o["msc"], o["msh"] = pow2((C,), -1, 1, seed + 5, signed=True), ints((C,), -3, 3, seed + 6)
    assert_integers("bn_bwd operands", o["x"], o["dz"], o["mean"], o["msh"])
    pre = o["x"] * o["msc"] + o["msh"]                                   # exact in fp32: halves below 2^4
    assert int((pre == 0).sum()) > pre.numel() // 50, "too few pre-activations are exactly zero"
    o["pre_pos"] = pre > 0
    z = torch.relu(pre)
    o["z_post"] = to_act((z * _per_pixel(o["post"], H * W)).double())    # the forward's z with post, and without
    o["z_plain"] = to_act(z.double())
    return o


def _bn_bwd_masked_g(o, mode, post_on):
    """(g, float32 [P, C]: post * dz where the ReLU of `mode` lets it through, +0 elsewhere; the z the kernel is given).
    mode: 'bits' / 'z' -- the mask is z > 0 of the STORED z (0 where post is 0); 'x' -- recomputed, pre-activation > 0;
    'norelu' -- no mask."""
    g = o["dz"] * _per_pixel(o["post"], o["hw"]) if post_on else o["dz"].clone()
    z = o["z_post"] if post_on else o["z_plain"]
    if mode == "norelu":
        return g, z
    m = o["pre_pos"] if mode == "x" else (z > 0)
    return torch.where(m, g, torch.zeros(())), z


def _bn_bwd_buffers(hb, o, mode, z, post_on, sliced):
    C = o["C"]
    lds = (C + 8, C + 16, C + 24) if sliced else (C, C, C)
    b = dict(x=guarded_copy(o["x"].to(ACT_DTYPE), DEV, lds[0]), dz=guarded_copy(o["dz"].to(ACT_DTYPE), DEV, lds[1]),
             mean=guarded_copy(o["mean"], DEV), invstd=guarded_copy(o["invstd"], DEV),
             post=guarded_copy(o["post"], DEV) if post_on else None,
             z=guarded_copy(z, DEV, lds[2]) if mode == "z" else None,
             mask=guarded_copy(sign_bytes(z), DEV) if mode == "bits" else None,
             msc=guarded_copy(o["msc"], DEV) if mode == "x" else None, msh=guarded_copy(o["msh"], DEV) if mode == "x" else None)
    return b


_BN_MODES = ("bits", "x", "z", "norelu")


@pytest.mark.parametrize("case", BN_CASES, ids=_BN_IDS)
def test_exact_bn_bwd_reduce(case):
    """sum(m g) and invstd (sum(m g x) - mean sum(m g)), g = post dz, summed over the replicas, equal to float64 with
    torch.equal -- for the three sources of the ReLU mask (which must also agree with one another) and without ReLU,
    nrep in {1, ssa_bn_stat_replicas(), 11}, with zero_sums = 1 over NaN and zero_sums = 0 over zeros."""
    hb, L, check = _bn_guard()
    name, C, B, H, W = case
    o = _bn_bwd_operands(case, 330)
    P = o["P"]
    reps = (1, hb.stat_replicas(), 11)
    if name in _BN_SMALL:
        cfgs = [(mode, nrep, not (mode == "x" and nrep == 1), i % 2 == 1)
                for i, (mode, nrep) in enumerate((m, n) for m in _BN_MODES for n in reps)]
    else:
        cfgs = [("bits", hb.stat_replicas(), True, True)]               # the sign-byte reload of the later chunks
    seen = {}
    for k, (mode, nrep, post_on, sliced) in enumerate(cfgs):
        g, z = _bn_bwd_masked_g(o, mode, post_on)
        gd, xd, mu, inv = g.double(), o["x"].double(), o["mean"].double(), o["invstd"].double()
        # in units of 2^-3 (g in halves, invstd >= 2^-2) every per-thread and per-workgroup fp32 sum is an integer < 2^24
        assert_premise("bn_bwd_reduce", 8 * inv * ((gd.abs() * xd.abs()).sum(0) + mu.abs() * gd.abs().sum(0)))
        s1 = gd.sum(0)
        want = torch.stack([s1, inv * ((gd * xd).sum(0) - mu * s1)])
        b = _bn_bwd_buffers(hb, o, mode, z, post_on, sliced)
        zero = k % 2
        sums = guarded((nrep, 2, C), torch.float64, DEV)
        if not zero:
            sums.view.zero_()
        check(L.ssa_bn_bwd_reduce(hb._p(b["x"].view), _ld(b["x"]), hb._p(b["dz"].view), _ld(b["dz"]), _pp(b["z"]),
                                  _ld(b["z"]) if b["z"] else 0, P, C, hb._p(b["mean"].view), hb._p(b["invstd"].view),
                                  int(mode != "norelu"), _pp(b["post"]), H * W, hb._p(sums.view), nrep, zero,
                                  _pp(b["msc"]), _pp(b["msh"]), _pp(b["mask"]), hb._s()), "ssa_bn_bwd_reduce")
        _bn_sync()
        tag = "bn_bwd_reduce %s mode=%s nrep=%d post=%d sliced=%d" % (name, mode, nrep, post_on, sliced)
        got = sums.view.sum(0).cpu()
        for row in (0, 1):
            assert torch.equal(got[row], want[row]), "%s row %d: %d channels differ; first %d" % (
                tag, row, int((got[row] != want[row]).sum()), int((got[row] != want[row]).nonzero()[0]))
        assert_guard_intact(tag, sums, *[v for v in b.values() if v is not None])
        if mode != "norelu" and post_on:
            seen.setdefault(mode, got)
    for mode in seen:                                                   # the three mask sources agree bit for bit
        assert_bits_equal("bn_bwd_reduce %s: mode %s against mode bits" % (name, mode), seen[mode], seen["bits"])
    assert len(seen) == (3 if name in _BN_SMALL else 1)


@pytest.mark.parametrize("case", BN_CASES, ids=_BN_IDS)
def test_exact_bn_bwd_apply(case):
    """dx = A g + Bx x + D and dres = g bit for bit, from sums the test supplies: c1 = s1 / count, c2 = s2 / count small
    integers (count a power of two), split over nrep replicas as large integer-valued pieces of mixed sign; gamma in
    {+-1, +-2, 0.5} or NULL, so that A, Bx, D are dyadic with a few bits and every fp32 step is exact.  dgamma / dbeta =
    s * param_grad_scale: written over NaN, added onto an integer pre-fill, or left alone (null pointers)."""
    hb, L, check = _bn_guard()
    name, C, B, H, W = case
    o = _bn_bwd_operands(case, 340)
    P = o["P"]
    count = 1024.0
    c = torch.stack([ints((C,), -12, 12, 347), ints((C,), -12, 12, 348)]).double()
    gamma = choice((C,), [1.0, -1.0, 2.0, -2.0, 0.5], 349)
    reps = (1, hb.stat_replicas(), 11)
    if name in _BN_SMALL:
        cfgs = [dict(mode=m, nrep=n, post=i % 4 != 3, sliced=i % 2 == 1, dres=i % 3 != 2, gamma=i % 5 != 4,
                     pg=("write", "acc", "null")[i % 3], pgs=(1.0, 0.5)[(i // 3) % 2])
                for i, (m, n) in enumerate((m, n) for m in _BN_MODES for n in reps)]
    else:
        cfgs = [dict(mode="bits", nrep=11, post=True, sliced=True, dres=True, gamma=True, pg="acc", pgs=0.5)]
    rounded = 0
    for k, cf in enumerate(cfgs):
        mode, nrep = cf["mode"], cf["nrep"]
        g, z = _bn_bwd_masked_g(o, mode, cf["post"])
        gd, xd, mu, inv = g.double(), o["x"].double(), o["mean"].double(), o["invstd"].double()
        A = (gamma.double() if cf["gamma"] else 1.0) * inv
        Bx = -A * c[1] * inv
        D = A * (c[1] * inv * mu - c[0])
        dx64 = A * gd + (Bx * xd + D)
        dx = to_act(dx64)                                               # (to_act asserts that fp32 holds it exactly)
        rounded += int((dx.double() != dx64).sum())
        dres = to_act(gd)
        pieces = split_replicas(c * count, nrep, 350 + k)
        b = _bn_bwd_buffers(hb, o, mode, z, cf["post"], cf["sliced"])
        sums = guarded_copy(pieces, DEV)
        gam = guarded_copy(gamma, DEV) if cf["gamma"] else None
        ldo = (C + 32, C + 40) if cf["sliced"] else (C, C)
        dxg = guarded((P, C), ACT_DTYPE, DEV, ldo[0])
        drg = guarded((P, C), ACT_DTYPE, DEV, ldo[1]) if cf["dres"] else None
        pre = ints((2, C), -9, 9, 360 + k)
        pgb = None
        if cf["pg"] != "null":
            pgb = guarded((2, C), torch.float32, DEV)                   # [0] dgamma, [1] dbeta; NaN unless accumulated onto
            if cf["pg"] == "acc":
                pgb.view.copy_(pre)
        check(L.ssa_bn_bwd_apply(hb._p(b["x"].view), _ld(b["x"]), hb._p(b["dz"].view), _ld(b["dz"]), _pp(b["z"]),
                                 _ld(b["z"]) if b["z"] else 0, hb._p(dxg.view), ldo[0], _pp(drg), ldo[1] if drg else 0, P, C,
                                 _pp(gam), hb._p(b["mean"].view), hb._p(b["invstd"].view), hb._p(sums.view), nrep, count,
                                 int(mode != "norelu"), _pp(b["post"]), H * W,
                                 hb._p(pgb.view[0]) if pgb else None, hb._p(pgb.view[1]) if pgb else None, cf["pgs"],
                                 _pp(b["msc"]), _pp(b["msh"]), int(cf["pg"] == "acc"), _pp(b["mask"]), hb._s()),
              "ssa_bn_bwd_apply")
        _bn_sync()
        tag = "bn_bwd_apply %s %s" % (name, " ".join("%s=%s" % kv for kv in sorted(cf.items())))
        assert_bits_equal(tag + " dx", dxg.view.cpu(), dx)
        if drg:
            assert_bits_equal(tag + " dres", drg.view.cpu(), dres)
        if pgb:
            wantpg = torch.stack([c[1], c[0]]) * count * cf["pgs"] + (pre.double() if cf["pg"] == "acc" else 0.0)
            assert_bits_equal(tag + " dgamma, dbeta", pgb.view.cpu(), to_f32(wantpg))
        assert_guard_intact(tag, sums, dxg, *[v for v in list(b.values()) + [gam, drg, pgb] if v is not None])
    # dx = A (g - c1 - c2 invstd (x - mean)), A a power of two: at invstd = 2 the bracket has steps of 1/2 (post = 0.5, odd dz)
    # at magnitudes up to 8 + 12 + 12 * 2 * 6 = 164 -- 9 bits: the 8 bits of bf16 do not hold it and the rounding decides
    # bits (the 11 bits of fp16 do hold it: as for the strip statistics the requirement can only be met in bf16; a
    # case of few channels may draw no such coefficients)
    if ACT_DTYPE == torch.bfloat16 and C >= 200:
        assert rounded > 0, "no dx of %s needs rounding" % name


@pytest.mark.parametrize("C", [8, 200, 720])
def test_exact_bn_param_grads(C):
    """ssa_bn_param_grads: dbeta / dgamma are the fp32 casts (round to nearest even) of the given fp64 sums; C = 200 and
    720 are no multiple of the 128-thread workgroup; one pointer NULL leaves only the other written."""
    hb, L, check = _bn_guard()
    g = torch.Generator().manual_seed(370 + C)
    s = (torch.rand(2, C, generator=g, dtype=torch.float64) - 0.5) * 1e5
    assert int((s.float().double() != s).sum()) > C                      # the cast rounds
    sums = guarded_copy(s, DEV)
    out = guarded((2, C), torch.float32, DEV)
    only = guarded((C,), torch.float32, DEV)
    check(L.ssa_bn_param_grads(hb._p(sums.view), C, hb._p(out.view[0]), hb._p(out.view[1]), hb._s()), "ssa_bn_param_grads")
    check(L.ssa_bn_param_grads(hb._p(sums.view), C, None, hb._p(only.view), hb._s()), "ssa_bn_param_grads")
    _bn_sync()
    assert_bits_equal("bn_param_grads dgamma", out.view[0].cpu(), s[1].float())
    assert_bits_equal("bn_param_grads dbeta", out.view[1].cpu(), s[0].float())
    assert_bits_equal("bn_param_grads dbeta alone", only.view.cpu(), s[0].float())
    assert_guard_intact("bn_param_grads", sums, out, only)


# ---- ssa_bn_apply_train: 1 / sqrt is v_rsq_f32 plus a Newton step, not bit-predictable -- a chain through the exact test
_F32_MOM, _F32_EPS = float(torch.tensor(0.1, dtype=torch.float32)), float(torch.tensor(1e-5, dtype=torch.float32))


def _bn_train_launch(hb, L, check, d, nrep, count, relu, res, pst, sliced, mask_on, track):
    """One ssa_bn_apply_train launch; returns the guarded buffers."""
    P, C, hw = d["P"], d["C"], d["hw"]
    lds = (C + 8, C + 16, C + 24) if sliced else (C, C, C)
    b = dict(x=guarded_copy(d["x"], DEV, lds[0]), res=guarded_copy(d["r"], DEV, lds[1]) if res else None,
             z=guarded((P, C), ACT_DTYPE, DEV, lds[2]), sums=guarded_copy(d["pieces"][nrep], DEV),
             gamma=guarded_copy(d["gamma"], DEV), beta=guarded_copy(d["beta"], DEV),
             post=guarded_copy(d["post"], DEV) if pst else None, coef=guarded((4, C), torch.float32, DEV),
             mask=guarded((P, C // 8), torch.uint8, DEV) if mask_on else None,
             rm=guarded_copy(d["rm"], DEV) if track else None, rv=guarded_copy(d["rv"], DEV) if track else None,
             ps=guarded((2 * C + 1,), torch.float32, DEV) if track else None,
             nbt=guarded_copy(torch.tensor([5], dtype=torch.int64), DEV) if track else None)
    check(L.ssa_bn_apply_train(hb._p(b["x"].view), lds[0], _pp(b["res"]), lds[1] if res else 0, hb._p(b["z"].view), lds[2],
                               P, C, hb._p(b["sums"].view), nrep, float(count), hb._p(b["gamma"].view), hb._p(b["beta"].view),
                               _pp(b["rm"]), _pp(b["rv"]), _pp(b["nbt"]), _F32_MOM, _F32_EPS, hb._p(b["coef"].view),
                               _pp(b["ps"]), int(relu), _pp(b["post"]), hw, _pp(b["mask"]), hb._s()), "ssa_bn_apply_train")
    _bn_sync()
    return b


@pytest.mark.parametrize("case", BN_CASES, ids=_BN_IDS)
def test_exact_bn_apply_train(case):
    """Real-valued data, the sums supplied by the test (the fp64 statistics of that data split over nrep replicas):
    (1) the coefficient table, the running statistics, pass_stats and num_batches_tracked against float64 -- mean, var,
        running statistics within 1 fp32 ulp; invstd and scale within 4 (a 1-ulp seed after one Newton step leaves the
        rounding of its four fp32 operations, about 2 ulp: the bound doubles that); shift within
        2^-21 (|beta| + |mean gamma invstd|);
    (2) z BIT-EQUAL to ssa_bn_apply -- pinned exactly by test_exact_bn_apply -- given the scale and shift the kernel
        itself published (both run bn_apply_rows);
    (3) the sign mask byte-equal to the bits of the kernel's own z.
    sign_mask = NULL, and null running pointers / pass_stats / num_batches_tracked, change nothing else.
    Measured on the MI355X over all cases and both storage builds (profiles/bn_exact_gpu_tests.log): mean, var and
    running statistics <= 0.50 ulp, invstd <= 1.14, scale <= 2.00, shift <= 1.3e-7 of its scale (bound 4.8e-7)."""
    hb, L, check = _bn_guard()
    name, C, B, H, W = case
    P = B * H * W
    d = dict(P=P, C=C, hw=H * W)
    d["x"] = bf16_round(_rand(P, C, seed=380) * 1.7 + 0.3).to(ACT_DTYPE)
    d["r"] = _rand(P, C, seed=381).to(ACT_DTYPE)
    g = torch.Generator().manual_seed(382)
    d["gamma"] = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g).float() * 2 - 1)
    d["beta"] = torch.randn(C, generator=g) * 0.3
    d["rm"], d["rv"] = torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5
    d["post"] = choice((B, C), _BN_POST, 383)
    xd = d["x"].double()
    stats = torch.stack([xd.sum(0), (xd * xd).sum(0)])
    del xd
    reps = (1, hb.stat_replicas(), 11)
    d["pieces"], d["acc"] = {}, {}
    for nrep in reps:
        d["pieces"][nrep], d["acc"][nrep] = split_replicas_real(stats, nrep, 384 + nrep)
    small = name in _BN_SMALL
    # nrep, count / P, relu, residual, post, sliced
    cfgs = [(11, 1, True, True, True, True)]
    if small:
        cfgs += [(1, 1, False, False, False, False), (reps[1], 3, True, False, True, False), (reps[1], 1, False, True, False, True)]
    for nrep, mult, relu, res, pst, sliced in cfgs:
        count = float(P * mult)                                         # a multiple of P: SyncBN's global count
        b = _bn_train_launch(hb, L, check, d, nrep, count, relu, res, pst, sliced, True, True)
        tag = "bn_apply_train %s nrep=%d count=%dP relu=%d res=%d post=%d sliced=%d" % (name, nrep, mult, relu, res, pst, sliced)
        # ---- (1) the coefficients against float64
        S = d["acc"][nrep]
        mean = S[0] / count
        var = torch.clamp_min(S[1] / count - mean * mean, 0.0)
        invstd = 1.0 / torch.sqrt(var + _F32_EPS)
        gm, bt = d["gamma"].double(), d["beta"].double()
        coef = b["coef"].view.cpu()
        ps = b["ps"].view.cpu()
        unbiased = var * count / (count - 1.0)
        e = dict(mean=ulp_err32(coef[2], mean).max(), invstd=ulp_err32(coef[3], invstd).max(),
                 scale=ulp_err32(coef[0], gm * invstd).max(), pass_mean=ulp_err32(ps[:C], mean).max(),
                 pass_var=ulp_err32(ps[C:2 * C], var).max(),
                 running_mean=ulp_err32(b["rm"].view.cpu(), (1.0 - _F32_MOM) * d["rm"].double() + _F32_MOM * mean).max(),
                 running_var=ulp_err32(b["rv"].view.cpu(), (1.0 - _F32_MOM) * d["rv"].double() + _F32_MOM * unbiased).max())
        shift_ref = bt - mean * gm * invstd
        shift_rel = ((coef[1].double() - shift_ref).abs() / (bt.abs() + (mean * gm * invstd).abs())).max()
        print("[%s] max error in fp32 ulp: %s; shift: %.3g of |beta| + |mean gamma invstd| (bound 2^-21 = %.3g)" % (
            tag, ", ".join("%s %.3f" % (k, float(v)) for k, v in e.items()), float(shift_rel), 2.0 ** -21))
        for k, v in e.items():
            assert float(v) <= (4.0 if k in ("invstd", "scale") else 1.0), "%s: %s off by %.3f fp32 ulp" % (tag, k, float(v))
        assert float(shift_rel) <= 2.0 ** -21, "%s: shift off by %.3g" % (tag, float(shift_rel))
        assert float(ps[2 * C]) == count and int(b["nbt"].view) == 6
        # ---- (2) z against ssa_bn_apply with the published scale and shift
        lds = (_ld(b["x"]), _ld(b["res"]) if res else 0, _ld(b["z"]))
        z2 = guarded((P, C), ACT_DTYPE, DEV, lds[2])
        check(L.ssa_bn_apply(hb._p(b["x"].view), lds[0], _pp(b["res"]), lds[1], hb._p(z2.view), lds[2], P, C,
                             hb._p(b["coef"].view[0]), hb._p(b["coef"].view[1]), int(relu), _pp(b["post"]), H * W, hb._s()),
              "ssa_bn_apply")
        _bn_sync()
        zc = b["z"].view.cpu()
        assert not bool(torch.isnan(zc.float()).any()), tag + ": z has unwritten elements"
        assert_bits_equal(tag + " z against ssa_bn_apply", zc, z2.view.cpu())
        # ---- (3) the sign bytes are the bits of the kernel's own z
        assert_bits_equal(tag + " sign mask", b["mask"].view.cpu(), sign_bytes(zc))
        assert_guard_intact(tag, z2, *[v for v in b.values() if v is not None])
        if not small:
            continue
        # ---- without the mask, and without the running statistics / pass_stats / num_batches_tracked: the rest unchanged
        for mask_on, track in ((False, True), (True, False)):
            b2 = _bn_train_launch(hb, L, check, d, nrep, count, relu, res, pst, sliced, mask_on, track)
            for k in ("z", "coef") + (("mask",) if mask_on else ()) + (("rm", "rv", "ps", "nbt") if track else ()):
                assert_bits_equal("%s mask=%d track=%d: %s" % (tag, mask_on, track, k), b2[k].view.cpu(), b[k].view.cpu())
            assert_guard_intact(tag, *[v for v in b2.values() if v is not None])


# ---- parity additions (oracle/ops.py, the tolerances of test_bn_train)
@pytest.mark.parametrize("param", [False, True], ids=["tensor", "param"])
@pytest.mark.parametrize("relu", [False, True], ids=["norelu", "relu"])
@pytest.mark.parametrize("C", [48, 720])
def test_bn_eval_backward(C, relu, param):
    """Evaluation-mode BatchNorm under autograd (frozen statistics, trainable affine): dx = gamma invstd g and the
    parameter gradients from ssa_bn_bwd_reduce + ssa_bn_param_grads; `param`: gamma / beta are registered step
    parameters, i.e. their gradients are ACCUMULATED into the gradient arena and published at the end of backward."""
    from oracle import ops as O
    hb = _hb()
    B, H, W = 2, 17, 23
    x = bf16_round(_rand(B, C, H, W, seed=1) * 1.7 + 0.3)
    g = torch.Generator().manual_seed(400 + C)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    rm, rv = torch.randn(C, generator=g) * 0.2 + 0.3, torch.rand(C, generator=g) * 2 + 1.5
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = O.batch_norm(xr, gr, br, rm.clone(), rv.clone(), False)
    if relu:
        y = torch.relu(y)
    gy = _rand(B, C, H, W, seed=3)
    y.backward(gy)
    hb.begin_step(torch.device(DEV))
    xd = _to_dev_nhwc(x).requires_grad_(True)
    if param:
        gd, bd = torch.nn.Parameter(gamma.to(DEV)), torch.nn.Parameter(beta.to(DEV))
    else:
        gd, bd = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    z = hb.BatchNormActFn.apply(xd, gd, bd, None, None, rm.to(DEV), rv.to(DEV), None, 0.1, 1e-5, False, relu, False)
    z.backward(nhwc(gy).to(DEV).to(ACT_DTYPE))
    torch.cuda.synchronize()
    check_close("bn_eval_fwd", nchw(z.float()), y)
    check_close("bn_eval_dx", nchw(xd.grad.float()), xr.grad, 2e-2, 6e-3)
    check_close("bn_eval_dgamma", gd.grad, gr.grad, 1e-2, 4e-3)
    check_close("bn_eval_dbeta", bd.grad, br.grad, 1e-2, 4e-3)


@pytest.mark.skipif(bool(os.environ.get("SSA_EMU")), reason="24 M elements: GPU only")
def test_bn_train_large_mean():
    """test_bn_train's body at x = 6 + N(0, 1), a mean / std of 6, on case c720b (33,798 pixels: the reduce pass walks
    two chunks of 8 rows per thread): guards the (sum g x - mean sum g) invstd centring, done per thread in fp32 by
    design.  Without ReLU: over 24 M elements some pre-activations lie within an fp32 rounding of zero, where the oracle's
    mask and the kernel's may differ by a whole element -- not what this test is about.  The existing tolerances are asserted; the relative error of dgamma against float64 is printed beside the
    same figure for centred data (MI355X: 2.4e-7 against 7.9e-8 of max|dgamma|; fp16 build 1.4e-6 against 9.6e-8)."""
    from oracle import ops as O
    hb = _hb()
    case = dict(zip(_BN_IDS, BN_CASES))["c720b"]
    _, C, B, H, W = case
    g = torch.Generator().manual_seed(410)
    n = bf16_round(torch.randn(B, C, H, W, generator=g))
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    gy = _rand(B, C, H, W, seed=3)
    gyd = nhwc(gy).to(DEV).to(ACT_DTYPE)

    def device(x):
        xd = _to_dev_nhwc(x).requires_grad_(True)
        gd, bd = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
        rmd, rvd = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        nbt = torch.zeros((), dtype=torch.long, device=DEV)
        z = hb.BatchNormActFn.apply(xd, gd, bd, None, None, rmd, rvd, nbt, 0.1, 1e-5, True, False, False, None)
        z.backward(gyd)
        torch.cuda.synchronize()
        return z, xd.grad, gd.grad, bd.grad, rmd, rvd

    def dgamma64(x):
        xd = x.double()
        mean = xd.mean((0, 2, 3), keepdim=True)
        var = (xd * xd).mean((0, 2, 3), keepdim=True) - mean * mean
        xd.sub_(mean).mul_(1.0 / torch.sqrt(var + 1e-5)).mul_(gy)
        return xd.sum((0, 2, 3))

    def rel(a, ref):
        return float((a.double().cpu() - ref).abs().max() / ref.abs().max())

    x = bf16_round(n + 6.0)
    z, dx, dg, db, rmd, rvd = device(x)
    err_far = rel(dg, dgamma64(x))
    err_centred = rel(device(n)[2], dgamma64(n))
    print("[bn_train_large_mean] dgamma against float64: max error / max|dgamma| = %.3g at mean / std = 6, %.3g on centred data"
          % (err_far, err_centred))
    rm, rv = torch.zeros(C), torch.ones(C)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = O.batch_norm(xr, gr, br, rm, rv, True, 0.1, 1e-5)
    y.backward(gy)
    check_close("bn_fwd", nchw(z.float()), y)
    check_close("bn_running_mean", rmd, rm, 1e-4, 1e-4)
    check_close("bn_running_var", rvd, rv, 1e-4, 1e-4)
    check_close("bn_dx", nchw(dx.float()), xr.grad, 2e-2, 6e-3)
    check_close("bn_dgamma", dg, gr.grad, 1e-2, 4e-3)
    check_close("bn_dbeta", db, br.grad, 1e-2, 4e-3)


# ================================================================ exact resampling and pooling tests
# csrc/resample.hip and csrc/pool.hip through the C ABI, bit for bit against tests/resample_ref.py at power-of-two resize
# ratios (the premise is asserted on the reference), per element within resize_bound elsewhere.  Every input sits in a
# NaN-guarded buffer, every output starts as NaN; the case tables are tests/resample_cases.py.
import resample_cases as RC  # noqa: E402
from exact_util import LIMIT, assert_within_bound  # noqa: E402
from resample_ref import (exact_grad_x, exact_resize, exact_resize_grad, grad_amp, half_ulp_act, is_dyadic, resize_bound,  # noqa: E402
                          resize_grad_ref64, resize_ref64)

_GRID_CAP = 8192 * 256            # grid_for of csrc/resample.hip: threads in flight before a kernel's grid-stride loop turns
_TILE_CAP = 16384                 # workgroups of the LDS-tiled backward (4 x 16 input pixels each)


def _rs():
    from semseg_amd._lib import check
    hb = _hb()
    return hb, hb.lib(), check


def _rs_dt(is16):
    return ACT_DTYPE if is16 else torch.float32


def _rs_want(ref64, is16):
    return to_act(ref64) if is16 else to_f32(ref64)


def _ld4(g):
    return g.view.stride(2)


def _rs_fwd(x, in16, out16, Ho, Wo, pads=(0, 0)):
    """x [B, Hi, Wi, C] (host) through ssa_bilinear_fwd: (guarded input, guarded output)."""
    hb, L, check = _rs()
    Bn, Hi, Wi, C = x.shape
    xg = guarded_copy(x.to(_rs_dt(in16)), DEV, C + pads[0])
    yg = guarded((Bn, Ho, Wo, C), _rs_dt(out16), DEV, C + pads[1])
    check(L.ssa_bilinear_fwd(hb._p(xg.view), 0 if in16 else 1, Bn, Hi, Wi, C, _ld4(xg), hb._p(yg.view), 0 if out16 else 1,
                             Ho, Wo, _ld4(yg), hb._s()), "ssa_bilinear_fwd")
    return xg, yg


def _rs_bwd(dy, dy16, dx16, Hi, Wi, pads=(0, 0)):
    hb, L, check = _rs()
    Bn, Ho, Wo, C = dy.shape
    dyg = guarded_copy(dy.to(_rs_dt(dy16)), DEV, C + pads[0])
    dxg = guarded((Bn, Hi, Wi, C), _rs_dt(dx16), DEV, C + pads[1])
    check(L.ssa_bilinear_bwd(hb._p(dyg.view), 0 if dy16 else 1, Bn, Ho, Wo, C, _ld4(dyg), hb._p(dxg.view), 0 if dx16 else 1,
                             Hi, Wi, _ld4(dxg), hb._s()), "ssa_bilinear_bwd")
    return dyg, dxg


def _rs_bwd_sep(dy, dy16, dx16, Hi, Wi, pads=(0, 0)):
    """The separable pair: (guarded dy, guarded fp32 tmp [B, Ho, Wi, C], guarded dx)."""
    hb, L, check = _rs()
    Bn, Ho, Wo, C = dy.shape
    dyg = guarded_copy(dy.to(_rs_dt(dy16)), DEV, C + pads[0])
    tg = guarded((Bn, Ho, Wi, C), torch.float32, DEV)
    dxg = guarded((Bn, Hi, Wi, C), _rs_dt(dx16), DEV, C + pads[1])
    check(L.ssa_bilinear_bwd_x(hb._p(dyg.view), 0 if dy16 else 1, Bn, Ho, Wo, C, _ld4(dyg), hb._p(tg.view), Wi, hb._s()),
          "ssa_bilinear_bwd_x")
    check(L.ssa_bilinear_bwd_y(hb._p(tg.view), Bn, Ho, Wi, C, hb._p(dxg.view), 0 if dx16 else 1, Hi, _ld4(dxg), hb._s()),
          "ssa_bilinear_bwd_y")
    return dyg, tg, dxg


# ---- 3a: exact by route
@pytest.mark.parametrize("case", RC.FWD_EXACT, ids=[c[0] for c in RC.FWD_EXACT])
def test_exact_bilinear_fwd(case):
    """ssa_bilinear_fwd bit for bit on its three kernels (8 channels per thread, per pixel, per element in the four dtype
    pairs), dense and with leading dimensions that differ from C."""
    name, C, Hi, Wi, Ho, Wo, in16, out16, pads = case
    x = RC.fwd_operand(case)
    ref = exact_resize(name, x, Ho, Wo)
    xg, yg = _rs_fwd(x, in16, out16, Ho, Wo, pads)
    torch.cuda.synchronize()
    assert_bits_equal("bilinear_fwd %s" % name, yg.view.cpu(), _rs_want(ref, out16))
    assert_guard_intact("bilinear_fwd %s" % name, xg, yg)


@pytest.mark.parametrize("case", RC.BWD_EXACT, ids=[c[0] for c in RC.BWD_EXACT])
def test_exact_bilinear_bwd(case):
    """ssa_bilinear_bwd bit for bit: the vectorised gather (hoisted and recomputed weights), the per-element gather and
    the LDS-tiled kernel (TAPS 4 and 8; 8 and 32 channels; ragged, full and one-pixel tiles)."""
    name, C, Hi, Wi, Ho, Wo, dy16, dx16, pads = case
    dy = RC.bwd_operand(case)
    ref = exact_resize_grad(name, dy, Hi, Wi)
    dyg, dxg = _rs_bwd(dy, dy16, dx16, Hi, Wi, pads)
    torch.cuda.synchronize()
    assert_bits_equal("bilinear_bwd %s" % name, dxg.view.cpu(), _rs_want(ref, dx16))
    assert_guard_intact("bilinear_bwd %s" % name, dyg, dxg)


@pytest.mark.parametrize("case", RC.SEP_EXACT, ids=[c[0] for c in RC.SEP_EXACT])
def test_exact_bilinear_bwd_separable(case):
    """ssa_bilinear_bwd_x then _y: the fp32 intermediate AND the result bit for bit (a failure is located to a pass), and
    the one-launch form ssa_bilinear_bwd of the same problem equal to the same reference."""
    name, C, Hi, Wi, Ho, Wo, dy16, dx16, pads = case
    dy = RC.bwd_operand(case)
    ref = exact_resize_grad(name, dy, Hi, Wi)
    tref = exact_grad_x(name, dy, Wi)
    dyg, tg, dxg = _rs_bwd_sep(dy, dy16, dx16, Hi, Wi, pads)
    torch.cuda.synchronize()
    assert_bits_equal("bilinear_bwd_x %s" % name, tg.view.cpu(), to_f32(tref))
    assert_bits_equal("bilinear_bwd_y %s" % name, dxg.view.cpu(), _rs_want(ref, dx16))
    assert_guard_intact("bilinear_bwd_x/_y %s" % name, dyg, tg, dxg)
    if dy16 == dx16 or not dy16:                          # (ssa_bilinear_bwd has no 16-bit -> fp32 form)
        dyg2, dxg2 = _rs_bwd(dy, dy16, dx16, Hi, Wi, pads)
        torch.cuda.synchronize()
        assert_bits_equal("bilinear_bwd (one launch) %s" % name, dxg2.view.cpu(), _rs_want(ref, dx16))
        assert_guard_intact("bilinear_bwd (one launch) %s" % name, dyg2, dxg2)


# the Python dispatch: (id, C, Hi, Wi, Ho, Wo, x 16-bit, output fp32, layout)
_RS_AUTOGRAD = [
    ("v8-separable", 48, 5, 7, 20, 28, True, False, "dense"),          # separable() true: bwd_x / bwd_y
    ("v8-separable-2x4", 48, 5, 7, 10, 28, True, False, "dense"),
    ("v8-gather-down", 48, 12, 20, 6, 10, True, False, "dense"),       # separable() false: the vectorised gather
    ("v8-gather-2x-by-1x", 48, 5, 7, 10, 7, True, False, "dense"),     # one axis below 2x: separable() false
    ("v8-slices", 48, 5, 7, 10, 14, True, False, "slices"),            # x a channel slice; dy a slice with ld % 8 != 0: re-packed
    ("px-tile", 19, 9, 21, 36, 84, False, True, "dense"),
    ("px16-tile16", 19, 9, 21, 36, 84, True, True, "dense"),
    ("px-tile-slices", 19, 9, 21, 18, 42, False, True, "slices"),
    ("el-f32", 40, 9, 21, 18, 42, False, True, "dense"),
    ("el-16", 19, 6, 10, 12, 20, True, False, "slices"),
]


@pytest.mark.parametrize("case", _RS_AUTOGRAD, ids=[c[0] for c in _RS_AUTOGRAD])
def test_exact_bilinear_autograd(case):
    """One pass per route through BilinearFn: _pixels on channel slices, the separable() predicate, the re-pack of a
    16-bit gradient whose leading dimension is no multiple of 8."""
    hb = _hb()
    name, C, Hi, Wi, Ho, Wo, x16, out_f32, layout = case
    x, dy = RC.fwd_operand(case), RC.bwd_operand(case)
    ref, gref = exact_resize(name, x, Ho, Wo), exact_resize_grad(name, dy, Hi, Wi)
    out16 = x16 and not out_f32
    if layout == "dense":
        xd = x.to(_rs_dt(x16)).to(DEV).requires_grad_(True)
        dyd = dy.to(_rs_dt(out16)).to(DEV)
    else:
        xg = guarded_copy(x.to(_rs_dt(x16)), DEV, C + 8)
        dyg = guarded_copy(dy.to(_rs_dt(out16)), DEV, C + 4)
        xd, dyd = xg.view.detach().requires_grad_(True), dyg.view
    yd = hb.BilinearFn.apply(xd, Ho, Wo, out_f32)
    yd.backward(dyd)
    torch.cuda.synchronize()
    assert_bits_equal("BilinearFn %s forward" % name, yd.detach().cpu(), _rs_want(ref, out16))
    assert_bits_equal("BilinearFn %s backward" % name, xd.grad.cpu(), _rs_want(gref, x16))
    if layout != "dense":
        assert_guard_intact("BilinearFn %s" % name, xg, dyg)


def test_exact_bilinear_upsample_cat():
    """UpsampleCatGroupFn: an identity copy, a 2x and a 4x resize written into channel slices of one buffer (ldy = 80),
    and the backward reading its slices of the gradient in place (lddy = 80)."""
    hb = _hb()
    shapes = [(16, 12, 20), (48, 6, 10), (16, 3, 5)]
    Ho, Wo = 12, 20
    xs = [ints((RC.B, H, W, C), -200, 200, 420 + i) for i, (C, H, W) in enumerate(shapes)]
    dys = [ints((RC.B, Ho, Wo, C), -grad_amp(Ho, H, Wo, W, 200), grad_amp(Ho, H, Wo, W, 200), 430 + i)
           for i, (C, H, W) in enumerate(shapes)]
    want = torch.cat([to_act(exact_resize("cat %d" % i, x, Ho, Wo)) for i, x in enumerate(xs)], 3)
    gwant = [to_act(exact_resize_grad("cat %d" % i, dy, H, W)) for i, (dy, (C, H, W)) in enumerate(zip(dys, shapes))]
    assert not_representable(exact_resize_grad("cat 2", dys[2], 3, 5)) > 0
    xgs = [guarded_copy(x.to(ACT_DTYPE), DEV) for x in xs]
    leaves = [g.view.detach().requires_grad_(True) for g in xgs]
    dyg = guarded_copy(torch.cat(dys, 3).to(ACT_DTYPE), DEV)
    (y,) = hb.UpsampleCatGroupFn.apply((3,), *leaves)
    y.backward(dyg.view)
    torch.cuda.synchronize()
    assert_bits_equal("UpsampleCat forward", y.detach().cpu(), want)
    for i, leaf in enumerate(leaves):
        assert_bits_equal("UpsampleCat backward %d" % i, leaf.grad.cpu(), gwant[i])
    assert_guard_intact("UpsampleCat", dyg, *xgs)


# ---- 3b: bounded by route
def _rs_bounded(tag, got, ref, bound, idx, variants=None):
    """Every element within its bound.  Prints the worst error / bound with the index term's share of that bound, and the
    worst error in units of the bound WITHOUT the index term.  variants (fp32 outputs; a diagnosis, not asserted): the
    references whose source index is rounded once, as a contracted multiply-add would, on either axis, each with its own
    arithmetic term -- the last figure is then taken against the nearest of the four per element: near or below 1 says the index term is what a
    contraction needs, and which ones fit says whether the device contracts."""
    def over(e, b):                                         # e / b per element; a zero bound allows no error at all
        return torch.where(b > 0, e / b.clamp_min(1e-300), torch.where(e > 0, torch.full_like(e, float("inf")), torch.zeros_like(e)))
    err = (got.detach().double().cpu() - ref).abs()
    ratio = over(err, bound)
    k = int(ratio.flatten().argmax())
    share = float(idx.flatten()[k] / bound.flatten()[k]) if float(bound.flatten()[k]) > 0 else 0.0
    rest = bound - idx
    line = "[resize_bound] %-36s worst error / bound = %.3g (index term %.0f%% of that bound); error / (bound - index term) = %.3g" % (
        tag, float(ratio.flatten()[k]), 100 * share, float(over(err, rest).max()))
    if variants:
        each = [over((got.detach().double().cpu() - v).abs(), r) for v, r in [(ref, rest)] + variants]
        line += "; against the nearest of the single-rounding variants %.3g (each alone: %s)" % (
            float(torch.stack(each).min(0).values.max()), " ".join("%.3g" % float(e.max()) for e in each))
    print(line)
    assert_within_bound("resize_bound " + tag, got, ref, bound)           # NaN-safe: an unwritten output is a violation


_FMA_VARIANTS = ((True, False), (False, True), (True, True))


@pytest.mark.parametrize("case", RC.BOUNDED, ids=[c[0] for c in RC.BOUNDED])
def test_exact_bilinear_bounded(case):
    """Ratios that are not dyadic: every element of forward and backward within resize_bound of the float64 reference,
    dense and sliced; the 16-bit upsampling cases through the separable pair as well."""
    name, C, Hi, Wi, Ho, Wo, is16 = case
    x, dy = RC.bounded_operands(case)
    ref, _ = resize_ref64(x, Ho, Wo)
    gref, _ = resize_grad_ref64(dy, Hi, Wi)
    bf, idf = resize_bound(x, Ho, Wo, Hi, Wi, False, is16, ref)
    bb, idb = resize_bound(dy, Ho, Wo, Hi, Wi, True, is16, gref)
    def arith(v, backward, fma):
        b, i = resize_bound(v, Ho, Wo, Hi, Wi, backward, False, None, fma)
        return b - i
    vf = None if is16 else [(resize_ref64(x, Ho, Wo, v)[0], arith(x, False, v)) for v in _FMA_VARIANTS]
    vb = None if is16 else [(resize_grad_ref64(dy, Hi, Wi, v)[0], arith(dy, True, v)) for v in _FMA_VARIANTS]
    for pads in ((0, 0), (16, 8) if is16 else (5, 3)):
        tag = "%s %s" % (name, "dense" if pads == (0, 0) else "sliced")
        xg, yg = _rs_fwd(x, is16, is16, Ho, Wo, pads)
        dyg, dxg = _rs_bwd(dy, is16, is16, Hi, Wi, pads)
        torch.cuda.synchronize()
        _rs_bounded("fwd " + tag, yg.view, ref, bf, idf, vf)
        _rs_bounded("bwd " + tag, dxg.view, gref, bb, idb, vb)
        assert_guard_intact("bilinear bounded " + tag, xg, yg, dyg, dxg)
        if is16 and Ho >= 2 * Hi and Wo >= 2 * Wi:
            dyg, tg, dxg = _rs_bwd_sep(dy, True, True, Hi, Wi, pads)
            torch.cuda.synchronize()
            _rs_bounded("bwd separable " + tag, dxg.view, gref, bb, idb)
            assert_guard_intact("bilinear bounded separable " + tag, dyg, tg, dxg)


# ---- 3c: the grid-stride loops (GPU only)
def _dev_ints(shape, amp, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-amp, amp + 1, shape, generator=g, device=DEV, dtype=torch.int32)


def _dev_resize64(x, Ho, Wo):
    """torch's own float64 interpolate on the device, NHWC in and out (any correct float64 bilinear is THE reference at a
    dyadic ratio); with it the same of |x| for the premise."""
    F = torch.nn.functional
    xd = x.permute(0, 3, 1, 2).double()
    y = F.interpolate(xd, size=(Ho, Wo), mode="bilinear", align_corners=False)
    mag = float(F.interpolate(xd.abs(), size=(Ho, Wo), mode="bilinear", align_corners=False).max())
    return y.permute(0, 2, 3, 1).contiguous(), mag


def _dev_grad64(dy, Hi, Wi):
    """The float64 gradient of that interpolate (ATen's own backward), image by image to bound the memory."""
    Bn, Ho, Wo, C = dy.shape
    out, mag = [], 0.0
    for b in range(Bn):
        g = dy[b:b + 1].permute(0, 3, 1, 2).double().contiguous()
        out.append(torch.ops.aten.upsample_bilinear2d_backward(g, [Ho, Wo], [1, C, Hi, Wi], False, None, None).permute(0, 2, 3, 1))
        mag = max(mag, float(torch.ops.aten.upsample_bilinear2d_backward(g.abs(), [Ho, Wo], [1, C, Hi, Wi], False, None, None).max()))
        del g
    return torch.cat(out).contiguous(), mag


def _dev_want(tag, ref64, mag, is16, sizes):
    """The premise of the exact tests, asserted on the device reference; the reference in the output's format."""
    for n_out, n_in in sizes:
        assert is_dyadic(n_out, n_in), (tag, n_out, n_in)
    assert mag * 65536.0 < LIMIT, "%s: exactness premise violated: the magnitude product reaches %g" % (tag, mag)
    f = ref64.float()
    assert torch.equal(f.double(), ref64), "%s: the reference is not exact in fp32" % tag
    return f.to(ACT_DTYPE) if is16 else f


def _dev_bits_equal(tag, got, want):
    """Bitwise comparison where the tensors live; on a mismatch the first differing image row goes through
    assert_bits_equal for its report."""
    it = torch.int16 if got.element_size() == 2 else torch.int32
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = got.contiguous().view(it) != want.contiguous().view(it)
    n = int(bad.sum())
    if n:
        b, h = (int(v) for v in bad.nonzero()[0][:2])
        assert_bits_equal("%s: %d elements differ in all, first in image %d row %d" % (tag, n, b, h),
                          got[b, h].cpu(), want[b, h].cpu())


def _dev_operand(shape, amp, seed, is16, ld):
    """Integer operand generated on the device inside a guarded buffer; asserted representable."""
    v = _dev_ints(shape, amp, seed)
    g = guarded(shape, _rs_dt(is16), DEV, ld)
    g.view.copy_(v)
    assert torch.equal(g.view.to(torch.int32), v), "operand not representable"
    return g


_GS_KERNELS = ["fwd-v8", "fwd-px", "fwd-el", "bwd-v8-and-separable", "bwd-el", "bwd-tile"]


@pytest.mark.skipif(bool(os.environ.get("SSA_EMU")), reason="2 M threads and more: GPU only")
@pytest.mark.parametrize("kernel", _GS_KERNELS)
def test_exact_bilinear_grid_stride(kernel):
    """One exact 2x (0.5x) case per kernel just past its grid cap -- 8192 x 256 threads, 16384 tiles for the tiled
    backward -- at sizes that are no multiple of 256 or of the tile, so that the grid-stride loop turns and its last
    turn is ragged.  Reference and comparison on the device."""
    hb, L, check = _rs()
    Bn, C = RC.B, 8
    if kernel.startswith("fwd"):
        Hi = Wi = 515
        Ho = Wo = 1030
        in16, out16, pads = {"fwd-v8": (True, True, (8, 24)), "fwd-px": (False, False, (5, 0)), "fwd-el": (False, True, (5, 3))}[kernel]
        threads = Bn * Ho * Wo * (C if kernel == "fwd-el" else 1)
        assert threads > _GRID_CAP and threads % 256
        xg = _dev_operand((Bn, Hi, Wi, C), 200, 440, in16, C + pads[0])
        yg = guarded((Bn, Ho, Wo, C), _rs_dt(out16), DEV, C + pads[1])
        check(L.ssa_bilinear_fwd(hb._p(xg.view), 0 if in16 else 1, Bn, Hi, Wi, C, _ld4(xg), hb._p(yg.view), 0 if out16 else 1,
                                 Ho, Wo, _ld4(yg), hb._s()), "ssa_bilinear_fwd")
        ref, mag = _dev_resize64(xg.view, Ho, Wo)
        want = _dev_want(kernel, ref, mag, out16, [(Ho, Hi), (Wo, Wi)])
        if out16:
            assert int((want.double() != ref).sum()) > 0, "no output needs rounding"
        torch.cuda.synchronize()
        _dev_bits_equal("grid stride " + kernel, yg.view, want)
        assert_guard_intact("grid stride " + kernel, xg, yg)
        return
    if kernel == "bwd-v8-and-separable":
        Hi = Wi = 1030
        Ho = Wo = 2060
        assert Bn * Hi * Wi > _GRID_CAP and Bn * Ho * Wi > _GRID_CAP and (Bn * Hi * Wi) % 256        # pass Y / the gather; pass X
        dyg = _dev_operand((Bn, Ho, Wo, C), grad_amp(Ho, Hi, Wo, Wi), 441, True, C + 8)
        tg = guarded((Bn, Ho, Wi, C), torch.float32, DEV)
        dxg, dxg2 = (guarded((Bn, Hi, Wi, C), ACT_DTYPE, DEV, C + 8) for _ in range(2))
        check(L.ssa_bilinear_bwd_x(hb._p(dyg.view), 0, Bn, Ho, Wo, C, _ld4(dyg), hb._p(tg.view), Wi, hb._s()), "ssa_bilinear_bwd_x")
        check(L.ssa_bilinear_bwd_y(hb._p(tg.view), Bn, Ho, Wi, C, hb._p(dxg.view), 0, Hi, _ld4(dxg), hb._s()), "ssa_bilinear_bwd_y")
        check(L.ssa_bilinear_bwd(hb._p(dyg.view), 0, Bn, Ho, Wo, C, _ld4(dyg), hb._p(dxg2.view), 0, Hi, Wi, _ld4(dxg2), hb._s()),
              "ssa_bilinear_bwd")
        tref, tmag = _dev_grad64(dyg.view, Ho, Wi)                                                   # the X pass alone: a 1x resize in y
        twant = _dev_want(kernel + " pass X", tref, tmag, False, [(Wo, Wi)])
        del tref
        ref, mag = _dev_grad64(dyg.view, Hi, Wi)
        want = _dev_want(kernel, ref, mag, True, [(Ho, Hi), (Wo, Wi)])
        assert int((want.double() != ref).sum()) > 0, "no output needs rounding"
        torch.cuda.synchronize()
        _dev_bits_equal("grid stride bwd_x", tg.view, twant)
        _dev_bits_equal("grid stride bwd_y", dxg.view, want)
        _dev_bits_equal("grid stride vectorised gather", dxg2.view, want)
        assert_guard_intact("grid stride " + kernel, dyg, tg, dxg, dxg2)
        return
    if kernel == "bwd-el":                                   # 0.5x: a downsampling gradient never takes the tiled route
        Hi = Wi = 1030
        Ho = Wo = 515
        assert Bn * Hi * Wi * C > _GRID_CAP
    else:                                                    # 2 * 183 * 46 tiles of 4 x 16; 730 = 182 * 4 + 2 = 45 * 16 + 10
        Hi = Wi = 730
        Ho = Wo = 1460
        assert Bn * (-(-Hi // 4)) * (-(-Wi // 16)) > _TILE_CAP and Hi % 4 and Wi % 16
    dyg = _dev_operand((Bn, Ho, Wo, C), grad_amp(Ho, Hi, Wo, Wi, 200), 442, False, C + 5)
    dxg = guarded((Bn, Hi, Wi, C), torch.float32, DEV, C + 3)
    check(L.ssa_bilinear_bwd(hb._p(dyg.view), 1, Bn, Ho, Wo, C, _ld4(dyg), hb._p(dxg.view), 1, Hi, Wi, _ld4(dxg), hb._s()),
          "ssa_bilinear_bwd")
    ref, mag = _dev_grad64(dyg.view, Hi, Wi)
    want = _dev_want(kernel, ref, mag, False, [(Ho, Hi), (Wo, Wi)])
    torch.cuda.synchronize()
    _dev_bits_equal("grid stride " + kernel, dxg.view, want)
    assert_guard_intact("grid stride " + kernel, dyg, dxg)


# ---- 3d: the neighbours in the same family
def _image_resize(x, Ho, Wo, cpad=16):
    hb, L, check = _rs()
    Bn, C, Hi, Wi = x.shape
    xg = guarded_copy(x, DEV)
    yg = guarded((Bn, Ho, Wo, cpad), ACT_DTYPE, DEV)
    check(L.ssa_image_resize_to_nhwc_bf16(hb._p(xg.view), Bn, C, Hi, Wi, hb._p(yg.view), Ho, Wo, cpad, hb._s()),
          "ssa_image_resize_to_nhwc_bf16")
    return xg, yg


@pytest.mark.parametrize("Hi,Wi,Ho,Wo", [(12, 20, 6, 10), (9, 21, 9, 21), (9, 21, 18, 42), (9, 21, 36, 42)],
                         ids=["half", "copy", "2x", "4x-by-2x"])
def test_exact_image_resize(Hi, Wi, Ho, Wo):
    """ssa_image_resize_to_nhwc_bf16 of an integer image: the three channels bit for bit, the thirteen padding channels
    exactly zero, nothing written around the output.  The image is fp32, so its integers go to 250: halves and quarters
    of them need rounding in bf16 (in fp16 at 2x and 4x)."""
    x = ints((RC.B, 3, Hi, Wi), -250, 250, 450)
    ref = exact_resize("image", nhwc(x), Ho, Wo)
    want = torch.zeros((RC.B, Ho, Wo, 16), dtype=ACT_DTYPE)
    want[..., :3] = to_act(ref)
    xg, yg = _image_resize(x, Ho, Wo)
    torch.cuda.synchronize()
    assert_bits_equal("image_resize", yg.view.cpu(), want)
    assert_guard_intact("image_resize", xg, yg)
    through = _hb().image_to_nhwc(xg.view, None if (Hi, Wi) == (Ho, Wo) else (Ho, Wo))
    torch.cuda.synchronize()
    assert_bits_equal("image_to_nhwc", through.cpu(), want)


def test_exact_image_resize_bounded():
    """A size that is not dyadic: every element within resize_bound, the padding exactly zero."""
    Hi, Wi, Ho, Wo = 13, 17, 40, 27
    x = ints((RC.B, 3, Hi, Wi), -64, 64, 451)
    ref, _ = resize_ref64(nhwc(x), Ho, Wo)
    bound, idx = resize_bound(nhwc(x), Ho, Wo, Hi, Wi, False, True, ref)
    xg, yg = _image_resize(x, Ho, Wo)
    torch.cuda.synchronize()
    _rs_bounded("image_resize 13x17 -> 40x27", yg.view[..., :3], ref, bound, idx)
    assert_bits_equal("image_resize padding", yg.view[..., 3:].cpu(), torch.zeros((RC.B, Ho, Wo, 13), dtype=ACT_DTYPE))
    assert_guard_intact("image_resize bounded", xg, yg)


@pytest.mark.parametrize("Bn,C,H,W", [(1, 8, 5, 7), (1, 64, 33, 47), (2, 8, 5, 7)])
def test_exact_pool_max(Bn, C, H, W):
    """Max-pool 3x3 / 2 on post-ReLU integers (half of them zero, the rest in 1..3: ties in nearly every window): values and
    the gradient bit for bit against PyTorch's first-maximum rule in float64 -- an integer dy makes every dx a sum of at
    most four integers -- with the input a channel slice (ldx = C + 8)."""
    hb, L, check = _rs()
    F = torch.nn.functional
    x = torch.relu(ints((Bn, H, W, C), -3, 3, 460))
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    dy = ints((Bn, Ho, Wo, C), -16, 16, 461)
    assert_integers("maxpool", x, dy)
    xr = nchw(x).double().requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2, 1)
    yr.backward(nchw(dy).double())
    assert float((x == 0).float().mean()) > 0.4
    xg = guarded_copy(x.to(ACT_DTYPE), DEV, C + 8)
    yg = guarded((Bn, Ho, Wo, C), ACT_DTYPE, DEV)
    ig = guarded((Bn, Ho, Wo, C), torch.uint8, DEV)
    dyg = guarded_copy(dy.to(ACT_DTYPE), DEV)
    dxg = guarded((Bn, H, W, C), ACT_DTYPE, DEV)
    check(L.ssa_maxpool3x3s2_fwd(hb._p(xg.view), _ld4(xg), Bn, H, W, C, hb._p(yg.view), hb._p(ig.view), Ho, Wo, hb._s()),
          "ssa_maxpool3x3s2_fwd")
    check(L.ssa_maxpool3x3s2_bwd(hb._p(dyg.view), hb._p(ig.view), Bn, Ho, Wo, C, hb._p(dxg.view), H, W, hb._s()),
          "ssa_maxpool3x3s2_bwd")
    torch.cuda.synchronize()
    assert_bits_equal("maxpool y", yg.view.cpu(), to_act(nhwc(yr.detach())))
    assert int(ig.view.max()) <= 8
    assert_bits_equal("maxpool dx", dxg.view.cpu(), to_act(nhwc(xr.grad)))
    assert_guard_intact("maxpool", xg, yg, ig, dyg, dxg)
    # the same through autograd
    xd = xg.view.detach().requires_grad_(True)
    yd = hb.MaxPool3x3s2Fn.apply(xd)
    yd.backward(dyg.view)
    torch.cuda.synchronize()
    assert_bits_equal("MaxPool3x3s2Fn dx", xd.grad.cpu(), to_act(nhwc(xr.grad)))


def _gap(x, dout, pads):
    hb, L, check = _rs()
    Bn, H, W, C = x.shape
    xg = guarded_copy(x.to(ACT_DTYPE), DEV, C + pads)
    og = guarded((Bn, C), ACT_DTYPE, DEV)
    dg = guarded_copy(dout.to(ACT_DTYPE), DEV)
    dxg = guarded((Bn, H, W, C), ACT_DTYPE, DEV)
    check(L.ssa_global_avg_pool_fwd(hb._p(xg.view), _ld4(xg), Bn, H * W, C, hb._p(og.view), hb._s()), "ssa_global_avg_pool_fwd")
    check(L.ssa_global_avg_pool_bwd(hb._p(dg.view), Bn, H * W, C, hb._p(dxg.view), hb._s()), "ssa_global_avg_pool_bwd")
    torch.cuda.synchronize()
    return xg, og, dg, dxg


@pytest.mark.parametrize("H,W", [(8, 16), (32, 64)], ids=["hw128", "hw2048"])
def test_exact_pool_gap(H, W):
    """Global average pool with HW a power of two: the fp32 sum of integers is exact (sum |x| < 2^24) and so is the
    division, the mean is rounded once; the backward dout / HW is exact.  HW = 2048: a thread sums eight pixels.  The
    input is a channel slice (ldx = C + 8)."""
    Bn, C = RC.B, 24
    x, dout = ints((Bn, H, W, C), -200, 200, 470), ints((Bn, C), -200, 200, 471)
    assert_integers("gap", x, dout)
    assert_premise("gap", x.double().abs().sum((1, 2)))
    ref = x.double().mean((1, 2))
    gref = (dout.double() / (H * W))[:, None, None, :].expand(Bn, H, W, C)
    assert not_representable(ref) > 0
    xg, og, dg, dxg = _gap(x, dout, 8)
    assert_bits_equal("gap fwd", og.view.cpu(), to_act(ref))
    assert_bits_equal("gap bwd", dxg.view.cpu(), to_act(gref.contiguous()))
    assert_guard_intact("gap", xg, og, dg, dxg)


def test_exact_pool_gap_bounded():
    """HW = 12 * 16, no power of two: against float64 within (HW + 2) 2^-24 mean|x| -- HW - 1 additions in any order, the
    division -- plus the rounding of the output; the backward within 2 * 2^-24 |dout| / HW (the reciprocal, the
    product) plus the same."""
    Bn, C, H, W = RC.B, 24, 12, 16
    hw = H * W
    x, dout = ints((Bn, H, W, C), -64, 64, 472), ints((Bn, C), -64, 64, 473)
    ref = x.double().mean((1, 2))
    gref = (dout.double() / hw)[:, None, None, :].expand(Bn, H, W, C).contiguous()
    xg, og, dg, dxg = _gap(x, dout, 8)
    b = (hw + 2) * 2.0 ** -24 * x.double().abs().mean((1, 2))
    b = b + half_ulp_act(ref.abs() + b)
    gb = 2 * 2.0 ** -24 * gref.abs()
    gb = gb + half_ulp_act(gref.abs() + gb)
    zero = torch.zeros(())
    _rs_bounded("gap fwd HW=192", og.view, ref, b, zero.expand_as(b))
    _rs_bounded("gap bwd HW=192", dxg.view, gref, gb, zero.expand_as(gb))
    assert_guard_intact("gap bounded", xg, og, dg, dxg)
