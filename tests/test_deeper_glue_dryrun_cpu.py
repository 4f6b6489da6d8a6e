"""Dry run of the HIP host glue (tests/test_hip_glue_dryrun_cpu.py's machinery: the real library's host entry points,
signature-checked stand-ins for every launch, CPU tensors) for deeper.DeeperX71 and mscale.DeeperW38: a train step and
an eval pass, and the route of the two 5x5 convs (conv_up2 320->256 at stride 4, conv_up3 288->256 at stride 2) and of
their data gradients -- ssa_conv2d_halo5 where the library's size policy (ssa_conv2d_halo5_supported: W >= 32 and
>= 16384 pixels) takes the problem, the implicit GEMM below it.  The weight gradients stay on ssa_conv2d_wgrad."""
import ctypes

import pytest
import torch

from test_hip_glue_dryrun_cpu import DryLib, dry, _batch  # noqa: F401  (dry: the fixture)
from test_x71_glue_dryrun_cpu import _spy

CONV_ENTRIES = ("ssa_conv2d_halo5", "ssa_conv2d_igemm_stats", "ssa_conv2d_igemm_affine", "ssa_conv2d_halo", "ssa_conv2d_tile",
                "ssa_conv2d_tile_p", "ssa_conv2d_tile_aux", "ssa_conv2d_gemm_wide", "ssa_conv2d_wgrad", "ssa_conv2d_wgrad_head",
                "ssa_conv2d_wgrad_tile")


def _five(log):
    """(entry point, Cin, Cout, H, W) of every logged conv launch with a 5x5 filter, in issue order."""
    out = []
    for name, a in log:
        d = a[0]._obj
        if d.KH == 5 and d.KW == 5:
            assert (d.stride, d.pad, d.dil, d.transposed) == (1, 2, 1, 0) and (d.Ho, d.Wo) == (d.H, d.W)
            out.append((name, d.Cin, d.Cout, d.H, d.W))
    return out


def _net(arch):
    from semseg_amd.loss import CrossEntropyLoss2d
    from semseg_amd.network import get_model
    return get_model(arch, 19, CrossEntropyLoss2d(ignore_index=255))


def test_size_policy_of_the_library():
    """ssa_conv2d_halo5_supported: the policy threshold and what the kernel takes at all."""
    from semseg_amd import _lib
    from semseg_amd._lib import ConvDesc
    L = _lib.lib()

    def sup(B=1, H=128, W=128, Cin=320, Cout=256, k=5, stride=1, pad=2, dil=1, ldx=None, out_f32=0):
        d = ConvDesc(B, H, W, Cin, ldx or Cin, H, W, Cout, Cout, k, k, stride, pad, dil, 0, 0, out_f32, -1)
        return L.ssa_conv2d_halo5_supported(ctypes.byref(d))
    assert sup() == 1 and sup(Cin=288) == 1 and sup(Cin=256, Cout=320) == 1 and sup(Cin=256, Cout=288) == 1
    assert sup(H=127) == 0 and sup(B=2, H=64) == 1              # 16384 pixels
    assert sup(H=1024, W=31) == 0 and sup(H=512, W=32) == 1     # W >= 32
    assert sup(Cin=72) == 0 and sup(k=3, pad=1) == 0 and sup(pad=1) == 0 and sup(dil=2) == 0 and sup(stride=2) == 0
    assert sup(out_f32=1) == 0 and sup(ldx=324) == 0 and sup(ldx=328) == 1
    # nothing that ran before changes route: the 3x3 / 1x1 policies do not know the 5x5 filter
    d = ConvDesc(1, 128, 128, 320, 320, 128, 128, 256, 256, 5, 5, 1, 2, 1, 0, 0, 0, -1)
    assert L.ssa_conv2d_halo_supported(ctypes.byref(d)) == 0 and L.ssa_conv2d_tile_supported(ctypes.byref(d)) == 0
    assert L.ssa_conv2d_gemm_wide_supported(ctypes.byref(d)) == 0


def test_deeper_x71_glue(dry, monkeypatch):
    """deeper.DeeperX71.  1 x 512 x 512: conv_up2 at 128 x 128 (exactly 16384 pixels) and conv_up3 at 256 x 256, forward
    and data gradient on ssa_conv2d_halo5.  2 x 64 x 96 (16 x 24 and 32 x 48): all four on the implicit GEMM."""
    log = []
    _spy(monkeypatch, type(dry), CONV_ENTRIES, log)
    net = _net("deeper.DeeperX71").train()
    big = _batch(1, 512, 512)
    loss = net(big)
    assert loss.dim() == 0 and loss.requires_grad
    assert _five(log) == [("ssa_conv2d_halo5", 320, 256, 128, 128), ("ssa_conv2d_halo5", 288, 256, 256, 256)]
    for name, a in log:
        if name == "ssa_conv2d_halo5":          # training: the BatchNorm sums come out of the conv's epilogue
            assert a[5] is not None and a[3] is None
    del log[:]
    loss.backward()
    missing = [n for n, p in net.named_parameters() if p.grad is None]
    assert not missing, missing[:5]
    for n, p in net.named_parameters():
        assert p.grad.shape == p.shape and p.grad.dtype == torch.float32, n
    five = _five(log)
    assert [f for f in five if f[0] == "ssa_conv2d_halo5"] == [("ssa_conv2d_halo5", 256, 288, 256, 256),
                                                              ("ssa_conv2d_halo5", 256, 320, 128, 128)]
    # the 5x5 weight gradients: the generic kernel, with the forward geometry
    assert sorted(f for f in five if f[0] != "ssa_conv2d_halo5") == [("ssa_conv2d_wgrad", 288, 256, 256, 256),
                                                                    ("ssa_conv2d_wgrad", 320, 256, 128, 128)]
    assert dry.calls["ssa_bn_update_running_batched"] == 1
    net.eval()
    del log[:]
    with torch.no_grad():
        out = net({"images": big["images"]})
    assert tuple(out["pred"].shape) == (1, 19, 512, 512) and out["pred"].dtype == torch.float32
    assert _five(log) == [("ssa_conv2d_halo5", 320, 256, 128, 128), ("ssa_conv2d_halo5", 288, 256, 256, 256)]
    assert all(a[5] is None for name, a in log if name == "ssa_conv2d_halo5")      # no statistics in evaluation

    net.train()
    del log[:]
    small = _batch()
    loss = net(small)
    assert _five(log) == [("ssa_conv2d_igemm_stats", 320, 256, 16, 24), ("ssa_conv2d_igemm_stats", 288, 256, 32, 48)]
    del log[:]
    loss.backward()
    assert sorted(_five(log)) == [("ssa_conv2d_igemm_stats", 256, 288, 32, 48), ("ssa_conv2d_igemm_stats", 256, 320, 16, 24),
                                  ("ssa_conv2d_wgrad", 288, 256, 32, 48), ("ssa_conv2d_wgrad", 320, 256, 16, 24)]
    net.eval()
    with torch.no_grad():
        out = net({"images": small["images"]})
    assert tuple(out["pred"].shape) == (2, 19, 64, 96) and out["pred"].dtype == torch.float32


def test_mscale_deeper_w38_glue(dry, monkeypatch):
    """mscale.DeeperW38 at 1 x 512 x 512 under the two-scale training forward: the 1.0x pass has conv_up2 at 128 x 128 and
    conv_up3 at 256 x 256 (ssa_conv2d_halo5), the 0.5x pass has them at 64 x 64 and 128 x 128 -- conv_up2 below the
    threshold (implicit GEMM), conv_up3 at it (ssa_conv2d_halo5).  Then the two-scale and the N-scale evaluation."""
    from semseg_amd.config import cfg
    monkeypatch.setattr(cfg.LOSS, "SUPERVISED_MSCALE_WT", 0.05)
    log = []
    _spy(monkeypatch, type(dry), CONV_ENTRIES, log)
    net = _net("mscale.DeeperW38").train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    big = _batch(1, 512, 512)
    loss = net(big)
    assert loss.dim() == 0 and loss.requires_grad
    want_fwd = [("ssa_conv2d_halo5", 288, 256, 128, 128), ("ssa_conv2d_halo5", 288, 256, 256, 256),
                ("ssa_conv2d_halo5", 320, 256, 128, 128), ("ssa_conv2d_igemm_stats", 320, 256, 64, 64)]
    assert sorted(_five(log)) == want_fwd
    del log[:]
    loss.backward()
    missing = [n for n, p in net.named_parameters() if p.grad is None]
    assert not missing, missing[:5]
    five = _five(log)
    assert sorted(f for f in five if "wgrad" not in f[0]) == [
        ("ssa_conv2d_halo5", 256, 288, 128, 128), ("ssa_conv2d_halo5", 256, 288, 256, 256),
        ("ssa_conv2d_halo5", 256, 320, 128, 128), ("ssa_conv2d_igemm_stats", 256, 320, 64, 64)]
    assert sorted(f for f in five if "wgrad" in f[0]) == [
        ("ssa_conv2d_wgrad", 288, 256, 128, 128), ("ssa_conv2d_wgrad", 288, 256, 256, 256),
        ("ssa_conv2d_wgrad", 320, 256, 64, 64), ("ssa_conv2d_wgrad", 320, 256, 128, 128)]
    assert dry.calls["ssa_bn_update_running_batched"] == 1
    net.eval()
    del log[:]
    with torch.no_grad():
        out = net({"images": big["images"]})
    assert sorted(out) == ["attn_05x", "pred", "pred_05x", "pred_10x"]
    assert tuple(out["pred"].shape) == (1, 19, 512, 512) and out["pred"].dtype == torch.float32
    assert tuple(out["attn_05x"].shape) == (1, 1, 256, 256)
    # (below the threshold the implicit GEMM carries the evaluation BatchNorm as its epilogue; behind ssa_conv2d_halo5 the
    # BatchNorm apply is a launch of its own)
    assert sorted(_five(log)) == want_fwd[:3] + [("ssa_conv2d_igemm_affine", 320, 256, 64, 64)]
    assert all(a[5] is None for name, a in log if name == "ssa_conv2d_halo5")
    monkeypatch.setattr(cfg.MODEL, "N_SCALES", [0.5, 1.0, 2.0])
    small = _batch()
    with torch.no_grad():
        out = net({"images": small["images"]})
    assert tuple(out["pred"].shape) == (2, 19, 64, 96)
