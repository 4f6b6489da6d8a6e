"""Dry run of the HIP host glue (tests/test_hip_glue_dryrun_cpu.py's machinery: the real library's host entry points,
signature-checked stand-ins for every launch, CPU tensors) for the Dense Prediction Cell: forward and backward of the
cell alone, the argument patterns of the rectangular-dilation entry points, the placement of the five layers in ONE
concatenated buffer, the group brackets, the launch budget, and a train step / eval pass of DeepV3Plus(use_dpc=True).

Placement, as built: a layer is conv -> BatchNorm -> ReLU.  The conv's raw output is a tensor of its own (the BatchNorm
backward reads it), the LAYER's output -- what the BatchNorm pass stores -- is the layer's 64-channel slice of the
[B,H,W,5 x 64] buffer (pixel stride 5 Cout), and b, c, d, e read their input out of that buffer (ldx = 5 Cout)."""
import collections

import pytest
import torch

from test_hip_glue_dryrun_cpu import dry, _batch  # noqa: F401  (dry: the fixture)
from test_x71_glue_dryrun_cpu import _spy, _ptr

NAMES = ("ssa_group_begin", "ssa_group_end", "ssa_dilconv3x3", "ssa_dilconv3x3_wgrad", "ssa_bn_apply_train", "ssa_bn_stats",
         "ssa_bn_bwd_reduce", "ssa_bn_bwd_apply", "ssa_pack_filter", "ssa_conv2d_igemm", "ssa_conv2d_igemm_stats")
CIN, C, H, W, B = 256, 64, 48, 52, 2
RATES8 = [(2, 12), (36, 30), (12, 42), (2, 2), (12, 6)]


def _brackets(log):
    """The launching calls of a log, grouped by the (outermost) group bracket they were issued in: [[(name, args)]];
    a call outside any bracket is a bracket of its own."""
    out, depth, cur = [], 0, None
    for n, a in log:
        if n == "ssa_group_begin":
            if depth == 0:
                cur = []
            depth += 1
        elif n == "ssa_group_end":
            depth -= 1
            if depth == 0:
                if cur:
                    out.append(cur)
                cur = None
        elif depth:
            cur.append((n, a))
        else:
            out.append([(n, a)])
    assert depth == 0
    return out


def _dil(a):
    d = a[0]._obj
    return (d.dil_h, d.dil_w)


def test_dpc_cell_forward_and_backward_glue(dry, monkeypatch):
    from semseg_amd import hip_backend as hb, ops
    from semseg_amd.network.deepv3 import DPC
    log = []
    _spy(monkeypatch, type(dry), NAMES, log)
    cell = DPC(CIN, C, output_stride=8).train()
    x = torch.zeros(B, H, W, CIN, dtype=hb.ACT_DTYPE).requires_grad_(True)
    bk = ops.backend()
    bk.begin_step(x.device)
    out = cell(x)
    bk.end_forward()
    assert tuple(out.shape) == (B, H, W, 5 * C) and out.is_contiguous() and out.requires_grad
    nrep = hb.stat_replicas()
    br = [[c for c in b if c[0] != "ssa_pack_filter"] for b in _brackets(log)]
    br = [b for b in br if b]
    kinds = [[n for n, _ in b] for b in br]
    # the launch budget of the forward: three conv launches (a | b, c, d | e) and three BatchNorm launches
    assert kinds == [["ssa_dilconv3x3"], ["ssa_bn_apply_train"], ["ssa_dilconv3x3"] * 3, ["ssa_bn_apply_train"] * 3,
                     ["ssa_dilconv3x3"], ["ssa_bn_apply_train"]], kinds
    assert sum(1 for n, _ in log if n == "ssa_pack_filter") == 5          # (first step only: the pack cache keeps them)
    convs = [a for n, a in log if n == "ssa_dilconv3x3"]
    bns = [a for n, a in log if n == "ssa_bn_apply_train"]
    assert [_dil(a) for a in convs] == RATES8
    # x, ldx, residual, ldr, z, ldz, P, C, sums, nrep: every layer's output is its slice of ONE buffer of pixel stride 5 C
    z = [_ptr(a[4]) for a in bns]
    esz = out.element_size()
    assert z[0] == out.data_ptr() and [p - z[0] for p in z] == [i * C * esz for i in range(5)]
    assert all(a[5] == 5 * C and a[6] == B * H * W and a[7] == C and a[2] is None for a in bns)
    for i, (cv, bn) in enumerate(zip(convs, bns)):
        d = cv[0]._obj
        assert (d.B, d.H, d.W, d.Cout, d.ldy) == (B, H, W, C, C)
        assert _ptr(cv[3]) == _ptr(bn[0]) and bn[1] == C, "the BatchNorm does not read the conv's output"
        assert _ptr(cv[4]) and _ptr(cv[4]) == _ptr(bn[8]) and bn[9] == nrep, "the statistics do not ride on the conv epilogue"
        if i == 0:
            assert (d.Cin, d.ldx) == (CIN, CIN) and _ptr(cv[1]) == x.data_ptr()
        else:
            src = z[0] if i < 4 else z[1]                          # b, c, d read a; e reads b -- out of the buffer
            assert (d.Cin, d.ldx) == (C, 5 * C) and _ptr(cv[1]) == src
    assert not [1 for n, _ in log if n in ("ssa_bn_stats", "ssa_conv2d_igemm", "ssa_conv2d_igemm_stats")]

    del log[:]
    before = dict(dry.calls)
    out.float().sum().backward()
    assert x.grad is not None and tuple(x.grad.shape) == tuple(x.shape)
    for n, p in cell.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == torch.float32, n
    br = [[c for c in b if c[0] != "ssa_pack_filter"] for b in _brackets(log)]
    conv_br = [b for b in br if b and b[0][0] == "ssa_dilconv3x3"]
    # data gradients: e | b, c, d in one bracket | a; all on the mode-3 filter, no statistics
    assert [len(b) for b in conv_br] == [1, 3, 1]
    assert [_dil(a) for b in conv_br for _, a in b] == [RATES8[4], RATES8[1], RATES8[2], RATES8[3], RATES8[0]]
    for b in conv_br:
        for _, a in b:
            d = a[0]._obj
            assert _ptr(a[4]) is None and d.Cin == C and d.ldx >= C and d.ldy == d.Cout
    assert conv_br[2][0][1][0]._obj.Cout == CIN
    assert sum(1 for n, _ in log if n == "ssa_pack_filter") == 5          # the five mode-3 operands
    wg = [a for n, a in log if n == "ssa_dilconv3x3_wgrad"]
    # d, x, dy, lddy, dw, accumulate, ws: added into the gradient arena; b, c, d, e read x out of the concat buffer
    assert sorted(_dil(a) for a in wg) == sorted(RATES8)
    for a in wg:
        d = a[0]._obj
        assert all(_ptr(a[i]) for i in (1, 2, 4, 6)) and a[3] >= C and a[5] == 1
        assert (d.Cin, d.ldx) == ((CIN, CIN) if _dil(a) == RATES8[0] else (C, 5 * C))
    # the launch budget of the backward: 3 data-gradient launches, 5 weight gradients of 2 launches each, and per
    # BatchNorm group (e | b, c, d | a) one reduce and one apply launch
    red = [b for b in br if b and b[0][0] == "ssa_bn_bwd_reduce"]
    app = [b for b in br if b and b[0][0] == "ssa_bn_bwd_apply"]
    assert [len(b) for b in red] == [1, 3, 1] and [len(b) for b in app] == [1, 3, 1]
    delta = {k: v - before.get(k, 0) for k, v in dry.calls.items() if v != before.get(k, 0)}
    assert {k: v for k, v in delta.items() if k.startswith("ssa_dilconv")} == {"ssa_dilconv3x3": 5, "ssa_dilconv3x3_wgrad": 5}
    assert not [k for k in delta if k.startswith("ssa_conv2d")], delta


def test_dpc_eval_glue(dry, monkeypatch):
    from semseg_amd import hip_backend as hb, ops
    from semseg_amd.network.deepv3 import DPC
    log = []
    _spy(monkeypatch, type(dry), NAMES + ("ssa_bn_apply",), log)
    cell = DPC(CIN, C, output_stride=16).eval()
    x = torch.zeros(1, 24, 28, CIN, dtype=hb.ACT_DTYPE)
    ops.backend().begin_step(x.device)
    with torch.no_grad():
        out = cell(x)
    assert tuple(out.shape) == (1, 24, 28, 5 * C)
    convs = [a for n, a in log if n == "ssa_dilconv3x3"]
    assert [_dil(a) for a in convs] == [(1, 6), (18, 15), (6, 21), (1, 1), (6, 3)]
    assert all(_ptr(a[4]) is None for a in convs), "an evaluation conv took statistics"
    assert len([1 for n, _ in log if n == "ssa_bn_apply"]) == 5 and not [1 for n, _ in log if n == "ssa_bn_apply_train"]


def test_unsupported_shape_raises(dry):
    """A channel count the kernels are not built for surfaces as a Python exception before anything is launched:
    there is no other route for a rectangular dilation."""
    from semseg_amd import hip_backend as hb, nn as snn, ops
    bk = ops.backend()
    bk.begin_step(torch.device("cpu"))
    for cin, cout in ((48, 64), (64, 40)):
        conv, bn = snn.DilConv2d(cin, cout, kernel_size=3, padding=(2, 3), dilation=(2, 3), bias=False), snn.BatchNorm2d(cout)
        before = sum(dry.calls.values())
        with pytest.raises(NotImplementedError, match="multiples of 64"):
            conv(torch.zeros(1, 8, 8, cin, dtype=hb.ACT_DTYPE), bn)
        assert sum(dry.calls.values()) == before
    conv, bn = snn.DilConv2d(64, 64, kernel_size=3, padding=(2, 3), dilation=(2, 3), bias=False), snn.BatchNorm2d(64)
    with pytest.raises(NotImplementedError, match="NHWC"):
        conv(torch.zeros(1, 8, 8, 64, dtype=torch.float32), bn)
    # the library's own answer, through check(): the codes become exceptions
    from semseg_amd._lib import DilConvDesc, check
    import ctypes
    L = hb.lib()
    bad = DilConvDesc(1, 8, 8, 48, 48, 64, 64, 2, 3)
    assert L.ssa_dilconv3x3_supported(ctypes.byref(bad)) == 0
    nb = ctypes.c_size_t(0)
    with pytest.raises(RuntimeError, match="unsupported configuration"):
        check(L.ssa_dilconv3x3_wgrad_plan(ctypes.byref(bad), None, ctypes.byref(nb)), "ssa_dilconv3x3_wgrad_plan")


def test_deepv3_dpc_train_step_and_eval_glue(dry, monkeypatch):
    from semseg_amd.loss import CrossEntropyLoss2d
    from semseg_amd.network.deepv3 import DeepV3Plus
    log = []
    _spy(monkeypatch, type(dry), ("ssa_dilconv3x3", "ssa_dilconv3x3_wgrad"), log)
    net = DeepV3Plus(19, trunk="resnet-50", criterion=CrossEntropyLoss2d(ignore_index=255), use_dpc=True).train()
    inputs = _batch()                                       # 2 x 64 x 96: 8 x 12 at stride 8
    loss = net(inputs)
    assert loss.dim() == 0 and loss.requires_grad
    fwd = [a for n, a in log if n == "ssa_dilconv3x3"]
    assert [_dil(a) for a in fwd] == RATES8 and fwd[0][0]._obj.Cin == 2048
    assert collections.Counter((a[0]._obj.H, a[0]._obj.W) for a in fwd) == {(8, 12): 5}
    del log[:]
    loss.backward()
    missing = [n for n, p in net.named_parameters() if p.grad is None]
    assert not missing, missing[:5]
    assert len([1 for n, _ in log if n == "ssa_dilconv3x3"]) == 5 and len([1 for n, _ in log if n == "ssa_dilconv3x3_wgrad"]) == 5
    net.eval()
    with torch.no_grad():
        out = net({"images": inputs["images"]})
    assert tuple(out["pred"].shape) == (2, 19, 64, 96) and out["pred"].dtype == torch.float32
