"""Dry run of the HIP host glue (tests/test_hip_glue_dryrun_cpu.py's machinery: the real library's host entry points,
signature-checked stand-ins for every launch, CPU tensors) for deepv3.DeepV3PlusSRNX50: a train step and an eval pass, and
the argument patterns of the grouped conv, SE gate and ceil pool entry points."""
import collections

import torch

from test_hip_glue_dryrun_cpu import dry, _batch  # noqa: F401  (dry: the fixture)
from test_x71_glue_dryrun_cpu import _spy, _ptr

# (C, stride, dil) of the 16 grouped convs: layer1 3, layer2 1 + 3, layer3 6, layer4 3.  HipBackend.GCONV_ROUTE keeps layer1's
# (128, 1, 1) on the block-diagonal dense filter (where the grouped kernels measured slower): 13 reach ssa_gconv3x3
ALL_GC = collections.Counter({(128, 1, 1): 3, (256, 2, 1): 1, (256, 1, 1): 3, (512, 1, 2): 6, (1024, 1, 4): 3})
GC_MULTISET = collections.Counter({(256, 2, 1): 1, (256, 1, 1): 3, (512, 1, 2): 6, (1024, 1, 4): 3})
SE_MULTISET = collections.Counter({256: 3, 512: 4, 1024: 6, 2048: 3})


def _geom(a):
    d = a[0]._obj
    return d.C, d.stride, d.dil


def test_srnx_train_step_and_eval_glue(dry, monkeypatch):
    from semseg_amd import hip_backend as hb
    from semseg_amd.loss import CrossEntropyLoss2d
    from semseg_amd.network import get_model
    from semseg_amd import ops
    assert {k for k, v in ops.HipBackend.GCONV_ROUTE.items() if not v} == set(ALL_GC) - set(GC_MULTISET)
    log = []
    names = ("ssa_gconv3x3", "ssa_gconv3x3_bwd", "ssa_se_squeeze_gate", "ssa_se_apply", "ssa_se_bwd_reduce", "ssa_se_gate_bwd",
             "ssa_se_apply_bwd", "ssa_maxpool3x3s2c_fwd", "ssa_maxpool3x3s2c_bwd", "ssa_maxpool3x3s2_fwd", "ssa_bn_stats",
             "ssa_bn_apply_train")
    _spy(monkeypatch, type(dry), names, log)
    net = get_model("deepv3.DeepV3PlusSRNX50", 19, CrossEntropyLoss2d(ignore_index=255)).train()
    inputs = _batch()                                       # 2 x 64 x 96
    loss = net(inputs)
    assert loss.dim() == 0 and loss.requires_grad
    by = collections.defaultdict(list)
    for n, a in log:
        by[n].append(a)
    assert not by["ssa_maxpool3x3s2_fwd"] and len(by["ssa_maxpool3x3s2c_fwd"]) == 1
    pool = by["ssa_maxpool3x3s2c_fwd"][0]                   # x, ldx, B, H, W, C, y, idx, Ho, Wo: 32 x 48 -> 16 x 24
    assert pool[2:6] == (2, 32, 48, 64) and pool[8:10] == (16, 24)
    fwd = by["ssa_gconv3x3"]
    assert len(fwd) == 13 and collections.Counter(_geom(a) for a in fwd) == GC_MULTISET
    nrep = hb.stat_replicas()
    train_sums = {_ptr(a[8]) for a in by["ssa_bn_apply_train"] if a[9] == nrep}
    gc_out = set()
    for a in fwd:
        d = a[0]._obj
        assert d.G == 32 and (d.Ho, d.Wo) == ((d.H - 1) // d.stride + 1, (d.W - 1) // d.stride + 1) and d.ldx >= d.C and d.ldy == d.C
        assert _ptr(a[1]) and _ptr(a[2]) and _ptr(a[3])
        assert _ptr(a[4]), "a training grouped conv without the statistics epilogue"
        assert _ptr(a[4]) in train_sums, "the grouped conv's sums did not reach ssa_bn_apply_train with the replica count"
        gc_out.add(_ptr(a[3]))
    assert not gc_out & {_ptr(a[0]) for a in by["ssa_bn_stats"]}, "bn2 took its statistics in a pass of its own"
    sq, ap = by["ssa_se_squeeze_gate"], by["ssa_se_apply"]
    assert len(sq) == len(ap) == 16 and collections.Counter(a[4] for a in sq) == SE_MULTISET
    for a, b in zip(sq, ap):
        # y, ldy, B, HW, C, Cr, w1, b1, w2, b2, mean, h, s, ws | y, ldy, r, ldr, s, z, ldz, B, HW, C, relu
        assert a[2] == 2 and a[5] * 16 == a[4] and all(_ptr(v) for v in a[6:14])
        assert _ptr(b[0]) == _ptr(a[0]) and _ptr(b[2]) and _ptr(b[4]) == _ptr(a[12]) and b[7:11] == (2, a[3], a[4], 1)
    # the dense filters of layer1's three convs are temporaries: none of them may sit in the packed-filter cache, whose
    # device job tables a new entry resets (the next step's begin_step would rebuild them inside a stream capture)
    cached = [e.wref() for e in hb._PACKED.values()]
    assert cached and all(isinstance(w, torch.nn.Parameter) for w in cached if w is not None)
    del log[:]
    loss.backward()
    assert all(isinstance(e.wref(), torch.nn.Parameter) for e in hb._PACKED.values() if e.wref() is not None)
    missing = [n for n, p in net.named_parameters() if p.grad is None]
    assert not missing, missing[:5]
    for n, p in net.named_parameters():
        assert p.grad.shape == p.shape and p.grad.dtype == torch.float32, n
    by = collections.defaultdict(list)
    for n, a in log:
        by[n].append(a)
    bwd = by["ssa_gconv3x3_bwd"]
    assert len(bwd) == 13 and collections.Counter(_geom(a) for a in bwd) == GC_MULTISET
    for a in bwd:
        d = a[0]._obj
        # x, dy, lddy, w, dx, lddx, dw, accumulate, ws: both gradients, dw added into the gradient arena
        assert _ptr(a[1]) and _ptr(a[2]) and a[3] >= d.C and _ptr(a[4]) and _ptr(a[5]) and a[6] == d.C
        assert _ptr(a[7]) and a[8] == 1 and _ptr(a[9])
    assert len(by["ssa_se_bwd_reduce"]) == len(by["ssa_se_gate_bwd"]) == len(by["ssa_se_apply_bwd"]) == 16
    for a in by["ssa_se_gate_bwd"]:
        assert all(_ptr(v) for v in a[:6]) and all(_ptr(v) for v in a[10:15]) and a[15] == 1 and _ptr(a[16])
    for a in by["ssa_se_apply_bwd"]:
        assert _ptr(a[10]) and _ptr(a[12]), "dy and dresidual both come out of the one pass"
    assert len(by["ssa_maxpool3x3s2c_bwd"]) == 1
    net.eval()
    del log[:]
    with torch.no_grad():
        out = net({"images": inputs["images"]})
    assert tuple(out["pred"].shape) == (2, 19, 64, 96) and out["pred"].dtype == torch.float32
    ev = [a for n, a in log if n == "ssa_gconv3x3"]
    assert len(ev) == 13 and all(_ptr(a[4]) is None for a in ev)
    assert len([1 for n, a in log if n == "ssa_se_apply"]) == 16
    assert not [1 for n, a in log if n in ("ssa_bn_stats", "ssa_bn_apply_train", "ssa_se_bwd_reduce")]
