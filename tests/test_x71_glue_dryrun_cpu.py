"""Dry run of the HIP host glue (tests/test_hip_glue_dryrun_cpu.py's machinery: the real library's host entry points,
signature-checked stand-ins for every launch, CPU tensors) for deepv3.DeepV3PlusX71: a train step and an eval pass, the
argument patterns of the depthwise entry points, and the two-rank SyncBN path."""
import collections

import pytest
import torch

from test_hip_glue_dryrun_cpu import DryLib, dry, _batch  # noqa: F401  (dry: the fixture)

# (C, stride, dil) of the 62 depthwise convs: entry flow 2 + 3 + 2 + 3, middle flow 16 x 3, exit flow 3 + 3
DW_MULTISET = collections.Counter({(64, 1, 1): 1, (128, 1, 1): 2, (128, 2, 1): 1, (256, 1, 1): 2, (728, 1, 1): 1, (728, 2, 1): 1,
                                   (728, 1, 2): 16 * 3 + 2, (1024, 1, 1): 1, (1024, 1, 4): 1, (1536, 1, 4): 2})


def _spy(monkeypatch, lib_type, names, log):
    real_getattr = lib_type.__getattr__

    def spy(self, name):
        fn = real_getattr(self, name)
        if name in names:
            def wrapped(*a):
                log.append((name, a))
                return fn(*a)
            return wrapped
        return fn
    monkeypatch.setattr(lib_type, "__getattr__", spy)


def _ptr(a):
    return None if a is None else (a.value if hasattr(a, "value") else a)


def _geom(a):
    d = a[0]._obj
    return d.C, d.stride, d.dil


def test_x71_train_step_and_eval_glue(dry, monkeypatch):
    from semseg_amd import hip_backend as hb
    from semseg_amd.loss import CrossEntropyLoss2d
    from semseg_amd.network import get_model
    log = []
    _spy(monkeypatch, type(dry), ("ssa_dwconv3x3", "ssa_dwconv3x3_bwd", "ssa_bn_stats", "ssa_bn_apply_train", "ssa_bn_apply"), log)
    assert sum(DW_MULTISET.values()) == 62
    net = get_model("deepv3.DeepV3PlusX71", 19, CrossEntropyLoss2d(ignore_index=255)).train()
    inputs = _batch()                                       # 2 x 64 x 96
    loss = net(inputs)
    assert loss.dim() == 0 and loss.requires_grad
    fwd = [a for n, a in log if n == "ssa_dwconv3x3"]
    assert len(fwd) == 62 and collections.Counter(_geom(a) for a in fwd) == DW_MULTISET
    nrep = hb.stat_replicas()
    train_sums = {_ptr(a[8]) for n, a in log if n == "ssa_bn_apply_train" and a[9] == nrep}
    dw_out = set()
    for a in fwd:
        d = a[0]._obj
        assert (d.Ho, d.Wo) == ((d.H - 1) // d.stride + 1, (d.W - 1) // d.stride + 1) and d.ldx >= d.C and d.ldy == d.C
        assert _ptr(a[1]) and _ptr(a[2]) and _ptr(a[3]) and _ptr(a[5]) is None and a[6] == 0
        assert _ptr(a[4]), "a training depthwise conv without the statistics epilogue"
        assert _ptr(a[4]) in train_sums, "the depthwise sums did not reach ssa_bn_apply_train with the replica count"
        dw_out.add(_ptr(a[3]))
    # (2 x 64 x 96: the entry flow's convs at /2 and /4, everything from block3's stride on at /8)
    assert sorted({(a[0]._obj.H, a[0]._obj.W) for a in fwd}) == [(8, 12), (16, 24), (32, 48)]
    stats_passes = [_ptr(a[0]) for n, a in log if n == "ssa_bn_stats"]
    assert not dw_out & set(stats_passes), "an inner BatchNorm took its statistics in a pass of its own"
    assert dry.calls["ssa_bn_update_running_batched"] == 1
    del log[:]
    loss.backward()
    missing = [n for n, p in net.named_parameters() if p.grad is None]
    assert not missing, missing[:5]
    for n, p in net.named_parameters():
        assert p.grad.shape == p.shape and p.grad.dtype == torch.float32, n
    bwd = [a for n, a in log if n == "ssa_dwconv3x3_bwd"]
    assert len(bwd) == 62 and collections.Counter(_geom(a) for a in bwd) == DW_MULTISET
    for a in bwd:
        d = a[0]._obj
        # x, dy, lddy, w, dx, lddx, dw, accumulate, ws: one pass for both gradients, added into the gradient arena
        assert _ptr(a[1]) and _ptr(a[2]) and a[3] >= d.C and _ptr(a[4]) and _ptr(a[5]) and a[6] == d.C
        assert _ptr(a[7]) and a[8] == 1 and _ptr(a[9])
    # eval: the inner BatchNorm is the depthwise kernel's epilogue (SSA_FUSE_EVAL_BN's default)
    net.eval()
    del log[:]
    with torch.no_grad():
        out = net({"images": inputs["images"]})
    assert tuple(out["pred"].shape) == (2, 19, 64, 96) and out["pred"].dtype == torch.float32
    ev = [a for n, a in log if n == "ssa_dwconv3x3"]
    assert len(ev) == 62 and collections.Counter(_geom(a) for a in ev) == DW_MULTISET
    for a in ev:
        assert _ptr(a[4]) is None and _ptr(a[5]) and a[6] == 0, "an eval depthwise conv without its BatchNorm epilogue"
    ev_out = {_ptr(a[3]) for a in ev}
    assert not ev_out & {_ptr(a[0]) for n, a in log if n == "ssa_bn_apply"}, "an inner BatchNorm ran as a pass of its own"
    assert not [1 for n, a in log if n in ("ssa_bn_stats", "ssa_bn_apply_train")]


def _dist_worker(rank, world, port, q):
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "semantic-segmentation_amd"), os.path.join(root, "tests")]
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from semseg_amd import _lib, hip_backend, ops, parallel, nn as snn
    from semseg_amd.config import cfg
    from semseg_amd.loss import CrossEntropyLoss2d
    from semseg_amd.network import get_model
    d = DryLib(_lib.lib())
    fused, counts = [], []
    real_getattr = DryLib.__getattr__

    def spy(self, name):
        fn = real_getattr(self, name)
        if name == "ssa_dwconv3x3":
            return lambda *a: (fused.append(_ptr(a[4])), fn(*a))[1]
        if name == "ssa_bn_apply_train":
            return lambda *a: (counts.append((_ptr(a[8]), a[6], a[10])), fn(*a))[1]
        return fn
    DryLib.__getattr__ = spy
    _lib._LIB = d
    hip_backend._s = lambda: None
    ops._set_backend_for_tests(ops.HipBackend())
    cfg.MODEL.BNFUNC = snn.SyncBatchNorm
    spans = []
    real = parallel.allreduce_bn_sums
    parallel.allreduce_bn_sums = lambda t, *a, **k: (spans.append((t.data_ptr(), t.numel())), real(t, *a, **k))[1]
    net = get_model("deepv3.DeepV3PlusX71", 19, CrossEntropyLoss2d(ignore_index=255)).train()
    net({"images": torch.randn(1, 3, 64, 64), "gts": torch.randint(0, 19, (1, 64, 64))}).backward()
    exchanged = all(p is not None and any(lo <= p < lo + 8 * n for lo, n in spans) for p in fused)
    # the global count (pixels x world) goes with the exchanged sums
    global_count = all(c == 2.0 * P for p, P, c in counts if p in set(fused))
    ok = all(p.grad is not None for p in net.parameters())
    q.put((rank, len(fused), exchanged, global_count, ok))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_x71_two_rank_syncbn_hands_the_depthwise_sums_to_the_exchange():
    """SyncBatchNorm over two gloo ranks: the sums ssa_dwconv3x3 accumulates are inside a span the SyncBN exchange
    all-reduces before ssa_bn_apply_train reads them, and that pass is given the global count."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dist_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=280) for _ in procs)
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    for rank, n_fused, exchanged, global_count, ok in got:
        assert n_fused == 62 and exchanged and global_count and ok, (rank, n_fused, exchanged, global_count, ok)
