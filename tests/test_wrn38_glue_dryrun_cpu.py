"""Dry run of the HIP host glue (tests/test_hip_glue_dryrun_cpu.py's machinery: the real library's host entry points,
signature-checked stand-ins for every launch, CPU tensors) for deepv3.DeepV3PlusW38: a train step and an eval pass, the
argument patterns of the two entry points of the pre-activation blocks, and the two-rank SyncBN path."""
import pytest
import torch

from test_hip_glue_dryrun_cpu import DryLib, dry, _batch  # noqa: F401  (dry: the fixture)

HEADS = 15          # blocks whose input is an open (conv output, shortcut) pair: all 17 but mod2.block1 and mod3.block1
IDENTITY = 11       # of these, the blocks without a projection: their input is also their shortcut


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


def test_wrn38_train_step_and_eval_glue(dry, monkeypatch):
    from semseg_amd.loss import CrossEntropyLoss2d
    from semseg_amd.network import get_model
    from semseg_amd.network.wider_resnet import IdentityResidualBlock
    log = []
    _spy(monkeypatch, type(dry), ("ssa_add_bn_stats", "ssa_bn_bwd_apply_add", "ssa_bn_bwd_apply", "ssa_bn_apply_train"), log)
    net = get_model("deepv3.DeepV3PlusW38", 19, CrossEntropyLoss2d(ignore_index=255)).train()
    blocks = [m for m in net.modules() if isinstance(m, IdentityResidualBlock)]
    assert len(blocks) == 17 and sum(1 for b in blocks if not hasattr(b, "proj_conv")) == IDENTITY
    inputs = _batch()                                       # 2 x 64 x 96
    loss = net(inputs)
    assert loss.dim() == 0 and loss.requires_grad
    fwd = [a for n, a in log if n == "ssa_add_bn_stats"]
    assert len(fwd) == HEADS
    train_sums = {_ptr(a[8]) for n, a in log if n == "ssa_bn_apply_train" and a[9] == 1}
    shapes = []
    for a in fwd:
        pa, lda, pb, ldb, ps, lds, P, C, sums, zero, stream = a
        assert _ptr(pa) and _ptr(pb) and _ptr(ps) and _ptr(sums) and zero == 0
        assert lda >= C and ldb >= C and lds == C and C % 8 == 0 and C <= 2048
        assert _ptr(sums) in train_sums, "the fused sums did not reach ssa_bn_apply_train with nrep = 1"
        shapes.append((P, C))
    # P per level at 2 x 64 x 96: /2 in mod2, /4 in mod3, /8 from mod4.block1's stride on
    p2, p4, p8 = 2 * 32 * 48, 2 * 16 * 24, 2 * 8 * 12
    assert shapes == [(p2, 128)] * 2 + [(p4, 256)] * 2 + [(p4, 256)] + [(p8, 512)] * 5 + [(p8, 512)] + [(p8, 1024)] * 2 + \
        [(p8, 1024), (p8, 2048)]
    assert dry.calls["ssa_bn_update_running_batched"] == 1
    del log[:]
    loss.backward()
    missing = [n for n, p in net.named_parameters() if p.grad is None]
    assert not missing, missing[:5]
    for n, p in net.named_parameters():
        assert p.grad.shape == p.shape and p.grad.dtype == torch.float32, n
    bwd = [a for n, a in log if n == "ssa_bn_bwd_apply_add"]
    assert len(bwd) == IDENTITY, "ssa_bn_bwd_apply_add is called exactly once per identity block"
    for a in bwd:
        x, ldx, dz, lddz, z, ldz, dx, lddx, dres, lddres, P, C = a[:12]
        relu, post, msc, msh, mask, dadd, lddadd = a[18], a[19], a[24], a[25], a[27], a[28], a[29]
        assert _ptr(x) and _ptr(dz) and _ptr(dx) and _ptr(z) is None and _ptr(dres) is None and _ptr(mask) is None
        assert relu == 1 and _ptr(msc) and _ptr(msh) and _ptr(post) is None
        assert _ptr(dadd) and lddadd >= C and ldx == C and lddx == C
    assert sorted(a[11] for a in bwd) == sorted([128] * 2 + [256] * 2 + [512] * 5 + [1024] * 2)
    # the four projection blocks behind an open pair: nobody else reads their input, the plain pass serves them
    plain = [a for n, a in log if n == "ssa_bn_bwd_apply" and _ptr(a[24])]
    assert len(plain) >= HEADS - IDENTITY
    # eval: ssa_sum_act closes the pairs, no statistics are taken
    net.eval()
    before = dry.calls["ssa_add_bn_stats"], dry.calls["ssa_sum_act"]
    with torch.no_grad():
        out = net({"images": inputs["images"]})
    assert tuple(out["pred"].shape) == (2, 19, 64, 96) and out["pred"].dtype == torch.float32
    assert dry.calls["ssa_add_bn_stats"] == before[0] and dry.calls["ssa_sum_act"] >= before[1] + 17


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
        if name == "ssa_add_bn_stats":
            return lambda *a: (fused.append(_ptr(a[8])), fn(*a))[1]
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
    net = get_model("deepv3.DeepV3PlusW38", 19, CrossEntropyLoss2d(ignore_index=255)).train()
    net({"images": torch.randn(1, 3, 64, 64), "gts": torch.randint(0, 19, (1, 64, 64))}).backward()
    exchanged = all(any(lo <= p < lo + 8 * n for lo, n in spans) for p in fused)
    # the global count (pixels x world) goes with the exchanged sums
    global_count = all(c == 2.0 * P for p, P, c in counts if p in set(fused))
    ok = all(p.grad is not None for p in net.parameters())
    q.put((rank, len(fused), exchanged, global_count, ok))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_wrn38_two_rank_syncbn_hands_the_fused_sums_to_the_exchange():
    """SyncBatchNorm over two gloo ranks: the sums ssa_add_bn_stats accumulates are inside a span the SyncBN exchange
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
        assert n_fused == HEADS and exchanged and global_count and ok, (rank, n_fused, exchanged, global_count, ok)
