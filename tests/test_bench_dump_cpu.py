"""bench.py --dump-outputs: the files it writes, the fixed sample of large tensors (the same elements in every run,
so that two builds compare output for output), the restore of the state the dumped step starts from, and the 64 MB
bound on the benchmarked model.  No GPU: the dump is taken from a small CPU module."""
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn


@pytest.fixture
def bench(monkeypatch):
    # bench.py reads its own argv and defaults SSA_ACT_DTYPE at import: keep this process's storage format
    monkeypatch.setenv("SSA_ACT_DTYPE", os.environ.get("SSA_ACT_DTYPE", "bf16"))
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    import bench
    return bench


def _net():
    """A trained-once module: parameters above the sample size, BatchNorm running statistics, an integer buffer."""
    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8), nn.Flatten(), nn.Linear(8 * 6 * 6, 40))
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    loss = net(x).square().mean()
    loss.backward()
    return net, float(loss.detach())


def test_dump_index_is_fixed_and_bounded(bench):
    k = bench.DUMP_SAMPLE
    assert torch.equal(bench._dump_index(100, 3), torch.arange(100))
    a, b = bench._dump_index(10 * k, 7), bench._dump_index(10 * k, 7)
    assert torch.equal(a, b) and a.numel() == k
    assert int(a.min()) >= 0 and int(a.max()) < 10 * k
    assert not torch.equal(a, bench._dump_index(10 * k, 8))


def test_dump_outputs_writes_the_step_state(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)    # the Linear weight (11520 elements) is sampled
    net, loss = _net()
    bench.dump_outputs(str(tmp_path / "a"), net, loss)
    bench.dump_outputs(str(tmp_path / "b"), net, loss)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["bn_buffers.npy", "loss.npy", "params.npy"]
    for n in names:
        got = np.load(tmp_path / "a" / n)
        assert got.dtype in (np.float32, np.float64), n
        assert np.array_equal(got, np.load(tmp_path / "b" / n)), n
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [loss]
    want = []
    for i, (_, p) in enumerate(net.named_parameters()):
        idx = bench._dump_index(p.numel(), i)
        assert idx.numel() == min(p.numel(), 1000)
        want.append(p.detach().reshape(-1)[idx])
    assert np.array_equal(np.load(tmp_path / "a" / "params.npy"), torch.cat(want).numpy())
    bn = net[1]
    assert np.array_equal(np.load(tmp_path / "a" / "bn_buffers.npy"),
                          torch.cat([bn.running_mean, bn.running_var]).numpy())


def test_restored_state_repeats_the_first_step(bench):
    """The dumped step starts from the state before the first step: after steps that moved parameters, momentum and
    BatchNorm statistics, restore_step_state brings back exactly that state, and the step repeats the first one."""
    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8), nn.Flatten(), nn.Linear(8 * 6 * 6, 4))
    optim = torch.optim.SGD(net.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    saved = bench.step_state(net, None)

    def step():
        optim.zero_grad(set_to_none=True)
        loss = net(x).square().mean()
        loss.backward()
        optim.step()
        return float(loss.detach()), [t.detach().clone() for t in list(net.parameters()) + list(net.buffers())]

    first = step()
    for _ in range(3):
        step()
    assert not torch.equal(net[0].weight, saved[0][1])
    bench.restore_step_state(saved, optim)
    for t, v in saved:
        assert torch.equal(t, v)
    assert all(not st["momentum_buffer"].any() for st in optim.state.values())
    again = step()
    assert again[0] == first[0]
    assert all(torch.equal(a, b) for a, b in zip(again[1], first[1]))


def test_dump_of_the_benchmarked_model_stays_under_64_mb(bench):
    from semseg_amd.config import cfg
    from semseg_amd.loss import RMILoss
    from semseg_amd.network import ocrnet
    saved = (cfg.LOSS.SUPERVISED_MSCALE_WT, cfg.LOSS.OCR_AUX_RMI, cfg.MODEL.N_SCALES)
    try:
        cfg.LOSS.SUPERVISED_MSCALE_WT, cfg.LOSS.OCR_AUX_RMI, cfg.MODEL.N_SCALES = 0.05, False, None
        net = ocrnet.HRNet_Mscale(19, RMILoss(num_classes=19, ignore_index=255))
    finally:
        cfg.LOSS.SUPERVISED_MSCALE_WT, cfg.LOSS.OCR_AUX_RMI, cfg.MODEL.N_SCALES = saved
    sampled = sum(min(p.numel(), bench.DUMP_SAMPLE) for p in net.parameters())
    buffers = sum(b.numel() for b in net.buffers() if b.is_floating_point())
    total = (sampled + buffers) * 4 + 8
    assert total <= 64 * 2 ** 20, total
