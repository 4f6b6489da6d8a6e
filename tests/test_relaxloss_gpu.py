"""The label relaxation kernels (csrc/relax_loss.hip) through the C ABI, through RelaxNllFn and through the public
criterion and transform, on cases 1-8 of tests/relaxloss_cases.py:

  class-set words, counts, the number of pixels without a class, class weights and the materialised multi-hot target
      bit for bit -- against the golden data of the real reference (cases 1-7) and tests/relaxloss_ref.py
  loss and gradient within check_close(1e-5, 1e-5) and (1e-4, 1e-4), the tolerances tests/test_kernels_gpu.py holds the
      cross entropy to -- against the golden data (cases 1-7) and the fp64 restatement (case 8)

Deviations seen on an MI355X are in profiles/relaxloss_notes.md.  tests/test_relaxloss_emu_cpu.py runs this file on the
CPU emulation of the kernel sources (the graph capture and the 1024 x 1024 run skip there: the GPU runs them)."""
import os

import numpy as np
import pytest
import torch

import relaxloss_cases as K
import relaxloss_ref as R
from util import check_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
_EMU = bool(os.environ.get("SSA_EMU"))
ALL = tuple(K.CASES)


def _hb():
    from semseg_amd import hip_backend
    return hip_backend


def _strict(k):
    return _hb().strict_bits(k["strict"], k["C"])


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _check_integers(n, sets, stats, w=None):
    ref = K.reference(n)
    assert torch.equal(sets.cpu(), ref["sets"]), "case %d: class sets" % n
    assert torch.equal(stats.cpu(), ref["stats"]), "case %d: counts" % n
    if w is not None:
        assert torch.equal(w.cpu().view(torch.int32), ref["w"].view(torch.int32)), "case %d: class weights" % n


def _check_floats(n, loss, grad_nhwc, tag):
    ref = K.reference(n)
    check_close("relax loss case %d %s" % (n, tag), loss.detach().reshape(1), ref["loss"].reshape(1), 1e-5, 1e-5)
    check_close("relax grad case %d %s" % (n, tag), grad_nhwc, _nhwc(ref["grad"]), 1e-4, 1e-4)
    if n == 7:      # image 0 has no pixel with a class: nothing of it reaches the loss
        assert float(grad_nhwc[0].abs().max()) == 0.0


@pytest.mark.parametrize("n", ALL)
def test_c_abi(n):
    from semseg_amd import _lib
    hb, L, p = _hb(), _lib.lib(), _hb()._p
    k, ref = K.CASES[n], K.reference(n)
    C, (B, H, W) = k["C"], k["shape"]
    labels = ref["labels"].long().to(DEV)
    lo, hi = _strict(k)
    sets = torch.full((B, H, W, 2), -1, dtype=torch.int64, device=DEV)
    stats = torch.full((B, C + 2), -1, dtype=torch.int64, device=DEV)
    assert L.ssa_relax_mask_labels(p(labels), 0, B, H, W, C, k["ignore"], k["border"], lo, hi, p(sets), p(stats), hb._s()) == 0
    _check_integers(n, sets, stats)
    # the reference's own target gives the same sets and counts
    mh_in = ref["mh"].to(DEV)
    sets2 = torch.full_like(sets, -1)
    stats2 = torch.full_like(stats, -1)
    assert L.ssa_relax_mask_multihot(p(mh_in), B, H, W, C, p(sets2), p(stats2), hb._s()) == 0
    assert torch.equal(sets2, sets) and torch.equal(stats2, stats)
    # ... and the sets give the reference's target back
    mh = torch.full((B, C + 1, H, W), 7, dtype=torch.uint8, device=DEV)
    assert L.ssa_relax_multihot(p(sets), B, H, W, C, p(mh), hb._s()) == 0
    assert torch.equal(mh.cpu(), ref["mh"])
    w = torch.full((B, C), -1.0, dtype=torch.float32, device=DEV)
    acc = torch.full((B,), 5.0, dtype=torch.float64, device=DEV)
    assert L.ssa_relax_weights(p(stats), B, C, k["ub"], int(k["batch"]), p(w), p(acc), hb._s()) == 0
    assert float(acc.abs().max()) == 0.0
    _check_integers(n, sets, stats, w)
    x = _nhwc(ref["logits"]).to(DEV)
    assert L.ssa_relax_nll_fwd(p(x), C, p(sets), p(w), B, H, W, C, p(acc), hb._s()) == 0
    loss = torch.zeros((), dtype=torch.float32, device=DEV)
    assert L.ssa_relax_nll_finalize(p(acc), p(stats), B, H, W, C, p(loss), hb._s()) == 0
    up = torch.tensor([k["up"]], dtype=torch.float32, device=DEV)
    g = torch.full((B, H, W, C), float("nan"), dtype=torch.float32, device=DEV)
    assert L.ssa_relax_nll_bwd(p(x), C, p(sets), p(w), p(stats), B, H, W, C, p(up), p(g), hb._s()) == 0
    torch.cuda.synchronize()
    _check_floats(n, loss, g, "abi")


def _fn(n, target, sliced=False):
    hb, k, ref = _hb(), K.CASES[n], K.reference(n)
    C = k["C"]
    x = _nhwc(ref["logits"]).to(DEV)
    if sliced:      # the logits as a channel slice of a wider NHWC buffer: ld = C + 5, the tile no longer 16-byte aligned
        wide = torch.full(x.shape[:3] + (C + 5,), float("nan"), dtype=torch.float32, device=DEV)
        wide[..., 3:3 + C] = x
        leaf = wide.requires_grad_(True)
        x = leaf[..., 3:3 + C]
    else:
        leaf = x.requires_grad_(True)
        x = leaf
    loss, sets, stats, w = hb.RelaxNllFn.apply(x, target, C, k["ignore"], k["border"], k["strict"], k["ub"], k["batch"])
    (loss * k["up"]).backward()
    torch.cuda.synchronize()
    g = leaf.grad[..., 3:3 + C] if sliced else leaf.grad
    return loss, sets, stats, w, g


@pytest.mark.parametrize("n", ALL)
def test_fn_on_uint8_labels(n):
    loss, sets, stats, w, g = _fn(n, K.reference(n)["labels"].to(DEV))
    _check_integers(n, sets, stats, w)
    _check_floats(n, loss, g, "fn")


@pytest.mark.parametrize("n", K.SLICED_CASES)
def test_fn_on_a_channel_slice(n):
    loss, sets, stats, w, g = _fn(n, K.reference(n)["labels"].long().to(DEV), sliced=True)
    _check_integers(n, sets, stats, w)
    _check_floats(n, loss, g, "sliced")


@pytest.mark.parametrize("n", (3, 5))
def test_fn_on_the_multihot_target(n):
    loss, sets, stats, w, g = _fn(n, K.reference(n)["mh"].to(DEV))
    _check_integers(n, sets, stats, w)
    _check_floats(n, loss, g, "multihot")


def test_criterion_reads_the_configuration(monkeypatch):
    """ImgWtLossSoftNLL on NCHW logits under case 3's cfg (strict classes, batch weighting) and, for B = 1, case 1's."""
    from semseg_amd.config import cfg
    from semseg_amd.loss import ImgWtLossSoftNLL
    monkeypatch.setattr(_hb(), "_FP16_TRAINING", [True])      # (the fp16-storage build: as with a loss scaler attached)
    for n in (3, 1):
        k, ref = K.CASES[n], K.reference(n)
        monkeypatch.setitem(cfg, "BORDER_WINDOW", k["border"])
        monkeypatch.setitem(cfg, "STRICTBORDERCLASS", k["strict"])
        monkeypatch.setitem(cfg, "BATCH_WEIGHTING", k["batch"])
        x = ref["logits"].to(DEV).requires_grad_(True)
        crit = ImgWtLossSoftNLL(k["C"], ignore_index=k["ignore"], upper_bound=k["ub"])
        loss = crit(x, ref["labels"].long().to(DEV), do_rmi=True)
        (loss * k["up"]).backward()
        torch.cuda.synchronize()
        _check_floats(n, loss, _nhwc(x.grad), "criterion")


def test_launch_budget():
    """Forward from label maps: five kernel launches (the counters are cleared by the first) and no memset; backward: one."""
    from semseg_amd import _lib
    hb, L, ref = _hb(), _lib.lib(), K.reference(2)
    x = _nhwc(ref["logits"]).to(DEV).requires_grad_(True)
    labels = ref["labels"].long().to(DEV)
    n0 = L.ssa_launch_count(0)
    loss = hb.RelaxNllFn.apply(x, labels, 19, 255, 1, None, 1.0, False)[0]
    n1 = L.ssa_launch_count(0)
    loss.backward()
    torch.cuda.synchronize()
    assert (n1 - n0, L.ssa_launch_count(0) - n1) == (5, 1)


def test_public_transform(monkeypatch):
    from semseg_amd.config import cfg
    from semseg_amd.datasets.transforms import RelaxedBoundaryLossToTensor
    for n in K.GOLDEN_CASES:
        k, ref = K.CASES[n], K.reference(n)
        monkeypatch.setitem(cfg, "BORDER_WINDOW", k["border"])
        monkeypatch.setitem(cfg, "STRICTBORDERCLASS", k["strict"])
        tr = RelaxedBoundaryLossToTensor(k["ignore"], k["C"])
        out = tr(ref["labels"].to(DEV))
        assert out.dtype == torch.uint8 and torch.equal(out.cpu(), ref["mh"]), n
        one = tr(ref["labels"][-1].long().to(DEV))
        assert torch.equal(one.cpu(), ref["mh"][-1]), n
    # H * W a multiple of 4 (the word stores of the materialising kernel), two label tiles in both directions, border 2
    monkeypatch.setitem(cfg, "BORDER_WINDOW", 2)
    monkeypatch.setitem(cfg, "STRICTBORDERCLASS", [1])
    g = torch.Generator().manual_seed(5)
    lab = torch.randint(0, 7, (2, 16, 36), generator=g)
    lab[torch.rand(2, 16, 36, generator=g) < 0.2] = 255
    lab[0, 3:12, 20:30] = 9            # outside [0, C) and not the ignore label: the ignore channel all the same
    out = RelaxedBoundaryLossToTensor(255, 7)(lab.to(DEV))
    assert np.array_equal(out.cpu().numpy(), R.multihot(lab.numpy(), 7, 255, 2, [1]))


def test_argument_rejection():
    """C = 0, C = 128, border 3 and null pointers: -1 or -2, and nothing is launched."""
    from semseg_amd import _lib
    hb, L, p = _hb(), _lib.lib(), _hb()._p
    B, H, W, C = 1, 4, 4, 19
    lab = torch.zeros((B, H, W), dtype=torch.int64, device=DEV)
    sets = torch.zeros((B, H, W, 2), dtype=torch.int64, device=DEV)
    stats = torch.zeros((B, 130), dtype=torch.int64, device=DEV)
    mh = torch.zeros((B, 130, H, W), dtype=torch.uint8, device=DEV)
    x = torch.zeros((B, H, W, 128), dtype=torch.float32, device=DEV)
    w = torch.zeros((B, 128), dtype=torch.float32, device=DEV)
    acc = torch.zeros((B,), dtype=torch.float64, device=DEV)
    up = torch.ones((1,), dtype=torch.float32, device=DEV)
    s = hb._s()
    before = L.ssa_launch_count(0)
    bad = (-1, -2)
    for c in (0, 128, -3):
        assert L.ssa_relax_mask_labels(p(lab), 0, B, H, W, c, 255, 1, 0, 0, p(sets), p(stats), s) in bad
        assert L.ssa_relax_mask_multihot(p(mh), B, H, W, c, p(sets), p(stats), s) in bad
        assert L.ssa_relax_multihot(p(sets), B, H, W, c, p(mh), s) in bad
        assert L.ssa_relax_weights(p(stats), B, c, 1.0, 0, p(w), p(acc), s) in bad
        assert L.ssa_relax_nll_fwd(p(x), 128, p(sets), p(w), B, H, W, c, p(acc), s) in bad
        assert L.ssa_relax_nll_finalize(p(acc), p(stats), B, H, W, c, p(up), s) in bad
        assert L.ssa_relax_nll_bwd(p(x), 128, p(sets), p(w), p(stats), B, H, W, c, p(up), p(x), s) in bad
    for b in (3, -1):
        assert L.ssa_relax_mask_labels(p(lab), 0, B, H, W, C, 255, b, 0, 0, p(sets), p(stats), s) == -2
    assert L.ssa_relax_mask_labels(None, 0, B, H, W, C, 255, 1, 0, 0, p(sets), p(stats), s) in bad
    assert L.ssa_relax_mask_labels(p(lab), 0, B, H, W, C, 255, 1, 0, 0, None, p(stats), s) in bad
    assert L.ssa_relax_mask_labels(p(lab), 0, B, H, W, C, 255, 1, 0, 0, p(sets), None, s) in bad
    assert L.ssa_relax_mask_labels(p(lab), 0, B, 0, W, C, 255, 1, 0, 0, p(sets), p(stats), s) in bad
    assert L.ssa_relax_mask_multihot(None, B, H, W, C, p(sets), p(stats), s) in bad
    assert L.ssa_relax_multihot(p(sets), B, H, W, C, None, s) in bad
    assert L.ssa_relax_weights(p(stats), B, C, 1.0, 0, None, p(acc), s) in bad
    assert L.ssa_relax_weights(p(stats), B, C, 1.0, 0, p(w), None, s) in bad
    assert L.ssa_relax_nll_fwd(None, C, p(sets), p(w), B, H, W, C, p(acc), s) in bad
    assert L.ssa_relax_nll_fwd(p(x), C - 1, p(sets), p(w), B, H, W, C, p(acc), s) in bad       # ld < C
    assert L.ssa_relax_nll_finalize(p(acc), None, B, H, W, C, p(up), s) in bad
    assert L.ssa_relax_nll_bwd(p(x), C, p(sets), p(w), p(stats), B, H, W, C, None, p(x), s) in bad
    assert L.ssa_relax_nll_bwd(p(x), C, p(sets), p(w), p(stats), B, H, W, C, p(up), None, s) in bad
    assert L.ssa_launch_count(0) == before
    torch.cuda.synchronize()
    assert int(sets.abs().max()) == 0 and int(stats.abs().max()) == 0


@pytest.mark.skipif(_EMU, reason="graph capture needs the device")
def test_graph_capture_replayed_on_two_inputs():
    """One torch.cuda.graph over forward + backward at case 2's shape, replayed on two different label maps and logits:
    each replay equals its eager run -- the counters are cleared inside the graph, nothing in it depends on the host.
    (The process keeps the default number of hardware queues.)"""
    hb, k = _hb(), K.CASES[2]
    C, (B, H, W) = k["C"], k["shape"]
    feeds = []
    for n in (2, 1):
        ref = K.reference(n)
        lab = ref["labels"].long()
        lg = _nhwc(ref["logits"])
        if n == 1:      # case 1 is one image: stack it with its mirror
            lab = torch.cat([lab, lab.flip(2)])
            lg = torch.cat([lg, lg.flip(2)])
        feeds.append((lab, lg))
    labels = feeds[0][0].to(DEV)
    x = feeds[0][1].to(DEV).requires_grad_(True)
    up = torch.tensor(k["up"], dtype=torch.float32, device=DEV)

    def step():
        loss, sets, stats, w = hb.RelaxNllFn.apply(x, labels, C, k["ignore"], k["border"], None, k["ub"], False)
        g, = torch.autograd.grad(loss * up, x)
        return loss, sets, stats, w, g

    eager = []
    for lab, lg in feeds:
        labels.copy_(lab)
        with torch.no_grad():
            x.copy_(lg)
        eager.append([t.detach().clone() for t in step()])
    torch.cuda.synchronize()
    _check_integers(2, eager[0][1], eager[0][2], eager[0][3])
    _check_floats(2, eager[0][0], eager[0][4], "eager")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for i in (1, 0, 1):
        labels.copy_(feeds[i][0])
        with torch.no_grad():
            x.copy_(feeds[i][1])
        graph.replay()
        torch.cuda.synchronize()
        for j in (1, 2):
            assert torch.equal(out[j], eager[i][j]), (i, j)
        assert torch.equal(out[3].view(torch.int32), eager[i][3].view(torch.int32)), i
        check_close("replay %d loss" % i, out[0].reshape(1), eager[i][0].reshape(1), 1e-5, 1e-5)
        check_close("replay %d grad" % i, out[4], eager[i][4], 1e-4, 1e-4)


@pytest.mark.skipif(_EMU, reason="a million pixels: the GPU runs it")
def test_full_size_counts_and_loss():
    """1 x 1024 x 1024 x 19 on a label map of 64 x 64 blocks: the integer outputs and the loss against the restatement
    -- grid-stride loops and 32-bit index products past their first wrap."""
    hb = _hb()
    C, H, W = 19, 1024, 1024
    g = torch.Generator().manual_seed(11)
    lab = torch.randint(0, C, (1, 16, 16), generator=g).repeat_interleave(64, 1).repeat_interleave(64, 2).clone()
    lab[torch.rand(1, H, W, generator=g) < 0.05] = 255
    lab[0, 100:140, 900:960] = 255
    logits = torch.randn(1, C, H, W, generator=g) * 2
    mh = R.multihot(lab.numpy(), C, 255, 1, None)
    x = _nhwc(logits).to(DEV)
    loss, sets, stats, w = hb.RelaxNllFn.apply(x, lab.to(torch.uint8).to(DEV), C, 255, 1, None, 1.0, False)
    torch.cuda.synchronize()
    assert torch.equal(sets.cpu(), R.class_sets(mh)) and torch.equal(stats.cpu(), R.stats(mh))
    assert torch.equal(w.cpu().view(torch.int32), R.class_weights(mh).view(torch.int32))
    want = R.loss(logits, mh)
    check_close("relax loss 1024", loss.reshape(1), want.reshape(1), 1e-5, 1e-5)
