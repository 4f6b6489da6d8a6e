"""The boundary F-score kernels (csrc/fboundary.hip) through the C ABI, through boundary_counts, eval_mask_boundary,
BoundaryMeter and eval_minibatch(boundary=...), on the cases of tests/fboundary_cases.py.

Every comparison is exact and covers every (image, class) entry: the four integer counts against tests/fboundary_ref.py
(pinned to the real reference by tests/test_fboundary_cpu.py), Fpc and Fc against the golden data of the real reference
with == in float64.  The full-size run is compared bit for bit with a composition of torch operators on the device
(per-class boundary maps, F.conv2d with the disk: sums below 2^24, exact in fp32).  tests/test_fboundary_emu_cpu.py
runs this file on the CPU emulation of the kernel sources (the full-size run skips there)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import evaltail_ref as ER
import fboundary_cases as K
import fboundary_ref as R
from fboundary_torch import torch_composition

pytestmark = pytest.mark.gpu

DEV = "cuda"
_EMU = bool(os.environ.get("SSA_EMU"))


def _hb():
    from semseg_amd import hip_backend
    return hip_backend


def _fb():
    from semseg_amd.utils import f_boundary
    return f_boundary


def _dev(name, gt_u8=False):
    pred, gt = K.inputs(name)
    g = torch.from_numpy(gt.copy())
    return torch.from_numpy(pred.copy()).to(DEV), (g.to(torch.uint8) if gt_u8 else g).to(DEV)


def _gt_kinds(name):
    return (False, True) if K.fits_u8(name) else (False,)


@pytest.mark.parametrize("name", K.ALL)
def test_c_abi(name):
    from semseg_amd import _lib
    hb, L, p = _hb(), _lib.lib(), _hb()._p
    k, ref = K.CASES[name], K.reference(name)
    for u8 in _gt_kinds(name):
        pred, gt = _dev(name, u8)
        B, H, W = pred.shape
        n = ctypes.c_size_t(0)
        assert L.ssa_fboundary_workspace_bytes(B, H, W, ctypes.byref(n)) == 0 and n.value == 8 * B * H * W
        counts = torch.full((B, k["C"], 4), -1, dtype=torch.int64, device=DEV)      # the first launch clears them
        work = torch.full((n.value // 4,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
        assert L.ssa_fboundary_counts(p(pred), p(gt), int(u8), B, H, W, k["C"], k["ignore"], ref["r"], p(counts), p(work),
                                      n.value, hb._s()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), ref["counts"]), (name, u8)


@pytest.mark.parametrize("name", K.ALL)
def test_boundary_counts(name):
    k, ref = K.CASES[name], K.reference(name)
    for u8 in _gt_kinds(name):
        pred, gt = _dev(name, u8)
        keep = (pred.clone(), gt.clone())
        counts = _fb().boundary_counts(pred, gt, k["C"], k["ignore"], k["bound_th"])
        torch.cuda.synchronize()
        assert counts.dtype == torch.int64 and counts.device == pred.device
        assert np.array_equal(counts.cpu().numpy(), ref["counts"]), (name, u8)
        assert torch.equal(pred, keep[0]) and torch.equal(gt, keep[1])             # the inputs are left as they were


@pytest.mark.parametrize("name", ("seam_r3", "labels65", "checker"))
def test_boundary_counts_on_non_contiguous_inputs(name):
    k, ref = K.CASES[name], K.reference(name)
    pred, gt = _dev(name)
    B, H, W = pred.shape
    wide = torch.full((B, H, W + 5), 7, dtype=torch.uint8, device=DEV)
    wide[:, :, 2:2 + W] = pred
    gt_t = gt.permute(0, 2, 1).contiguous().permute(0, 2, 1)                        # [B,H,W] view of [B,W,H] storage
    assert not wide[:, :, 2:2 + W].is_contiguous() and (not gt_t.is_contiguous() or min(H, W) == 1)
    counts = _fb().boundary_counts(wide[:, :, 2:2 + W], gt_t, k["C"], k["ignore"], k["bound_th"])
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy(), ref["counts"])


@pytest.mark.parametrize("name", K.ALL)
def test_eval_mask_boundary_equals_the_reference_fixture(name, monkeypatch):
    from semseg_amd.config import cfg
    g, k = K.golden(), K.CASES[name]
    monkeypatch.setattr(cfg.DATASET, "IGNORE_LABEL", k["ignore"])
    pred, gt = K.inputs(name)
    seg, gtm = pred.astype(np.int64), gt.copy()         # as the reference's caller holds them: int64 arrays on the host
    Fpc, Fc = _fb().eval_mask_boundary(seg, gtm, k["C"], num_proc=3, bound_th=k["bound_th"], device=DEV)
    assert isinstance(Fpc, np.ndarray) and Fpc.dtype == np.float64 and Fc.dtype == np.float64
    assert (Fpc == g[name + "/Fpc"]).all() and (Fc == g[name + "/Fc"]).all()
    assert np.array_equal(seg, pred) and np.array_equal(gtm, gt)                    # not mutated
    # tensors in, on either side
    Fpc2, Fc2 = _fb().eval_mask_boundary(torch.from_numpy(pred.copy()).to(DEV), torch.from_numpy(gt.copy()), k["C"],
                                         bound_th=k["bound_th"], device=DEV)
    assert (Fpc2 == Fpc).all() and (Fc2 == Fc).all()


def test_argument_rejection():
    """NULL, C = 0 / 255, radius 33, B = 0, a short workspace: -1 or -2, and nothing is launched."""
    from semseg_amd import _lib
    hb, L, p = _hb(), _lib.lib(), _hb()._p
    B, H, W, C = 1, 4, 6, 19
    pred = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    gt = torch.zeros((B, H, W), dtype=torch.int64, device=DEV)
    counts = torch.full((B, 255, 4), 3, dtype=torch.int64, device=DEV)
    work = torch.full((2 * B * H * W,), 5, dtype=torch.int32, device=DEV)
    s, nb = hb._s(), 8 * B * H * W
    before = L.ssa_launch_count(0)
    bad = (-1, -2)
    assert L.ssa_fboundary_counts(None, p(gt), 0, B, H, W, C, 255, 2, p(counts), p(work), nb, s) in bad
    assert L.ssa_fboundary_counts(p(pred), None, 0, B, H, W, C, 255, 2, p(counts), p(work), nb, s) in bad
    assert L.ssa_fboundary_counts(p(pred), p(gt), 0, B, H, W, C, 255, 2, None, p(work), nb, s) in bad
    assert L.ssa_fboundary_counts(p(pred), p(gt), 0, B, H, W, C, 255, 2, p(counts), None, nb, s) in bad
    for c in (0, 255, -3):
        assert L.ssa_fboundary_counts(p(pred), p(gt), 0, B, H, W, c, 255, 2, p(counts), p(work), nb, s) in bad
    for r in (33, -1):
        assert L.ssa_fboundary_counts(p(pred), p(gt), 0, B, H, W, C, 255, r, p(counts), p(work), nb, s) == -2
    for b in (0, 65536):
        assert L.ssa_fboundary_counts(p(pred), p(gt), 0, b, H, W, C, 255, 2, p(counts), p(work), nb, s) in bad
    assert L.ssa_fboundary_counts(p(pred), p(gt), 0, B, 0, W, C, 255, 2, p(counts), p(work), nb, s) in bad
    assert L.ssa_fboundary_counts(p(pred), p(gt), 0, B, H, W, C, 255, 2, p(counts), p(work), nb - 1, s) == -1
    assert L.ssa_launch_count(0) == before
    torch.cuda.synchronize()
    assert int((counts != 3).sum()) == 0 and int((work != 5).sum()) == 0
    with pytest.raises(ValueError):
        _fb().boundary_counts(pred, gt, C, 255, 33)
    with pytest.raises(ValueError):
        _fb().boundary_counts(pred, gt, 255, 255, 2)


def test_launch_budget():
    """Two kernel launches (the first clears the counters) and no memset."""
    from semseg_amd import _lib
    L = _lib.lib()
    pred, gt = _dev("seam_r3")
    n0 = L.ssa_launch_count(0)
    _fb().boundary_counts(pred, gt, 19, 255, 0.02)
    torch.cuda.synchronize()
    assert L.ssa_launch_count(0) - n0 == 2


def test_eval_minibatch_feeds_the_meter(monkeypatch):
    """eval_minibatch(boundary=meter): the meter holds what a separate update on the returned predictions gives, and
    what the restatement counts on them; without calc_metrics, and by default, nothing is fed."""
    from semseg_amd.config import cfg
    from semseg_amd.loss.criteria import CrossEntropyLoss2d
    from semseg_amd.utils import eval_minibatch, BoundaryMeter
    C, ignore = 19, 255
    monkeypatch.setattr(cfg.DATASET, "NUM_CLASSES", C)
    monkeypatch.setattr(cfg.DATASET, "IGNORE_LABEL", ignore)
    monkeypatch.setattr(cfg.MODEL, "MSCALE", True)
    data = ER.make_batch(2, 24, 40, C, ignore, seed=31)
    net = ER.MscaleStub(C, 3).to(DEV)
    crit = CrossEntropyLoss2d(ignore_index=ignore)
    meter = BoundaryMeter()
    assets, _ = eval_minibatch(data, net, crit, ER.Meter(), True, ER.Args(do_flip=True), 0, boundary=meter)
    torch.cuda.synchronize()
    preds, gts = assets["predictions"], data[1]
    apart = BoundaryMeter(C, ignore)
    apart.update(torch.from_numpy(preds).to(torch.uint8).to(DEV), gts.to(DEV))
    assert np.array_equal(meter.counts(), apart.counts())
    r = _fb().boundary_radius((24, 40), 0.008)
    assert np.array_equal(meter.counts(), R.counts(preds, gts.numpy(), C, ignore, r))
    F = R.scores(meter.counts())[0]
    Fpc, Fc = R.fpc_fc(F)
    assert (meter.Fpc == Fpc).all() and (meter.Fc == Fc).all() and meter.avg == float(np.mean(Fpc / Fc))
    quiet = BoundaryMeter()
    eval_minibatch(data, net, crit, ER.Meter(), False, ER.Args(do_flip=True), 0, boundary=quiet)
    assert quiet._counts == []
    again, _ = eval_minibatch(data, net, crit, ER.Meter(), True, ER.Args(do_flip=True), 0)
    assert np.array_equal(again["predictions"], preds)


def test_torch_composition_is_the_restatement():
    """(the yardstick of the full-size run, itself held to the restatement where that is cheap)"""
    k, ref = K.CASES["labels65"], K.reference("labels65")
    pred, gt = _dev("labels65")
    assert np.array_equal(torch_composition(pred, gt, k["C"], k["ignore"], ref["r"]).cpu().numpy(), ref["counts"])


@pytest.mark.skipif(_EMU, reason="two million pixels: the GPU runs it")
def test_full_size_against_the_torch_composition():
    """1 x 1024 x 2048 x 19 at radius 19 on labels of 64 x 64 blocks with 5 % ignore, the prediction shifted by (3, -5)
    with 3 % noise: grid-stride loops over 2,048 tiles, every count against the composition of torch operators
    (F.conv2d in row strips through torch's own im2col + GEMM: below a second on an MI355X)."""
    C, H, W = 19, 1024, 2048
    g = torch.Generator().manual_seed(41)
    gt = torch.randint(0, C, (1, H // 64, W // 64), generator=g).repeat_interleave(64, 1).repeat_interleave(64, 2).clone()
    pred = torch.roll(gt, (3, -5), (1, 2)).clone()
    noise = torch.rand(1, H, W, generator=g) < 0.03
    pred[noise] = torch.randint(0, C, (int(noise.sum()),), generator=g)
    gt[torch.rand(1, H, W, generator=g) < 0.05] = 255
    pred, gt = pred.to(torch.uint8).to(DEV), gt.to(DEV)
    assert _fb().boundary_radius((H, W), 0.008) == 19
    counts = _fb().boundary_counts(pred, gt, C, 255, 0.008)
    want = torch_composition(pred, gt, C, 255, 19)
    torch.cuda.synchronize()
    assert int(want[..., 0].min()) > 0 and int(want[..., 2].sum()) < int(want[..., 0].sum())
    assert torch.equal(counts, want)
