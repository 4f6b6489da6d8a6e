"""ssa_eval_tail and semseg_amd.utils.eval_minibatch against the CPU restatement of the reference's evaluation tail
(tests/evaltail_ref.py; pinned to the reference by tests/test_eval_tail_cpu.py).  Expected values never come from the
code under test.  Integer outputs are compared exactly under the precondition, asserted on the CPU, that the argmax of
softmax(out) is the argmax of out; `avg` bit for bit; the probability against an fp64 softmax of the same fp32 `out`
to (2C + 8) * 2^-24 relative (a C-term fp32 sum, one exp per term, one reciprocal); the loss as
test_kernels_gpu.py::test_cross_entropy does (1e-5)."""
import os

import numpy as np
import pytest
import torch

import evaltail_ref as R
from util import check_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
EMU = bool(os.environ.get("SSA_EMU"))


def _sync():
    torch.cuda.synchronize()


def _logits(n, B, C, H, W, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, C, H, W, generator=g) * scale for _ in range(n)]


def _labels(B, H, W, C, ignore, seed, negative=False):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, C, (B, H, W), generator=g)
    r = torch.rand(B, H, W, generator=g)
    lab[r < 0.1] = ignore
    if negative:
        lab[(r >= 0.1) & (r < 0.13)] = -1
    return lab.long()


def _on_device(t, layout):
    """[B,C,H,W] CPU tensor -> the same values on DEV as the permuted view of an NHWC buffer ("view": what the networks
    return), a contiguous NCHW tensor ("nchw") or a channel slice of a wider NHWC buffer ("slice": ld != C)."""
    if layout == "nchw":
        return t.to(DEV).contiguous()
    x = t.permute(0, 2, 3, 1).contiguous()
    if layout == "slice":
        wide = torch.full(x.shape[:3] + (x.shape[3] + 5,), 1e30)
        wide[..., 2:2 + x.shape[3]] = x
        return wide.to(DEV)[..., 2:2 + x.shape[3]].permute(0, 3, 1, 2)
    return x.to(DEV).permute(0, 3, 1, 2)


def _prob_bound(C):
    return (2 * C + 8) * 2.0 ** -24


def _check_prob(prob, out, C):
    ref = torch.softmax(out.double(), dim=1).max(1)[0]
    rel = ((prob.cpu().double() - ref).abs() / ref).max().item()
    print("prob: max relative error %.3g (bound %.3g)" % (rel, _prob_bound(C)))
    assert rel <= _prob_bound(C), (rel, _prob_bound(C))


def _run_case(srcs, flips, div, C, ignore, lab, layouts=None, with_loss=True, avg=True):
    from semseg_amd.utils import eval_tail
    ref = R.tail(srcs, flips, div[0], div[1], lab, C, ignore, with_loss=with_loss)
    assert R.argmax_is_softmax_argmax(ref["avg"])
    layouts = layouts or ["view"] * len(srcs)
    dsrcs = [_on_device(s, l) for s, l in zip(srcs, layouts)]
    res = eval_tail(dsrcs, flips, C, gts=None if lab is None else lab.to(DEV), ignore_label=ignore, n_scales=div[0],
                    n_flips=div[1], avg=avg)
    _sync()
    assert res.pred.dtype == torch.uint8 and np.array_equal(res.pred.cpu().numpy().astype(np.int64), ref["predictions"])
    if avg:
        assert tuple(res.avg.shape) == tuple(ref["avg"].shape)
        assert torch.equal(res.avg.cpu(), ref["avg"]), float((res.avg.cpu() - ref["avg"]).abs().max())
    _check_prob(res.prob, ref["avg"], C)
    if lab is not None:
        assert np.array_equal(res.err.cpu().numpy().astype(int), ref["err_mask"])
        assert res.hist.dtype == torch.int64 and np.array_equal(res.hist.cpu().numpy(), ref["hist"])
        if with_loss:
            print("loss: device %.8g reference %.8g" % (res.loss(), ref["loss"]))
            check_close("loss", torch.tensor([res.loss()]), torch.tensor([ref["loss"]]), 1e-5, 1e-5)
    return res, ref


def test_mapillary_two_sources_first_mirrored():
    """B=2, C=65, ignore 65, 37x61, the recipe's do_flip pair: (0.0 + flip(a) + b) / 1 / 2."""
    B, C, H, W = 2, 65, 37, 61
    _run_case(_logits(2, B, C, H, W, 1), [1, 0], (1, 2), C, 65, _labels(B, H, W, C, 65, 2))


def test_cityscapes_ties_and_negative_labels():
    """C=19, ignore 255, labels -1 present, 67x93; exact ties between two classes and all-equal rows: the first maximum
    wins.  (No loss here: the reference's nll_loss refuses a label of -1.)"""
    B, C, H, W = 1, 19, 67, 93
    a, b = _logits(2, B, C, H, W, 3)
    a[:, :, 5:9] = 0.0
    b[:, :, 5:9] = 0.0                      # all-equal rows -> class 0
    a[:, 7, 20:30] = 50.0
    a[:, 3, 20:30] = 50.0                   # tie of classes 3 and 7 (b mirrored adds the same to both)
    b[:, 7, 20:30] = b[:, 3, 20:30]
    res, ref = _run_case([a, b], [0, 1], (1, 2), C, 255, _labels(B, H, W, C, 255, 4, negative=True), with_loss=False)
    assert (ref["predictions"][:, 5:9] == 0).all() and (ref["predictions"][:, 20:30] == 3).all()


def test_cityscapes_loss():
    B, C, H, W = 1, 19, 67, 93
    _run_case(_logits(2, B, C, H, W, 5), [1, 0], (1, 2), C, 255, _labels(B, H, W, C, 255, 6))


def test_six_sources_pin_summation_order_and_divisions():
    """Scales 1.0, 0.5, 2.0 x flips 1, 0 (already at the input size), / 3 / 2: `avg` bit-equal."""
    B, C, H, W = 1, 19, 31, 45
    _run_case(_logits(6, B, C, H, W, 7), [1, 1, 1, 0, 0, 0], (3, 2), C, 255, _labels(B, H, W, C, 255, 8))


@pytest.mark.parametrize("layouts", [("view", "view"), ("nchw", "view"), ("slice", "slice"), ("slice", "view")])
@pytest.mark.parametrize("C,shape", [(128, (1, 9, 70)), (19, (2, 5, 301)), (65, (1, 3, 131))])
def test_layouts_class_counts_and_ragged_tiles(C, shape, layouts):
    """The permuted view of an NHWC buffer, a contiguous NCHW tensor, a channel slice of a wider NHWC buffer (ld != C, an
    unaligned base: the scalar staging path), mixed; 128 classes; row lengths that are no multiple of the tile."""
    B, H, W = shape
    _run_case(_logits(2, B, C, H, W, C), [1, 0], (1, 2), C, C, _labels(B, H, W, C, C, C + 1), layouts=list(layouts))


def test_histogram_and_loss_accumulate_over_calls():
    from semseg_amd.utils import eval_tail
    B, C, H, W = 1, 19, 21, 33
    a, b = _logits(2, B, C, H, W, 11)
    la, lb = _labels(B, H, W, C, 255, 12), _labels(B, H, W, C, 255, 13)
    ra = R.tail([a], [0], 1, 1, la, C, 255)
    rb = R.tail([b], [1], 1, 1, lb, C, 255)
    r1 = eval_tail([_on_device(a, "view")], [0], C, gts=la.to(DEV))
    r2 = eval_tail([_on_device(b, "view")], [1], C, gts=lb.to(DEV), hist=r1.hist, loss_acc=r1.loss_acc)
    _sync()
    assert r2.hist is r1.hist and np.array_equal(r2.hist.cpu().numpy(), ra["hist"] + rb["hist"])
    na, nb = int((la != 255).sum()), int((lb != 255).sum())
    acc = r2.loss_acc.cpu().tolist()
    assert acc[1] == na + nb
    check_close("loss sum", torch.tensor([acc[0]]), torch.tensor([ra["loss"] * na + rb["loss"] * nb]), 1e-5, 1e-5)


def test_all_labels_ignored():
    from semseg_amd.utils import eval_tail
    B, C, H, W = 1, 19, 11, 17
    (a,) = _logits(1, B, C, H, W, 14)
    lab = torch.full((B, H, W), 255, dtype=torch.int64)
    ref = R.tail([a], [0], 1, 1, lab, C, 255)
    res = eval_tail([_on_device(a, "view")], [0], C, gts=lab.to(DEV))
    _sync()
    assert np.isnan(ref["loss"]) and np.isnan(res.loss())
    assert int(res.hist.sum()) == 0 and int(res.err.sum()) == 0 and ref["hist"].sum() == 0 and ref["err_mask"].sum() == 0
    assert np.array_equal(res.pred.cpu().numpy().astype(np.int64), ref["predictions"])


def test_without_labels_only_predictions_and_probability():
    B, C, H, W = 1, 19, 11, 17
    res, _ = _run_case(_logits(1, B, C, H, W, 15), [0], (1, 1), C, 255, None, avg=False)
    assert res.err is None and res.hist is None and res.loss_acc is None and res.avg is None


@pytest.mark.skipif(EMU, reason="full size: the emulation runs a workgroup as 256 fibers")
@pytest.mark.parametrize("C,H,W,ignore", [(19, 1024, 2048, 255), (65, 1632, 2177, 65)])
def test_full_size(C, H, W, ignore):
    g = torch.Generator().manual_seed(C)
    srcs = [torch.randn(1, H, W, C, generator=g).mul_(3.0).permute(0, 3, 1, 2) for _ in range(2)]
    _run_case(srcs, [1, 0], (1, 2), C, ignore, _labels(1, H, W, C, ignore, C + 2))


# ------------------------------------------------------------------------------------------------ eval_minibatch
class _Cfg:
    """semseg_amd.config.cfg set for one test and restored."""

    def __init__(self, C, ignore, mscale):
        self.v = (C, ignore, mscale)

    def __enter__(self):
        from semseg_amd.config import cfg
        self.saved = (cfg.DATASET.NUM_CLASSES, cfg.DATASET.IGNORE_LABEL, cfg.MODEL.MSCALE)
        cfg.DATASET.NUM_CLASSES, cfg.DATASET.IGNORE_LABEL, cfg.MODEL.MSCALE = self.v

    def __exit__(self, *a):
        from semseg_amd.config import cfg
        cfg.DATASET.NUM_CLASSES, cfg.DATASET.IGNORE_LABEL, cfg.MODEL.MSCALE = self.saved


def _both_sides(make_net, data, args, C, ignore, mscale):
    from semseg_amd.loss.criteria import CrossEntropyLoss2d
    from semseg_amd.utils import eval_minibatch
    dbg, ref_loss, got_loss = {}, R.Meter(), R.Meter()
    ref = R.eval_minibatch(data, make_net(), R.CpuCrossEntropyLoss2d(ignore), ref_loss, True, args, 0, C, ignore, mscale,
                           debug=dbg)
    assert R.argmax_is_softmax_argmax(dbg["output"])
    with _Cfg(C, ignore, mscale):
        got = eval_minibatch(data, make_net().to(DEV), CrossEntropyLoss2d(ignore_index=ignore), got_loss, True, args, 0)
    _sync()
    (ra, rh), (ga, gh) = ref, got
    assert list(ga.keys()) == list(ra.keys())
    for k in ra:
        assert type(ga[k]) is type(ra[k]), k
        assert ga[k].dtype == ra[k].dtype and tuple(ga[k].shape) == tuple(ra[k].shape), k
    assert not ga["prob_mask"].is_cuda
    assert gh.dtype == rh.dtype and gh.shape == rh.shape
    assert got_loss.count == ref_loss.count
    return ra, rh, ga, gh, dbg["output"], ref_loss.avg, got_loss.avg


@pytest.mark.parametrize("C,ignore", [(19, 255), (65, 65)])
def test_eval_minibatch_mscale_do_flip(C, ignore):
    """MSCALE + do_flip: two passes, (0.0 + flip(pred(flip(x))) + pred(x)) / 1 / 2; the stub's outputs are one rounding
    each, so both sides see the same logits bit for bit: every integer asset and the histogram are equal."""
    data = R.make_batch(2, 24, 40, C, ignore, seed=C)
    ra, rh, ga, gh, out, rl, gl = _both_sides(lambda: R.MscaleStub(C, 3), data, R.Args(do_flip=True), C, ignore, True)
    assert set(ra) == {"pred_05x", "pred_10x", "attn_05x", "predictions", "prob_mask", "err_mask"}
    for k in ("predictions", "err_mask", "pred_05x", "pred_10x"):
        assert np.array_equal(ga[k], ra[k]), k
    assert torch.equal(ga["attn_05x"].cpu(), ra["attn_05x"])
    assert np.array_equal(gh, rh)
    _check_prob(ga["prob_mask"], out, C)
    print("val_loss.avg: device %.8g reference %.8g" % (gl, rl))
    check_close("val_loss", torch.tensor([gl]), torch.tensor([rl]), 1e-5, 1e-5)


def test_eval_minibatch_multi_scale_inference():
    """Not MSCALE, multi_scale_inference with extra scales 0.5 and 2.0, do_flip: six passes, / 3 / 2.  The stub returns
    seeded logits whatever the pixels, so the two sides differ only by the bilinear resize of the 0.5x / 2.0x
    predictions to the input size (CPU interpolate against ssa_bilinear_fwd, held to 1e-5 + 1e-5 |x| by test_bilinear):
    thr = 2 (1e-5 + 1e-5 max|out|).  Integer assets are compared where the top-2 gap of the REFERENCE's averaged logits
    exceeds thr (at most 0.1 % of the pixels may be left out, the histograms may differ by at most two counts per such
    pixel); the probability gets thr on top of its bound (softmax is 1/2-Lipschitz in the sup norm), the loss thr on top
    of its tolerance."""
    C, ignore = 19, 255
    data = R.make_batch(1, 48, 80, C, ignore, seed=21)
    args = R.Args(multi_scale_inference=True, extra_scales="0.5,2.0", do_flip=True)
    ra, rh, ga, gh, out, rl, gl = _both_sides(lambda: R.SeededStub(C, 300), data, args, C, ignore, False)
    assert set(ra) == {"pred_2.0x", "predictions", "prob_mask", "err_mask"} and ra["pred_2.0x"].shape == (1, 96, 160)
    assert np.array_equal(ga["pred_2.0x"], ra["pred_2.0x"])          # no resize on the way: exact
    mx = float(out.abs().max())                 # of the reference's averaged logits
    thr = 2.0 * (1e-5 + 1e-5 * mx)
    top2 = out.topk(2, dim=1)[0]
    sure = ((top2[:, 0] - top2[:, 1]) > thr).numpy()
    left_out = int((~sure).sum())
    print("thr %.3g, smallest top-2 gap %.3g, pixels left out %d of %d" % (
        thr, float((top2[:, 0] - top2[:, 1]).min()), left_out, sure.size))
    assert left_out <= 1e-3 * sure.size
    for k in ("predictions", "err_mask"):
        assert np.array_equal(ga[k][sure], ra[k][sure]), k
    assert np.abs(gh - rh).sum() <= 2 * left_out
    ref_prob = torch.softmax(out.double(), dim=1).max(1)[0]
    err = (ga["prob_mask"].double() - ref_prob).abs()
    print("prob_mask: max abs error %.3g" % float(err.max()))
    assert bool((err <= _prob_bound(C) * ref_prob + thr).all())
    print("val_loss.avg: device %.8g reference %.8g" % (gl, rl))
    assert abs(gl - rl) <= 1e-5 * abs(rl) + thr
