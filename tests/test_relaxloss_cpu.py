"""The label relaxation (--jointwtborder) without a GPU and without the kernels: the restatement the kernel tests use
(tests/relaxloss_ref.py) against the golden data recorded from the REAL reference (tests/golden/relaxloss_golden.pt,
cases 1-7 of tests/relaxloss_cases.py), and the public surface -- get_loss, the reduced-border refusal, the
configuration sync.

Tolerances: check_close(loss, 1e-5, 1e-5) and (gradient, 1e-4, 1e-4), what tests/test_kernels_gpu.py holds the cross
entropy to.  The reference's own fp32 result sits ~3e-8 (loss) and 2-3e-7 of max|g| (gradient) from this fp64 restatement."""
import types

import numpy as np
import pytest
import torch

import relaxloss_cases as K
import relaxloss_ref as R
from util import check_close


@pytest.mark.parametrize("n", K.GOLDEN_CASES)
def test_restatement_equals_the_reference(n):
    k, ref = K.CASES[n], K.reference(n)
    mh = R.multihot(ref["labels"].numpy(), k["C"], k["ignore"], k["border"], k["strict"])
    assert np.array_equal(mh, ref["mh"].numpy())
    w = R.class_weights(mh, k["ub"], k["batch"])
    assert w.dtype == torch.float32 and torch.equal(w.view(torch.int32), ref["w"].view(torch.int32))
    x = ref["logits"].double().requires_grad_(True)
    loss = R.loss(x, mh, k["ub"], k["batch"])
    (loss * k["up"]).backward()
    check_close("relax loss case %d" % n, loss.detach().reshape(1), ref["loss"].reshape(1), 1e-5, 1e-5)
    check_close("relax grad case %d" % n, x.grad, ref["grad"], 1e-4, 1e-4)


def test_cases_have_pixels_without_a_class_and_wide_sets():
    for n in K.CASES:
        ref = K.reference(n)
        assert int(ref["stats"][:, -1].min()) >= 6, n
        assert int(ref["mh"][:, :-1].sum(1).max()) >= 3, n
    s7 = K.reference(7)
    assert int(s7["stats"][0, -1]) == 9 * 11 and bool((s7["w"][0] == 1).all()) and float(s7["grad"][0].abs().max()) == 0.0
    sets = K.reference(5)["sets"]
    assert bool((sets[..., 1] != 0).any()) and bool((sets[..., 0] != 0).any())      # 65 classes need both words


def test_get_loss_builds_the_relaxation_criterion():
    from semseg_amd.loss import ImgWtLossSoftNLL, CrossEntropyLoss2d, get_loss
    from semseg_amd.loss import criteria
    crit, val = get_loss(types.SimpleNamespace(jointwtborder=True, wt_bound=0.5))
    assert isinstance(crit, ImgWtLossSoftNLL) and crit.upper_bound == 0.5 and isinstance(val, CrossEntropyLoss2d)
    assert crit.num_classes == criteria.cfg.DATASET.NUM_CLASSES and crit.ignore_index == criteria.cfg.DATASET.IGNORE_LABEL
    crit, _ = get_loss(types.SimpleNamespace(jointwtborder=True))
    assert crit.upper_bound == 1.0
    with pytest.raises(NotImplementedError, match="img_wt_loss") as e:
        get_loss(types.SimpleNamespace(img_wt_loss=True))
    assert "jointwtborder" not in str(e.value) and "rmi" not in str(e.value)
    with pytest.raises(AssertionError):
        ImgWtLossSoftNLL(19, norm=True)


def test_reduced_border_mode_is_refused(monkeypatch):
    from semseg_amd.config import cfg
    from semseg_amd.datasets.transforms import RelaxedBoundaryLossToTensor
    from semseg_amd.loss import ImgWtLossSoftNLL
    monkeypatch.setitem(cfg, "REDUCE_BORDER_EPOCH", 3)
    monkeypatch.setitem(cfg, "EPOCH", 4)
    with pytest.raises(NotImplementedError, match="rlx_off_epoch"):
        ImgWtLossSoftNLL(19)(torch.zeros(1, 19, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="rlx_off_epoch"):
        RelaxedBoundaryLossToTensor(255, 19)(torch.zeros(4, 4, dtype=torch.uint8))
    # before that epoch both go on to the library
    monkeypatch.setitem(cfg, "EPOCH", 3)
    import semseg_amd.loss.criteria as criteria
    assert not criteria._reduced_border()


def test_config_defaults_and_sync():
    from semseg_amd import config
    d = config._defaults()
    assert (d.BORDER_WINDOW, d.STRICTBORDERCLASS, d.BATCH_WEIGHTING, d.EPOCH) == (1, None, False, 0)
    NS = types.SimpleNamespace
    model = NS(OCR=NS(MID_CHANNELS=512, KEY_CHANNELS=256), ALIGN_CORNERS=False)
    ref = NS(MODEL=model, LOSS=NS(OCR_ALPHA=0.4, OCR_AUX_RMI=False, SUPERVISED_MSCALE_WT=0),
             DATASET=NS(NUM_CLASSES=19, IGNORE_LABEL=255), OPTIONS=NS(INIT_DECODER=False),
             BORDER_WINDOW=2, STRICTBORDERCLASS=[3, 7], BATCH_WEIGHTING=True, EPOCH=5, REDUCE_BORDER_EPOCH=-1)
    saved = dict(config.cfg)
    try:
        config.sync_from_reference(ref)
        c = config.cfg
        assert (c.BORDER_WINDOW, c.STRICTBORDERCLASS, c.BATCH_WEIGHTING, c.EPOCH) == (2, [3, 7], True, 5)
        bare = NS(MODEL=model, LOSS=ref.LOSS, DATASET=ref.DATASET, OPTIONS=ref.OPTIONS)
        config.sync_from_reference(bare)
        assert (c.BORDER_WINDOW, c.STRICTBORDERCLASS, c.BATCH_WEIGHTING, c.EPOCH) == (1, None, False, 0)
    finally:
        config.cfg.clear()
        config.cfg.update(saved)
