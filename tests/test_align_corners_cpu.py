"""--align_corners (cfg.MODEL.ALIGN_CORNERS = True) at the network level, on the CPU.

  * The oracle (oracle/model.py) with oracle.ops.bilinear / resize_x switched to align_corners=True INSIDE the test
    reproduces tests/golden/aligncorners_golden.pt, which tests/golden/make_golden_aligncorners.py wrote from the real
    reference's ocrnet.HRNet_Mscale with the flag set before any network import -- with the tolerances of
    tests/test_oracle_golden.py's test of the same architecture; the fixture differs from mscale_golden.pt (the same
    weights and batch with the flag off) by far more than those tolerances, so the flag is what is being checked.
  * The configuration accepts the flag (sync_from_reference), and a dry run of the HIP glue with the flag on -- train
    step, backward and evaluation of every architecture, on the harness of tests/test_hip_glue_dryrun_cpu.py -- reaches
    the kernels through the ssa_resize_* entry points only, every call with align_corners = 1."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

from test_hip_glue_dryrun_cpu import ARCHS, _batch, _build, dry  # noqa: F401  (dry: the fixture)
from test_oracle_golden import _load, _oracle_net
from util import check_close

OLD = ("ssa_bilinear_fwd", "ssa_bilinear_bwd", "ssa_bilinear_bwd_x", "ssa_bilinear_bwd_y", "ssa_image_resize_to_nhwc_bf16")
NEW = ("ssa_resize_bilinear_fwd", "ssa_resize_bilinear_bwd", "ssa_resize_bilinear_bwd_x", "ssa_resize_bilinear_bwd_y",
       "ssa_image_resize_to_nhwc")
# position of `int align_corners` in each new entry point's argument list (in front of the stream)
AC_ARG = {"ssa_resize_bilinear_fwd": 12, "ssa_resize_bilinear_bwd": 12, "ssa_resize_bilinear_bwd_x": 9,
          "ssa_resize_bilinear_bwd_y": 9, "ssa_image_resize_to_nhwc": 9}


@pytest.fixture()
def flag_on():
    from semseg_amd.config import cfg
    prev = cfg.MODEL.ALIGN_CORNERS
    cfg.MODEL.ALIGN_CORNERS = True
    try:
        yield cfg
    finally:
        cfg.MODEL.ALIGN_CORNERS = prev


@pytest.fixture()
def oracle_ac(monkeypatch):
    """oracle.ops.bilinear / resize_x under align_corners=True, for one test."""
    from oracle import ops as O
    monkeypatch.setattr(O, "bilinear", lambda x, size: F.interpolate(x, size=size, mode="bilinear", align_corners=True))
    monkeypatch.setattr(O, "resize_x", lambda x, scale_factor: F.interpolate(
        x, scale_factor=scale_factor, mode="bilinear", align_corners=True, recompute_scale_factor=True))
    return O


@pytest.fixture(scope="module")
def gold():
    return _load("aligncorners_golden.pt")


def _unpack(p):
    out, off = {}, 0
    for k, n in zip(p["names"], p["lengths"]):
        out[k] = p["data"][off:off + n]
        off += n
    return out


def _grads(p):
    out = {}
    for k, v in _unpack(p).items():
        n = (v.numel() - 1) // 2
        out[k] = (v[:n].long(), v[n:2 * n].float(), v[2 * n].float())
    return out


def _batch_of(gold):
    """tests/golden/make_golden.py's synth_batch, regenerated from the seed the fixture names."""
    B, H, W, seed = gold["batch"]
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(B, 3, H, W, generator=g)
    blocks = torch.randint(0, 19, (B, (H + 15) // 16, (W + 15) // 16), generator=g)
    gts = blocks.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :H, :W].clone()
    gts[torch.rand(B, H, W, generator=g) < 0.1] = 255
    return images, gts.long()


def test_batch_is_the_fixture_of_the_flag_off_golden(gold):
    old = _load("mscale_golden.pt")
    images, gts = _batch_of(gold)
    assert torch.equal(images, old["images"]) and torch.equal(gts, old["gts"]) and gold["seed"] == old["seed"]
    assert gold["align_corners"] is True


def test_train_step_matches_reference(gold, oracle_ac):
    images, gts = _batch_of(gold)
    net, sd, used = _oracle_net(True, mscale_wt=0.05)
    loss = net.two_scale_forward(images, gts)
    loss.backward()
    assert used == set(sd.keys())
    check_close("train loss", loss.detach().view(1), gold["train_loss"].view(1), 1e-5, 1e-5)
    for name, (idx, vals, norm) in _grads(gold["grads"]).items():
        gflat = sd[name].grad.flatten()
        rel = float((gflat.norm() - norm).abs() / (norm + 1e-12))
        assert rel < 2e-3, (name, rel)
        assert torch.allclose(gflat[idx], vals, rtol=5e-3, atol=1e-6 + 2e-3 * float(vals.abs().max())), name
    bad = [k for k, v in _unpack(gold["running_sample"]).items()
           if not torch.allclose(sd[k].flatten()[:4], v.float(), rtol=1e-3, atol=1e-5)]
    assert len(bad) <= 3, bad   # a few 4-sample BN layers are noise-dominated


def test_eval_matches_reference(gold, oracle_ac):
    """The oracle calibrates its BN statistics as the fixture's generator did (one training-mode pass at momentum 1.0;
    checked against the fixture's samples of the reference's calibrated statistics), then evaluates on them."""
    from oracle.model import Net
    images, gts = _batch_of(gold)
    net, sd, _ = _oracle_net(False)
    with torch.no_grad():
        Net(sd, 19, training=True, bn_momentum=1.0, mscale_wt=0.05).two_scale_forward(images, gts)
    bad = [k for k, v in _unpack(gold["calib_sample"]).items()
           if not torch.allclose(sd[k].flatten()[:4], v.float(), rtol=1e-3, atol=1e-5)]
    assert len(bad) <= 3, bad
    with torch.no_grad():
        o = net.two_scale_forward(images)
    for k, v in gold["eval"].items():
        check_close("eval " + k, o[k][:, :, ::8, ::8], v, 1e-4, 1e-4)
    with torch.no_grad():
        o = net.nscale_forward(images, [0.5, 1.0, 2.0])
    for k, v in gold["eval_nscale"].items():
        check_close("nscale " + k, o[k][:, :, ::8, ::8], v, 1e-4, 1e-4)


def test_fixture_differs_from_the_flag_off_golden(gold):
    """Far outside the tolerances above (1e-5 on the loss, 1e-4 on the eval outputs): the flag decides these numbers."""
    old = _load("mscale_golden.pt")
    dl = abs(float(gold["train_loss"]) - float(old["train_loss"])) / abs(float(old["train_loss"]))
    print("train loss: flag on %.6f, off %.6f (relative difference %.3g)" % (float(gold["train_loss"]), float(old["train_loss"]), dl))
    assert dl > 1e-3
    for k, v in gold["eval"].items():
        d = float((v - old["eval"][k]).abs().max() / old["eval"][k].abs().max())
        print("eval %-9s max difference / max |off| = %.3g" % (k, d))
        assert d > 1e-2, (k, d)
    for k, v in gold["eval_nscale"].items():
        assert float((v - old["eval_nscale"][k]).abs().max() / old["eval_nscale"][k].abs().max()) > 1e-2, k


def test_sync_from_reference_accepts_the_flag():
    """A reference cfg made with --align_corners (config.py:292-293) no longer stops dropin.install()'s configuration sync."""
    from semseg_amd import config
    ref = copy.deepcopy(config._defaults())
    ref.OPTIONS = config.AttrDict(INIT_DECODER=False)
    ref.MODEL.ALIGN_CORNERS = True
    saved = copy.deepcopy(config.cfg)
    try:
        config.sync_from_reference(ref)
        assert config.cfg.MODEL.ALIGN_CORNERS is True
    finally:
        for k in list(config.cfg):
            config.cfg[k] = saved[k]
    assert config.cfg.MODEL.ALIGN_CORNERS is False


def _spy(dry_lib):
    """Record the align_corners argument of every call of a new entry point on the dry library."""
    seen = []
    real = type(dry_lib).__getattr__

    def getattr_(self, name):
        fn = real(self, name)
        if name in AC_ARG:
            def wrapped(*a):
                seen.append((name, a[AC_ARG[name]]))
                return fn(*a)
            return wrapped
        return fn
    return seen, getattr_


@pytest.mark.parametrize("name,crit", ARCHS)
def test_glue_with_the_flag_on_calls_only_the_new_entry_points(name, crit, dry, flag_on, monkeypatch):  # noqa: F811
    seen, getattr_ = _spy(dry)
    monkeypatch.setattr(type(dry), "__getattr__", getattr_)
    flag_on.LOSS.SUPERVISED_MSCALE_WT = 0.05
    net = _build(name, crit).train()
    inputs = _batch()
    loss = net(inputs)
    loss.backward()
    assert not [n for n, p in net.named_parameters() if p.grad is None]
    net.eval()
    with torch.no_grad():
        out = net({"images": inputs["images"]})
    assert tuple(out["pred"].shape) == (2, 19, 64, 96)
    assert not [k for k in OLD if dry.calls[k]], {k: dry.calls[k] for k in OLD}
    assert dry.calls["ssa_resize_bilinear_fwd"] > 0
    assert dry.calls["ssa_resize_bilinear_bwd"] + dry.calls["ssa_resize_bilinear_bwd_x"] > 0
    assert dry.calls["ssa_resize_bilinear_bwd_x"] == dry.calls["ssa_resize_bilinear_bwd_y"]
    assert seen and all(ac == 1 for _, ac in seen), [s for s in seen if s[1] != 1][:5]
    assert {n for n, _ in seen} >= {"ssa_resize_bilinear_fwd", "ssa_resize_bilinear_bwd"}


def test_backward_runs_under_its_forwards_rule(dry, flag_on, monkeypatch):  # noqa: F811
    """The flag is kept in ctx: switched off between forward and backward, the backward still passes 1; the eval tail's
    resize_tensor reads the flag when called."""
    import importlib
    from semseg_amd import hip_backend as hb
    seen, getattr_ = _spy(dry)
    monkeypatch.setattr(type(dry), "__getattr__", getattr_)
    from semseg_amd import ops
    x = torch.zeros(2, 5, 7, 48, dtype=hb.ACT_DTYPE, requires_grad=True)
    y = ops.backend().bilinear(x, (17, 25))
    flag_on.MODEL.ALIGN_CORNERS = False
    y.backward(torch.zeros_like(y))
    assert [ac for _, ac in seen] == [1, 1, 1] and [n for n, _ in seen] == [
        "ssa_resize_bilinear_fwd", "ssa_resize_bilinear_bwd_x", "ssa_resize_bilinear_bwd_y"]
    del seen[:]
    eval_tail = importlib.import_module("semseg_amd.utils.eval_tail")
    eval_tail.resize_tensor(torch.zeros(1, 19, 8, 8), (16, 16))
    flag_on.MODEL.ALIGN_CORNERS = True
    eval_tail.resize_tensor(torch.zeros(1, 19, 8, 8), (16, 16))
    assert seen == [("ssa_resize_bilinear_fwd", 0), ("ssa_resize_bilinear_fwd", 1)]
