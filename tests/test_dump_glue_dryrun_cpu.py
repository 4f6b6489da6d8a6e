"""semseg_amd.utils.dumper.ImageDumper without a GPU: the kernels run from the library of emu_util.emu_backend() on CPU
tensors and are never launched on a device.  Host assets (what the reference's eval_minibatch returns) and device-form
assets (eval_minibatch(assets_on_device=True)), in the three modes, against the files tests/dump_ref.py describes for the
same inputs; the launch and synchronisation counts; the dump-frequency and rank rules; the web page; the drop-in
registration; and eval_minibatch's default path left as it was."""
import importlib
import inspect
import io
import os
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

import dump_cases as K
import dump_ref as R

MODES = {"visual": dict(dump_assets=True), "submission": dict(dump_for_submission=True),
         "auto_labelling": dict(dump_for_auto_labelling=True)}
# launches per dumped image of the golden case: one ssa_dump_tail for everything at the image's size (the bytes of
# prob_mask and err_mask ride in it), one ssa_mask_u8 for attn_0.5x; pred_0.5x travels as the index bytes it is
LAUNCHES = {"visual": 2, "submission": 1, "auto_labelling": 1}


@pytest.fixture()
def env(tmp_path, monkeypatch):
    from emu_util import emu_backend
    from semseg_amd.config import cfg
    from semseg_amd.utils import dumper
    eval_tail = importlib.import_module("semseg_amd.utils.eval_tail")
    z, meta = R.load_golden()
    monkeypatch.setitem(cfg, "DATASET_INST", R.golden_dataset(meta))
    monkeypatch.setitem(cfg, "GLOBAL_RANK", 0)
    monkeypatch.setitem(cfg, "RESULT_DIR", str(tmp_path))
    monkeypatch.setitem(cfg.DATASET, "MEAN", meta["mean"])
    monkeypatch.setitem(cfg.DATASET, "STD", meta["std"])
    monkeypatch.setattr(dumper, "_default_device", lambda: torch.device("cpu"))
    monkeypatch.delitem(sys.modules, "config", raising=False)
    trips = []
    real = eval_tail._to_host
    monkeypatch.setattr(eval_tail, "_to_host", lambda ts: (trips.append(sum(t.numel() * t.element_size() for t in ts)),
                                                           real(ts))[1])
    with emu_backend():
        from semseg_amd import _lib
        yield types.SimpleNamespace(z=z, meta=meta, cfg=cfg, dumper=dumper, trips=trips, tmp=tmp_path,
                                    launches=lambda: _lib.lib().ssa_launch_count(0))


def _expected_bytes(entry):
    """The file Pillow writes for an entry of dump_ref: the bytes the dumper's own write must equal."""
    buf = io.BytesIO()
    if entry[0] == "P":
        im = Image.fromarray(entry[1]).convert("P")
        im.putpalette(list(entry[2]))
    else:
        im = Image.fromarray(entry[1])
    im.save(buf, format="PNG")
    return buf.getvalue()


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("mode", list(MODES))
def test_dump_writes_what_the_restatement_describes(env, mode, form):
    ds = env.cfg.DATASET_INST
    d = env.dumper.ImageDumper(val_len=100, tensorboard=False, **MODES[mode])
    dd = R.golden_dump_dict(env.z, env.meta)
    want = R.dump(R.golden_dump_dict(env.z, env.meta), 0, ds, env.meta["mean"], env.meta["std"], **MODES[mode])
    if form == "device":
        dd = K.device_form(dd, "cpu")
    before = env.launches()
    d.dump(dd, 0)
    assert env.launches() - before == LAUNCHES[mode]
    assert len(env.trips) == 1                                   # one trip back, one synchronisation
    H, W = env.z["gt_images"].shape[1:]
    if mode != "visual":
        assert env.trips[0] <= (2 if mode == "auto_labelling" else 1) * (H * W + 15)
    assert "predictions" not in dd["assets"]
    assert d.save_dir == str(env.tmp / {"visual": "best_images", "submission": "submit", "auto_labelling": ""}[mode]
                             ).rstrip("/")
    assert sorted(f for f in os.listdir(d.save_dir) if f.endswith(".png")) == sorted(want)
    golden = R.golden_files(env.z, env.meta, mode)
    for fn, entry in want.items():
        path = os.path.join(d.save_dir, fn)
        assert R.same(R.decode(path), entry), (mode, fn)
        assert R.same(entry, golden[fn]), (mode, fn)
        with open(path, "rb") as fh:
            assert fh.read() == _expected_bytes(entry), (mode, fn)      # byte-identical to a Pillow write of the same
    if mode == "visual":
        order = [a for a in env.meta["asset_order"] if a != "predictions"]
        assert d.imgs_to_webpage == [R.webpage_rows(env.meta["img_names"], order, d.save_dir, True)]
        assert d.imgs_to_tensorboard == []
        d.write_summaries(True)
        page = open(os.path.join(d.save_dir, "index.html")).read()
        assert page.startswith("<!DOCTYPE html>\n<html>\n  <head>\n    <title>Experiment = prediction examples</title>")
        assert page.count("<td halign") == 6 and page.endswith("  </body>\n</html>")
        d.reset()
        assert d.imgs_to_webpage == []
    else:
        assert d.imgs_to_webpage == []


def test_dump_frequency_and_rank_rules(env):
    name = env.meta["img_names"][0]

    def run(rank=0, **kw):
        env.cfg["GLOBAL_RANK"] = rank
        env.cfg["RESULT_DIR"] = str(env.tmp / ("r%d_%s" % (rank, "_".join(sorted(kw)))))
        d = env.dumper.ImageDumper(val_len=100, tensorboard=False, **kw)
        wrote = []
        for val_idx in range(25):
            dd = R.golden_dump_dict(env.z, env.meta)
            dd["img_names"] = ["%s_%02d" % (name, val_idx), "other"]
            had = "predictions" in dd["assets"]
            d.dump(dd, val_idx)
            if any(f.startswith("%s_%02d" % (name, val_idx)) for f in os.listdir(d.save_dir)):
                wrote.append(val_idx)
                assert had and "predictions" not in dd["assets"]
            else:
                assert "predictions" in dd["assets"]             # the early return touches nothing
        return d, wrote

    d, wrote = run()
    assert (d.viz_frequency, d.dump_frequency) == (10, 10) and wrote == [0, 10, 20] and len(d.imgs_to_webpage) == 3
    d, wrote = run(dump_all_images=True, dump_assets=True)
    assert (d.viz_frequency, d.dump_frequency) == (10, 1) and wrote == list(range(25)) and len(d.imgs_to_webpage) == 3
    files = os.listdir(d.save_dir)                               # assets only for the visualised ones
    assert sorted(f for f in files if "attn_" in f) == ["%s_%02d_attn_0.5x.png" % (name, i) for i in (0, 10, 20)]
    assert len([f for f in files if f.startswith("composited_")]) == 25
    d, wrote = run(rank=1, dump_all_images=True)
    assert wrote == [] and d.imgs_to_webpage == []
    d, wrote = run(rank=1, dump_for_submission=True)             # the labelling modes dump every image on every rank
    assert wrote == list(range(25))
    d = env.dumper.ImageDumper(val_len=5, dump_num=10)
    assert (d.viz_frequency, d.dump_frequency) == (1, 1)


def test_constructor_signature_is_the_references():
    from semseg_amd.utils import dumper
    sig = inspect.signature(dumper.ImageDumper.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("val_len", inspect.Parameter.empty), ("tensorboard", True), ("write_webpage", True),
        ("webpage_fn", "index.html"), ("dump_all_images", False), ("dump_assets", False), ("dump_err_prob", False),
        ("dump_num", 10), ("dump_for_auto_labelling", False), ("dump_for_submission", False)]
    for m in ("dump", "reset", "write_summaries"):
        assert callable(getattr(dumper.ImageDumper, m))


def test_dropin_registers_the_class_and_the_device_assets_switch(monkeypatch):
    import semseg_amd.dropin as dropin
    from semseg_amd.utils import dumper
    eval_tail = importlib.import_module("semseg_amd.utils.eval_tail")
    misc = types.ModuleType("utils.misc")
    misc.ImageDumper = misc.AverageMeter = object()
    utils_pkg = types.ModuleType("utils")
    utils_pkg.misc = misc
    for k in list(sys.modules):
        if k in ("apex", "apex.amp", "apex.parallel", "utils.trnval_utils") or k.startswith(("network.", "loss.")):
            monkeypatch.delitem(sys.modules, k)
    monkeypatch.setitem(sys.modules, "utils", utils_pkg)
    monkeypatch.setitem(sys.modules, "utils.misc", misc)
    monkeypatch.setattr(eval_tail, "_SYNC_CFG", [False])
    assert inspect.signature(dropin.install).parameters["device_dumper"].default is False
    dropin.install(replace_apex=False, device_eval_tail=True)
    assert misc.ImageDumper is misc.AverageMeter                 # off by default
    assert sys.modules["utils.trnval_utils"].eval_minibatch is eval_tail.eval_minibatch
    dropin.install(replace_apex=False, device_dumper=True)
    assert misc.ImageDumper is dumper.ImageDumper and misc.AverageMeter is not dumper.ImageDumper
    em = sys.modules["utils.trnval_utils"].eval_minibatch
    assert em.func is eval_tail.eval_minibatch and em.keywords == {"assets_on_device": True}
    for k in list(sys.modules):                                  # what install() registered goes with the test
        if k == "utils.trnval_utils" or k.startswith(("network.", "loss.")):
            monkeypatch.delitem(sys.modules, k, raising=False)


class _Net(torch.nn.Module):
    """Three 1x1 mixes of the image as 19 logits, returned the way the package's networks return them, with an attention
    map and a scale's own prediction at half size."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.w = torch.nn.Parameter(torch.randn(19, 3, generator=g))

    def forward(self, inputs):
        x = inputs["images"]
        pred = torch.einsum("kc,bchw->bkhw", self.w, x).contiguous()
        return {"pred": pred, "pred_0.5x": pred[:, :, ::2, ::2].contiguous(), "attn_0.5x": torch.sigmoid(x[:, :1, ::2, ::2])}


def test_eval_minibatch_default_path_is_unchanged_and_the_device_form_holds_the_same(env, monkeypatch):
    import collections
    eval_tail = importlib.import_module("semseg_amd.utils.eval_tail")
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: collections.namedtuple("S", "cuda_stream")(0))
    assert inspect.signature(eval_tail.eval_minibatch).parameters["assets_on_device"].default is False
    env.cfg.MODEL.MSCALE = True
    args = types.SimpleNamespace(default_scale=1.0, multi_scale_inference=False, extra_scales="", do_flip=False)
    images = torch.from_numpy(env.z["input_images"].copy())
    gts = torch.from_numpy(env.z["gt_images"].copy())
    data = (images, gts, env.meta["img_names"], 1.0)
    net = _Net()

    class Loss:
        def __init__(self):
            self.seen = []

        def update(self, v, n):
            self.seen.append((v, n))

    try:
        la, lb = Loss(), Loss()
        crit = torch.nn.CrossEntropyLoss(ignore_index=255)
        host, hist = eval_tail.eval_minibatch(data, net, crit, la, True, args, 0)
        dev, hist_d = eval_tail.eval_minibatch(data, net, crit, lb, True, args, 0, assets_on_device=True)
    finally:
        env.cfg.MODEL.MSCALE = False
    # the default path: the reference's types, key for key
    assert list(host) == ["pred_0.5x", "attn_0.5x", "predictions", "prob_mask", "err_mask"]
    assert isinstance(host["predictions"], np.ndarray) and host["predictions"].dtype == np.int64
    assert isinstance(host["pred_0.5x"], np.ndarray) and host["pred_0.5x"].dtype == np.int64
    assert isinstance(host["err_mask"], np.ndarray) and host["err_mask"].dtype == np.dtype(int)
    assert isinstance(host["prob_mask"], torch.Tensor) and host["prob_mask"].dtype == torch.float32
    logits = net({"images": images})["pred"]
    assert np.array_equal(host["predictions"], logits.argmax(1).numpy())
    assert np.array_equal(hist, hist_d) and hist.dtype == np.int64 and la.seen == lb.seen and len(la.seen) == 1
    # the device form: the same values where the tail wrote them, and the uploaded batch
    assert list(dev) == ["pred_0.5x", "attn_0.5x", "predictions", "prob_mask", "err_mask", "input_images", "gt_images"]
    for k in ("predictions", "pred_0.5x", "err_mask"):
        assert dev[k].dtype == torch.uint8 and np.array_equal(dev[k].numpy().astype(np.int64), host[k]), k
    assert torch.equal(dev["prob_mask"], host["prob_mask"]) and dev["attn_0.5x"].dtype == torch.float32
    assert torch.equal(dev["input_images"], images) and torch.equal(dev["gt_images"], gts)
    # and the dumper writes the same files from either
    out = {}
    for form, assets in (("host", host), ("device", dev)):
        env.cfg["RESULT_DIR"] = str(env.tmp / form)
        d = env.dumper.ImageDumper(val_len=100, dump_assets=True)
        d.dump({"gt_images": gts, "input_images": images, "img_names": env.meta["img_names"], "assets": assets}, 0)
        out[form] = {f: open(os.path.join(d.save_dir, f), "rb").read() for f in sorted(os.listdir(d.save_dir))}
    assert out["host"] == out["device"] and len(out["host"]) == 8
