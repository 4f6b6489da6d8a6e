"""The restatement of ImageDumper.dump the dump-tail kernels are held to (tests/dump_ref.py), against what it restates:
the files the REAL reference wrote (tests/golden/dump_golden.npz, made by tests/golden/make_golden_dump.py) and, line by
line, the live Pillow and torch of this machine.  No kernel runs here."""
import numpy as np
import torch
from PIL import Image

import dump_cases as K
import dump_ref as R

MODES = {"visual": dict(dump_assets=True), "submission": dict(dump_for_submission=True),
         "auto_labelling": dict(dump_for_auto_labelling=True)}


def test_restatement_equals_the_reference_files():
    z, meta = R.load_golden()
    ds = R.golden_dataset(meta)
    assert set(meta["files"]) == set(MODES)
    for mode, kw in MODES.items():
        dd = R.golden_dump_dict(z, meta)
        got = R.dump(dd, 0, ds, meta["mean"], meta["std"], val_len=meta["val_len"], **kw)
        want = R.golden_files(z, meta, mode)
        assert "predictions" not in dd["assets"]
        assert sorted(got) == sorted(want), mode
        for fn in want:
            assert R.same(got[fn], want[fn]), (mode, fn)
    assert len(meta["files"]["visual"]) == 8 and len(meta["files"]["auto_labelling"]) == 2
    assert [fn for fn, _ in meta["webpage"][0]] == [
        fn if "/" not in fn else fn.split("/")[-1] for fn, _ in R.webpage_rows(
            meta["img_names"], [a for a in meta["asset_order"] if a != "predictions"], "", True)]


def test_blend_line_equals_live_pillow_on_all_byte_pairs():
    a = np.repeat(np.arange(256, dtype=np.uint8).reshape(256, 1), 256, 1)
    b = np.ascontiguousarray(a.T)
    live = np.array(Image.blend(Image.fromarray(a), Image.fromarray(b), 0.4))
    assert np.array_equal(R.blend_bytes(a, b, 0.4), live)
    rgb_a, rgb_b = np.stack([a] * 3, -1), np.stack([b, b[::-1], b[:, ::-1]], -1)
    live = np.array(Image.blend(Image.fromarray(rgb_a), Image.fromarray(rgb_b), 0.4))
    assert np.array_equal(R.blend_bytes(rgb_a, rgb_b, 0.4), live)
    # the same expression in fp64 is NOT Pillow's
    f64 = (a.astype(np.float64) + float(np.float32(0.4)) * (b.astype(np.float64) - a)).astype(np.uint8)
    assert (f64 != live[..., 0]).sum() > 1000


def test_denormalise_line_equals_torch_on_every_byte():
    x = K.all_bytes_image()
    inv_mean, inv_std = R.inv_norm(K.MEAN, K.STD)
    t = torch.from_numpy(x.copy())
    t.sub_(torch.as_tensor([-m / s for m, s in zip(K.MEAN, K.STD)], dtype=torch.float32).view(3, 1, 1))
    t.div_(torch.as_tensor([1 / s for s in K.STD], dtype=torch.float32).view(3, 1, 1))
    live = t.mul(255).byte().permute(1, 2, 0).numpy()
    got = R.denorm_bytes(x, inv_mean, inv_std)
    assert np.array_equal(got, live)
    ident = np.arange(256, dtype=np.uint8)
    assert got[0, 1, 0] == 0                                    # byte 1 on channel 0 comes back as 0
    assert (np.abs(got[0].astype(int) - ident[:, None]) <= 1).all() and (got[0] != ident[:, None]).any()


def test_mask_line_at_every_byte_boundary():
    v = K.mask_values()
    got = R.mask_bytes(v)
    finite = np.isfinite(v) & (v >= 0) & (v * np.float32(255) < 256)
    live = (torch.from_numpy(v[finite]) * 255).numpy().astype(np.uint8)          # (mask * 255).astype(np.uint8)
    assert np.array_equal(got[finite], live)
    assert np.array_equal(got[finite], (v[finite] * 255).astype(np.uint8))
    k = np.arange(256)
    assert got[256 + 255] == 254 and got[255] == 255 and got[0] == 0           # just below 1, 1, 0
    assert set(got[:256].astype(int) - k) <= {0, -1}
    tail = got[768:]
    assert list(tail) == [0, 255, 254, 0, 0, 255, 255, 0, 0, 255, 0]


def test_palette_table_for_cityscapes_and_a_short_palette():
    z, meta = R.load_golden()
    ds = R.golden_dataset(meta)
    pal = R.palette_table(ds.colorize_mask)
    assert pal.shape == (256, 3) and pal.dtype == np.uint8
    assert np.array_equal(pal.reshape(-1), np.array(meta["color_mapping"], np.uint8))
    assert tuple(pal[0]) == (128, 64, 128) and tuple(pal[18]) == (119, 11, 32) and not pal[19:].any()
    short = R.Dataset([255, 0, 0, 0, 255, 0, 0, 0, 255], {})
    pal3 = R.palette_table(short.colorize_mask)
    assert np.array_equal(pal3[:3], np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)) and not pal3[3:].any()
    img = np.array([[0, 1, 2, 3, 200, 255]], np.uint8)
    assert np.array_equal(np.array(short.colorize_mask(img).convert("RGB")), pal3[img])
    from semseg_amd.utils import dumper
    assert np.array_equal(dumper.palette_table(ds.colorize_mask), pal)
    assert np.array_equal(dumper.palette_table(short.colorize_mask), pal3)


def test_id_table_equals_the_reference_loop():
    z, meta = R.load_golden()
    ds = R.golden_dataset(meta)
    lut = R.id_table(ds.id_to_trainid)
    prediction = np.array([list(range(19)) + [255], [255] + list(range(18, -1, -1))], np.int64)
    label_out = np.zeros_like(prediction)
    for label_id, train_id in ds.id_to_trainid.items():
        label_out[np.where(prediction == train_id)] = label_id
    assert np.array_equal(lut[prediction], label_out)
    assert lut[0] == 7 and lut[18] == 33 and lut[255] == 30 and lut[19] == 0     # later entries win: 255 -> trailer
    assert np.array_equal(R.id_table({300: 1, 5: 2, -1: -1, 9: 700}), np.eye(1, 256, 1, dtype=np.uint8)[0] * 255
                          + np.eye(1, 256, 2, dtype=np.uint8)[0] * 5)
    from semseg_amd.utils import dumper
    assert np.array_equal(dumper.id_table(ds.id_to_trainid), lut)


def test_dump_rules_of_frequency_and_rank():
    writes = [i for i in range(25) if R.dumps(i, 100)[0]]
    assert writes == [0, 10, 20]
    assert [i for i in range(25) if R.dumps(i, 100, dump_all_images=True)[0]] == list(range(25))
    assert [i for i in range(25) if R.dumps(i, 100, dump_all_images=True)[1]] == [0, 10, 20]
    assert not any(R.dumps(i, 100, dump_all_images=True, global_rank=1)[0] for i in range(25))
    assert all(R.dumps(i, 100, global_rank=1, labelling=True)[0] for i in range(25))
