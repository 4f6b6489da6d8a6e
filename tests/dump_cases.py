"""The cases the dump-tail kernels (csrc/dump_tail.hip) are held to, shared by tests/test_dump_emu_cpu.py (the CPU
emulation of both storage builds) and tests/test_dump_gpu.py (the device): every function runs the kernels through the C
ABI of the library handle `L` on torch tensors of `dev` and compares every output byte with tests/dump_ref.py.  Each
returns the number of output planes it compared."""
import ctypes

import numpy as np
import torch

import dump_ref as R

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
OUTS = ("input_rgb", "gt_rgb", "pred_rgb", "comp_rgb", "label_ids", "prob_u8", "err_u8")
SHAPES = ((37, 53), (64, 128), (1, 4099))        # odd everywhere and under one workgroup's span; even; one row, tail of 3


def _sync(dev):
    if str(dev).startswith("cuda"):
        torch.cuda.synchronize()


def first_difference(got, want):
    d = np.argwhere(got != want)
    i = tuple(d[0])
    return "%d of %d differ, first at %s: got %s want %s" % (len(d), got.size, i, got[i], want[i])


def tables():
    z, meta = R.load_golden()
    ds = R.golden_dataset(meta)
    return R.palette_table(ds.colorize_mask), R.id_table(ds.id_to_trainid)


def identity_tables():
    g = np.arange(256, dtype=np.uint8)
    return np.ascontiguousarray(np.stack([g, g, g], 1)), np.ascontiguousarray(g[::-1])


def random_inputs(H, W, seed, hostile=True):
    """A normalised random byte image, labels, predictions over every byte, a probability and an error mask; `hostile`
    sprinkles what the reference leaves undefined (values outside [0, 256) after the scaling, NaN, infinities), labels
    beyond a byte and negative ones (the low 8 bits count)."""
    rng = np.random.RandomState(seed)
    u8 = rng.randint(0, 256, (3, H, W)).astype(np.uint8)
    x = torch.from_numpy(u8).float().div(255).sub(torch.tensor(MEAN).view(3, 1, 1)).div(torch.tensor(STD).view(3, 1, 1))
    x = x.numpy().copy()
    gts = rng.randint(0, 19, (H, W)).astype(np.int64)
    gts[rng.rand(H, W) < 0.15] = 255
    pred = rng.randint(0, 256, (H, W)).astype(np.uint8)
    pred[rng.rand(H, W) < 0.7] %= 19
    prob = rng.rand(H, W).astype(np.float32)
    err = (rng.rand(H, W) < 0.3).astype(np.uint8)
    flat = prob.reshape(-1)
    flat[:3] = (0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)))
    if hostile:
        n = H * W
        k = rng.choice(n, size=min(n, 12), replace=False)
        xs = x.reshape(3, -1)
        xs[0, k[0]], xs[1, k[1]], xs[2, k[2]] = np.nan, np.inf, -np.inf
        xs[0, k[3]], xs[1, k[4]], xs[2, k[5]] = 40.0, -40.0, 3.0e38
        flat[k[6]], flat[k[7]], flat[k[8]], flat[k[9]] = np.nan, -0.5, 7.0, np.inf
        g = gts.reshape(-1)
        g[k[10]], g[k[11]] = 256 + 7, -1
    return x, gts, pred, prob, err


def expected(x, gts, pred, prob, err, pal, ids, alpha=R.ALPHA):
    inv_mean, inv_std = R.inv_norm(MEAN, STD)
    rgb = R.denorm_bytes(x, inv_mean, inv_std)
    prgb = pal[pred]
    return {"input_rgb": rgb, "gt_rgb": pal[(gts & 255).astype(np.uint8)], "pred_rgb": prgb,
            "comp_rgb": R.blend_bytes(rgb, prgb, alpha), "label_ids": ids[pred], "prob_u8": R.mask_bytes(prob),
            "err_u8": R.err_bytes(err)}


def _offset(t, dev, shift):
    """t on dev, as a view that starts `shift` elements into a larger buffer (shift = 1 misses every wide alignment)."""
    flat = torch.zeros(t.numel() + shift, dtype=t.dtype, device=dev)
    v = flat[shift:].view(t.shape)
    v.copy_(t)
    return v


def run_dump_tail(L, dev, x, gts, pred, prob, err, pal, ids, want=OUTS, alpha=R.ALPHA, shift=0, mean_std=(MEAN, STD),
                  shape=None):
    """One ssa_dump_tail with the outputs named in `want` (an input that is None goes in as a null pointer); returns
    {name: ndarray} after checking the guard bytes around every output."""
    H, W = shape or pred.shape
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    up = lambda a: None if a is None else _offset(torch.from_numpy(np.ascontiguousarray(a)), dev, shift)   # noqa: E731
    d = {k: up(v) for k, v in dict(x=x, gts=gts, pred=pred, prob=prob, err=err, pal=pal, ids=ids).items()}
    outs = {}
    for k in want:
        shape = (H, W, 3) if k.endswith("_rgb") else (H, W)
        guard = torch.full((int(np.prod(shape)) + shift + 16,), 0xA5, dtype=torch.uint8, device=dev)
        outs[k] = guard
    view = {k: g[shift:g.numel() - 16] for k, g in outs.items()}
    inv_mean, inv_std = R.inv_norm(*mean_std)
    im = (ctypes.c_float * 3)(*inv_mean.tolist())
    isd = (ctypes.c_float * 3)(*inv_std.tolist())
    rc = L.ssa_dump_tail(P(d["x"]), H * W, im, isd, P(d["gts"]), P(d["pred"]), P(d["pal"]), P(d["ids"]), P(d["prob"]),
                         P(d["err"]), alpha, H, W, *[P(view.get(k)) for k in OUTS], None)
    assert rc == 0, rc
    _sync(dev)
    got = {}
    for k, g in outs.items():
        h = g.cpu().numpy()
        assert (h[:shift] == 0xA5).all() and (h[-16:] == 0xA5).all(), "%s: written outside the output" % k
        got[k] = h[shift:-16].reshape((H, W, 3) if k.endswith("_rgb") else (H, W))
    return got


def compare(got, exp):
    for k, g in got.items():
        assert g.dtype == np.uint8 and np.array_equal(g, exp[k]), "%s: %s" % (k, first_difference(g, exp[k]))
    return len(got)


def check_shapes_all_outputs(L, dev, shapes=SHAPES):
    pal, ids = tables()
    n = 0
    for s, (H, W) in enumerate(shapes):
        inp = random_inputs(H, W, 100 + s)
        n += compare(run_dump_tail(L, dev, *inp, pal, ids), expected(*inp, pal, ids))
    return n


def check_subsets_of_outputs(L, dev, shape=(37, 53)):
    """Each subset with ONLY the inputs it is made from (the others null): nothing else is read or written."""
    pal, ids = tables()
    x, gts, pred, prob, err = random_inputs(*shape, 7)
    exp = expected(x, gts, pred, prob, err, pal, ids)
    n = 0
    for want, kw in ((("comp_rgb",), dict(x=x, pred=pred, pal=pal)),
                     (("label_ids", "prob_u8"), dict(pred=pred, ids=ids, prob=prob)),
                     (("label_ids",), dict(pred=pred, ids=ids)),
                     (("gt_rgb",), dict(gts=gts, pal=pal)),
                     (("pred_rgb",), dict(pred=pred, pal=pal)),
                     (("input_rgb", "err_u8"), dict(x=x, err=err)),
                     (("prob_u8", "err_u8"), dict(prob=prob, err=err))):
        full = dict(x=None, gts=None, pred=None, prob=None, err=None, pal=None, ids=None)
        full.update(kw)
        got = run_dump_tail(L, dev, *[full[k] for k in ("x", "gts", "pred", "prob", "err", "pal", "ids")], want=want,
                            shape=shape)
        n += compare(got, exp)
    return n


def check_unaligned_pointers(L, dev, shapes=((37, 53), (1, 4099))):
    """Every tensor one element into its buffer: the pixel-by-pixel path, same bytes."""
    pal, ids = tables()
    n = 0
    for s, (H, W) in enumerate(shapes):
        inp = random_inputs(H, W, 200 + s)
        n += compare(run_dump_tail(L, dev, *inp, pal, ids, shift=1), expected(*inp, pal, ids))
    return n


def all_pairs_inputs():
    """The 256 x 256 image of all byte pairs: the input de-normalises to byte a = row (mean 0, std 1: (a + 0.5) / 255
    scales back into [a, a + 1)), the prediction is b = column under a grey identity palette."""
    a = np.repeat(np.arange(256, dtype=np.float32).reshape(256, 1), 256, 1)
    x = np.ascontiguousarray(np.stack([(a + np.float32(0.5)) / np.float32(255)] * 3)).astype(np.float32)
    pred = np.ascontiguousarray(np.repeat(np.arange(256, dtype=np.uint8).reshape(1, 256), 256, 0))
    return x, pred


def check_all_pairs_blend(L, dev):
    from PIL import Image
    pal, ids = identity_tables()
    x, pred = all_pairs_inputs()
    got = run_dump_tail(L, dev, x, None, pred, None, None, pal, None, want=("input_rgb", "pred_rgb", "comp_rgb"),
                        mean_std=([0.0, 0.0, 0.0], [1.0, 1.0, 1.0]))
    a = np.repeat(np.arange(256, dtype=np.uint8).reshape(256, 1), 256, 1)
    assert np.array_equal(got["input_rgb"], np.stack([a] * 3, -1)) and np.array_equal(got["pred_rgb"], pal[pred])
    live = np.array(Image.blend(Image.fromarray(got["input_rgb"]), Image.fromarray(got["pred_rgb"]), 0.4))
    assert np.array_equal(got["comp_rgb"], live), first_difference(got["comp_rgb"], live)
    assert np.array_equal(got["comp_rgb"], R.blend_bytes(got["input_rgb"], got["pred_rgb"]))
    return 3


def all_bytes_image():
    """Every byte on each ImageNet channel as the loader normalises it (ToTensor, Normalize): fp32 [3][1][256]."""
    b = torch.arange(256, dtype=torch.float32).div(255).view(1, 1, 256).repeat(3, 1, 1)
    return b.sub(torch.tensor(MEAN).view(3, 1, 1)).div(torch.tensor(STD).view(3, 1, 1)).numpy().copy()


def check_all_bytes_denormalise(L, dev):
    x = all_bytes_image()
    got = run_dump_tail(L, dev, x, None, None, None, None, None, None, want=("input_rgb",), shape=(1, 256))
    inv_mean, inv_std = R.inv_norm(MEAN, STD)
    t = torch.from_numpy(x.copy())
    t.sub_(torch.from_numpy(inv_mean).view(3, 1, 1)).div_(torch.from_numpy(inv_std).view(3, 1, 1))
    live = t.mul(255).byte().permute(1, 2, 0).numpy()
    assert np.array_equal(got["input_rgb"], live), first_difference(got["input_rgb"], live)
    assert got["input_rgb"][0, 1, 0] == 0        # byte 1 of channel 0 does not survive the round trip
    return 1


def check_full_size(L, dev, shape=(1024, 2048)):
    """Past the cap of the grid: the grid-stride loop takes a second turn."""
    pal, ids = tables()
    inp = random_inputs(*shape, 5)
    return compare(run_dump_tail(L, dev, *inp, pal, ids), expected(*inp, pal, ids))


def mask_values():
    """k / 255 and its two fp32 neighbours for every k, 0, 1, the largest float below 1, and what saturates."""
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    v = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)),
                        np.array([0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), -0.0, -3.0, 1.5, 1e30, -1e30,
                                  np.nan, np.inf, -np.inf], np.float32)])
    return np.ascontiguousarray(v.astype(np.float32))


def run_mask_u8(L, dev, m, shift=0):
    t = _offset(torch.from_numpy(np.ascontiguousarray(m.reshape(-1))), dev, shift)
    guard = torch.full((m.size + shift + 16,), 0xA5, dtype=torch.uint8, device=dev)
    rc = L.ssa_mask_u8(ctypes.c_void_p(t.data_ptr()), m.size, ctypes.c_void_p(guard[shift:].data_ptr()), None)
    assert rc == 0, rc
    _sync(dev)
    h = guard.cpu().numpy()
    assert (h[:shift] == 0xA5).all() and (h[-16:] == 0xA5).all()
    return h[shift:-16].reshape(m.shape)


def check_mask_u8(L, dev):
    rng = np.random.RandomState(3)
    n = 0
    for m in (mask_values(), rng.rand(19, 27).astype(np.float32), rng.rand(3).astype(np.float32),
              rng.rand(1, 4099).astype(np.float32), rng.rand(300, 1031).astype(np.float32)):
        for shift in (0, 1):
            got = run_mask_u8(L, dev, m, shift)
            want = R.mask_bytes(m)
            assert np.array_equal(got, want), first_difference(got, want)
            n += 1
    return n


def device_form(dump_dict, dev):
    """The dump_dict of the reference's host assets as eval_minibatch(assets_on_device=True) leaves it: `predictions`,
    `err_mask` and every `pred_*` uint8 on dev, `prob_mask` and the `attn_*` fp32 on dev, the uploaded batch under
    `input_images` / `gt_images` of the assets; the loader's own tensors stay on the host."""
    assets = {}
    for k, v in dump_dict["assets"].items():
        t = torch.as_tensor(v)
        assets[k] = (t if t.is_floating_point() else t.to(torch.uint8)).to(dev)
    assets["input_images"] = dump_dict["input_images"].to(dev)
    assets["gt_images"] = dump_dict["gt_images"].to(dev)
    return dict(dump_dict, assets=assets)
