"""Cases shared by tests/test_colorjitter_gpu.py (the kernels on the device) and tests/test_colorjitter_cpu.py (the same
kernel sources on the CPU emulation): each runs the product on `dev` and compares with the restatement
(tests/colorjit_ref.py), exactly.  Expected values never come from the code under test."""
import itertools

import numpy as np
import torch

import colorjit_ref as R

# one factor per operation for the hand-made chains: a truncating blend (<= 1), two clipping ones (> 1), a negative
# hue factor (byte 230)
FACTORS = {"brightness": 1.2, "contrast": 0.8, "saturation": 1.25, "hue": -0.1}
ORDERS24 = list(itertools.permutations(R.OPS))
WINDOW_CASES = [((3, 5, 37, 29), False), ((3, 5, 37, 29), True), ((0, 0, 80, 64), False), ((0, 0, 80, 64), True)]


def params(draws):
    """[(op, factor)] in application order (hue with its factor) -> the product's JitterParams."""
    from semseg_amd.datasets import JitterParams
    return JitterParams([op for op, _ in draws], **dict(draws))


def draws_of(order, factors=FACTORS):
    return [(op, factors[op]) for op in order]


def images_37x53():
    return R.load_golden()[0]


def window_source():
    return np.random.RandomState(7).randint(0, 256, (64, 80, 3)).astype(np.uint8)


def run_u8(dev, img, p, window=None, flip=False):
    from semseg_amd.datasets import color_jitter
    return color_jitter(torch.from_numpy(img).to(dev), p, window, flip).cpu().numpy()


def run_fused(dev, img, p, window, flip):
    """The image half of crop_flip_normalize(..., jitter=p) -> CPU tensor [h, w, 16]."""
    from semseg_amd.datasets.transforms import _image_half
    h, w = img.shape[:2]
    return _image_half(torch.from_numpy(img).to(dev), window or (0, 0, w, h), flip, p)[0].cpu()


def first_difference(got, want, img):
    ys, xs = np.nonzero((got != want).any(-1))
    if len(ys) == 0:
        return "shapes %s / %s" % (got.shape, want.shape)
    y, x = int(ys[0]), int(xs[0])
    return "%d of %d pixels differ; first at (y %d, x %d): source %s got %s want %s" % (
        len(ys), got.shape[0] * got.shape[1], y, x, img[y, x].tolist() if img.shape == got.shape else "?",
        got[y, x].tolist(), want[y, x].tolist())


def check_chain(dev, img, draws, window=None, flip=False):
    want = R.jitter(img, R.program_of(draws), window, flip)
    got = run_u8(dev, img, params(draws), window, flip)
    assert got.dtype == np.uint8 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), (draws, window, flip, first_difference(got, want, img))


def check_all_orders(dev):
    for img in images_37x53():
        for order in ORDERS24:
            check_chain(dev, img, draws_of(order))


def check_short_programs(dev):
    """Programs of 0, 1, 2 and 3 operations; contrast first and contrast last."""
    img = images_37x53()[0]
    for order in [(), ("brightness",), ("contrast",), ("saturation",), ("hue",), ("hue", "contrast"),
                  ("contrast", "saturation"), ("saturation", "hue", "brightness"), ("contrast", "hue", "saturation"),
                  ("brightness", "hue", "contrast"), ("contrast", "brightness", "saturation", "hue"),
                  ("hue", "saturation", "brightness", "contrast")]:
        check_chain(dev, img, draws_of(order))
    assert np.array_equal(run_u8(dev, img, params([])), img)


def check_fixture_entries(dev):
    images, outputs, meta = R.load_golden()
    for e, want in zip(meta["entries"], outputs):
        draws = [(op, v) for op, v in e["draws"]]
        got = run_u8(dev, images[e["image"]], params(draws))
        assert np.array_equal(got, want), (e["seed"], draws, first_difference(got, want, images[e["image"]]))


def check_mean_rounding(dev):
    """m = int(S / N + 0.5): L {10, 11} -> 10.5 -> 11; L {10, 10, 11} -> 10.33 -> 10; one pixel -> its own L.  Contrast
    at factor 0 writes m itself."""
    def grey(*ls):
        return np.array([[[v, v, v] for v in ls]], dtype=np.uint8)
    for img, m in ((grey(10, 11), 11), (grey(10, 10, 11), 10), (grey(200), 200),
                   (np.array([[[255, 0, 3]]], dtype=np.uint8), 77)):
        assert R.contrast_mean(img) == m
        got = run_u8(dev, img, params([("contrast", 0.0)]))
        assert np.array_equal(got, np.full_like(img, m)), (img.tolist(), got.tolist(), m)
        for f in (0.5, 1.25):
            check_chain(dev, img, [("contrast", f)])


def check_windows(dev):
    src = window_source()
    for window, flip in WINDOW_CASES:
        check_chain(dev, src, draws_of(("saturation", "contrast", "hue", "brightness")), window, flip)
        check_chain(dev, src, draws_of(("hue", "brightness")), window, flip)


def check_fused_equals_two_steps(dev):
    """ssa_jitter_crop_flip_normalize == ssa_jitter_apply_u8 followed by today's ssa_image_u8_crop_flip_normalize (through
    the C ABI here, so that the case also runs on CPU tensors), and the u8 step equals the restatement."""
    import ctypes
    from semseg_amd import _lib, hip_backend as hb
    from semseg_amd.datasets.transforms import MEAN_STD
    src = window_source()
    for window, flip in WINDOW_CASES:
        for order in (("saturation", "contrast", "hue", "brightness"), ("brightness",), ()):
            draws = draws_of(order)
            p = params(draws)
            fused = run_fused(dev, src, p, window, flip)
            u8 = run_u8(dev, src, p, window, flip)
            assert np.array_equal(u8, R.jitter(src, R.program_of(draws), window, flip))
            h, w = u8.shape[:2]
            t = torch.from_numpy(u8).to(dev)
            two = torch.empty((h, w, 16), dtype=hb.ACT_DTYPE, device=dev)
            mean, std = (ctypes.c_float * 3)(*MEAN_STD[0]), (ctypes.c_float * 3)(*MEAN_STD[1])
            _lib.check(_lib.lib().ssa_image_u8_crop_flip_normalize(hb._p(t), h, w, 0, 0, w, h, 0, mean, std, hb._p(two), 16,
                                                                   hb._s()), "ssa_image_u8_crop_flip_normalize")
            assert fused.dtype == hb.ACT_DTYPE and tuple(fused.shape) == (h, w, 16)
            assert torch.equal(fused.view(torch.int16), two.cpu().view(torch.int16)), (window, flip, order)


def check_padded_store(dev):
    """The normalise store at the padded channel counts the Python layer never passes -- 8 (no zero piece) and 24 (two) --
    through the C ABI, from the plain tail and from the jitter entry (empty program; four operations with the contrast
    step in the middle): channels 0-2 equal the oracle's tail (on the window; for the jitter entry on the restatement's
    jittered, mirrored window) cast to the build's element type, the padding is all-zero bits, and the pixel after the
    last keeps the NaN pattern the buffer was filled with."""
    import ctypes
    from oracle.data import crop_flip_normalize as oracle
    from semseg_amd import _lib, hip_backend as hb
    from semseg_amd.datasets.transforms import MEAN_STD
    L = _lib.lib()
    src = np.random.RandomState(11).randint(0, 256, (12, 16, 3)).astype(np.uint8)
    H, W = src.shape[:2]
    window = x0, y0, w, h = (3, 2, 7, 5)
    nolab = np.zeros((H, W), np.uint8)
    t = torch.from_numpy(src).to(dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    mean, std = (ctypes.c_float * 3)(*MEAN_STD[0]), (ctypes.c_float * 3)(*MEAN_STD[1])
    for flip in (False, True):
        for cpad in (8, 24):
            for draws in (None, [], draws_of(("brightness", "contrast", "hue", "saturation"))):
                out = torch.full((h * w + 1, cpad), 0x7FC1, dtype=torch.int16, device=dev)
                if draws is None:
                    _lib.check(L.ssa_image_u8_crop_flip_normalize(hb._p(t), H, W, x0, y0, w, h, int(flip), mean, std,
                                                                  hb._p(out), cpad, hb._s()), "ssa_image_u8_crop_flip_normalize")
                    want = oracle(src, nolab, window, flip, *MEAN_STD)[0]
                else:
                    pg = params(draws).program()
                    _lib.check(L.ssa_jitter_luma_sum(hb._p(t), H, W, x0, y0, w, h, ctypes.byref(pg), hb._p(counter), hb._s()),
                               "ssa_jitter_luma_sum")
                    _lib.check(L.ssa_jitter_crop_flip_normalize(hb._p(t), H, W, x0, y0, w, h, int(flip), ctypes.byref(pg),
                                                                hb._p(counter), mean, std, hb._p(out), cpad, hb._s()),
                               "ssa_jitter_crop_flip_normalize")
                    jittered = R.jitter(src, R.program_of(draws), window, flip)
                    want = oracle(jittered, nolab, (0, 0, w, h), False, *MEAN_STD)[0]
                want = torch.from_numpy(want).permute(1, 2, 0).to(hb.ACT_DTYPE).contiguous().view(torch.int16).reshape(h * w, 3)
                got = out.cpu()
                case = (flip, cpad, draws)
                assert torch.equal(got[:h * w, :3], want), case
                assert int(got[:h * w, 3:].count_nonzero()) == 0, case
                assert bool((got[h * w] == 0x7FC1).all()), case
