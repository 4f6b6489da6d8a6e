"""Cases shared by tests/test_randaugment_gpu.py (the kernels on the device) and tests/test_randaugment_cpu.py (the same
kernel sources on the CPU emulation): each runs the product on `dev`, compares with the restatement
(tests/randaug_ref.py) byte for byte and returns the number of comparisons it made.  Expected values never come from the
code under test."""
import numpy as np
import torch

import randaug_ref as R

TILE_H, TILE_W = 16, 64                           # the Sharpness tile of csrc/randaugment.hip
MAGNITUDES = (0, 1, 9, 15, 30)
SHARP = (0.1, 1.0, 1.9)
# chains that together run every kernel: both warps of the image, both of the labels, the histogram and both tables,
# every point operation, the stencil, the copy; with one, two and three launches on a buffer (the ping-pong)
PROGRAMS = [
    [("ShearX", 0.21), ("Sharpness", 1.9)],
    [("Rotate", -17.0), ("Equalize", 0.0), ("TranslateY", 3.3)],
    [("AutoContrast", 0.0), ("Color", 1.54), ("ShearY", -0.3)],
    [("TranslateX", -5.445), ("Solarize", 33.0), ("Posterize", 5), ("Invert", 0.0), ("Brightness", 0.64)],
    [("Sharpness", 0.1)],
    [("Equalize", 0.0), ("AutoContrast", 0.0)],
    [("Identity", 0.3)],
    [("Rotate", 0.0), ("Identity", 1.0)],
    [],
]
# a2 + 0.5 inside (-1, 0) and within 2^-17 of an integer, and on both sides of other integers: where Pillow's scale routine
# (a double running sum, truncated; negative = outside) and its 16.16 fixed-point path disagree
TRANSLATION_OFFSETS = [k - 0.5 + e for k in (0, 1, 5, -3) for e in (2.0 ** -18, -2.0 ** -18, 1e-9, -1e-9, 0.3, -0.3)]


def image(h, w, seed=0):
    return np.random.RandomState(1000 * h + w + seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def narrow_image(h=37, w=53):
    """Values 60..190 in R, 3..4 in G, 0..255 in B: AutoContrast stretches, nearly saturates, and leaves."""
    img = image(h, w, 5).astype(np.int64)
    img[..., 0] = 60 + img[..., 0] % 131
    img[..., 1] = 3 + img[..., 1] % 2
    img[0, 0, 2], img[0, 1, 2] = 0, 255
    return img.astype(np.uint8)


def one_value_band_image(h=37, w=53):
    img = image(h, w, 6)
    img[..., 1] = 77
    return img


def step_zero_image():
    """12 x 20 = 240 pixels: (N - last count) // 255 == 0 in every band, Equalize's second identity branch."""
    return image(12, 20, 7)


def all_values_image():
    """64 x 64 holding all 256 values in every band, 16 times each, in a different order per band."""
    rng = np.random.RandomState(8)
    return np.stack([rng.permutation(np.repeat(np.arange(256), 16)).reshape(64, 64) for _ in range(3)], -1).astype(np.uint8)


def hostile_source(window, H, W, seed=3):
    """(image, labels) whose window holds random bytes / classes and whose every pixel OUTSIDE the window is 255 - (the
    window pixel nearest to it), resp. class 200: a kernel that clamps to the source instead of the window, or reads past
    the window, reads a byte that differs from the right one."""
    x0, y0, w, h = window
    inner = image(h, w, seed)
    yy = np.clip(np.arange(H) - y0, 0, h - 1)
    xx = np.clip(np.arange(W) - x0, 0, w - 1)
    src = np.ascontiguousarray(255 - inner[yy][:, xx], dtype=np.uint8)
    src[y0:y0 + h, x0:x0 + w] = inner
    lab = np.full((H, W), 200, np.uint8)
    lab[y0:y0 + h, x0:x0 + w] = R.label_map(h, w, seed)
    return src, lab


def params(program, w, h):
    from semseg_amd.datasets import AugmentParams
    return AugmentParams(program, (w, h))


def run(dev, img, lab, program, window=None, flip=False, ignore_label=255):
    from semseg_amd.datasets import rand_augment
    w, h = (img.shape[1], img.shape[0]) if window is None else (window[2], window[3])
    gi, gl = rand_augment(torch.from_numpy(img).to(dev), None if lab is None else torch.from_numpy(lab).to(dev),
                          params(program, w, h), window, flip, ignore_label)
    return gi.cpu().numpy(), None if gl is None else gl.cpu().numpy()


def first_difference(got, want):
    if got.shape != want.shape:
        return "shapes %s / %s" % (got.shape, want.shape)
    d = (got != want).reshape(got.shape[0], got.shape[1], -1).any(-1)
    ys, xs = np.nonzero(d)
    y, x = int(ys[0]), int(xs[0])
    return "%d of %d pixels differ; first at (y %d, x %d): got %s want %s" % (
        len(ys), d.size, y, x, got[y, x].tolist(), want[y, x].tolist())


def check(dev, img, lab, program, window=None, flip=False, ignore_label=255):
    wi, wl = R.augment(img, lab, program, window, flip, ignore_label)
    gi, gl = run(dev, img, lab, program, window, flip, ignore_label)
    assert gi.dtype == np.uint8 and gi.shape == wi.shape, (gi.shape, wi.shape)
    assert np.array_equal(gi, wi), (program, window, flip, "image", first_difference(gi, wi))
    if lab is None:
        assert gl is None
    else:
        assert gl.dtype == np.uint8 and np.array_equal(gl, wl), (program, window, flip, "labels", first_difference(gl, wl))
    return 1


def signed_value(op, m, negate, w, h):
    v = R.magnitude(op, m)
    if op in R.GEOMETRIC and negate:
        v = -v
    if op == "TranslateX":
        v *= w
    if op == "TranslateY":
        v *= h
    return int(v) if op == "Posterize" else v


def per_op_programs(w, h):
    """Every operation at every magnitude of the fixture, both signs of the five signed ones: 95 one-step programs."""
    out = []
    for op in R.OPS:
        for m in MAGNITUDES:
            for negate in ((False, True) if op in R.GEOMETRIC else (False,)):
                out.append([(op, signed_value(op, m, negate, w, h))])
    return out


def check_every_op_on_the_fixture_images(dev):
    z, meta = R.load_golden()
    n = 0
    for k, program in enumerate(per_op_programs(53, 37)):
        n += check(dev, z["images"][k % 2], z["labels"][k % 2], program, ignore_label=meta["ignore_label"])
    return n


def check_table_ops_on_special_images(dev):
    """AutoContrast and Equalize where their branches lie, and every table / point operation over all 256 values."""
    n = 0
    for img in (narrow_image(), one_value_band_image(), step_zero_image()):
        for op in ("AutoContrast", "Equalize"):
            n += check(dev, img, None, [(op, 0.0)])
    img = all_values_image()
    for program in ([("AutoContrast", 0.0)], [("Equalize", 0.0)], [("Invert", 0.0)], [("Solarize", 0.0)],
                    [("Solarize", 33.0)], [("Solarize", 109.99999)], [("Solarize", 110.0)], [("Posterize", 4)],
                    [("Posterize", 6)], [("Posterize", 8)], [("Color", 0.1)], [("Color", 1.9)], [("Brightness", 0.1)],
                    [("Brightness", 1.9)]):
        n += check(dev, img, None, program)
    return n


def check_sharpness_images(dev):
    n = 0
    for img in (R.levels_image(), R.checkerboard()):
        for v in SHARP:
            n += check(dev, img, None, [("Sharpness", v)])
    return n


def check_label_translations(dev):
    """The offsets at which Pillow's two nearest routines disagree, on both axes, at 53 and 64 columns."""
    n = 0
    for w in (53, 64):
        img, lab = image(37, w, 9), R.label_map(37, w, 7)
        for off in TRANSLATION_OFFSETS:
            for op in ("TranslateX", "TranslateY"):
                n += check(dev, img, lab, [(op, off)])
    # 1100 columns (rows): the running sum crosses every power of two up to 1024, from a start far below zero as well
    wide, tall = R.label_map(2, 1100, 3), R.label_map(1100, 2, 4)
    for off in (-300.5 + 1e-9, -0.3 - 2.0 ** -30, 0.7 / 3, 17.123456789, -1.0 - 1e-12):
        n += check(dev, np.zeros((2, 1100, 3), np.uint8), wide, [("TranslateX", off)])
        n += check(dev, np.zeros((1100, 2, 3), np.uint8), tall, [("TranslateY", off)])
    return n


def check_fixture_chains(dev):
    """The product on the drawn programs of the fixture equals what the reference produced."""
    z, meta = R.load_golden()
    n = 0
    for e in meta["chains"]:
        img, lab = z["images"][e["image"]], z["labels"][e["image"]]
        gi, gl = run(dev, img, lab, [tuple(s) for s in e["program"]], ignore_label=meta["ignore_label"])
        wi, wl = z["out_images"][e["out_image"]], z["out_labels"][e["out_label"]]
        assert np.array_equal(gi, wi), (e["seed"], e["program"], first_difference(gi, wi))
        assert np.array_equal(gl, wl), (e["seed"], e["program"], first_difference(gl, wl))
        n += 1
    return n


def check_window_inside_a_larger_source(dev):
    window = (5, 3, 53, 37)
    src, lab = hostile_source(window, 37 + 9, 53 + 12)
    n = 0
    for program in PROGRAMS:
        for flip in (False, True):
            n += check(dev, src, lab, program, window, flip, ignore_label=254)
    return n


def check_window_over_several_tiles(dev):
    """(TILE_H + 3) x (2 TILE_W + 5) at (7, 5): two rows and three columns of Sharpness tiles with partial tiles at the
    right and at the bottom, more than one workgroup of every streaming kernel."""
    window = (7, 5, 2 * TILE_W + 5, TILE_H + 3)
    src, lab = hostile_source(window, TILE_H + 3 + 11, 2 * TILE_W + 5 + 16)
    n = 0
    for program in PROGRAMS[:6]:
        for flip in (False, True):
            n += check(dev, src, lab, program, window, flip)
    return n


def check_tiny_windows(dev):
    n = 0
    for h, w in ((1, 1), (1, 9), (7, 1), (2, 2)):
        window = (4, 2, w, h)
        src, lab = hostile_source(window, 11, 17)
        for program in PROGRAMS:
            n += check(dev, src, lab, program, window, True)
    return n


def check_labels_absent(dev):
    window = (5, 3, 53, 37)
    src, _ = hostile_source(window, 37 + 9, 53 + 12)
    n = 0
    for program in PROGRAMS:
        n += check(dev, src, None, program, window, True)
    return n


class _OnDevice(torch.Tensor):
    """A CPU tensor that answers is_cuda as a device tensor does (crop_flip_normalize asserts it of its inputs): how the
    emulation, whose device memory is host memory, runs the public entry point."""
    is_cuda = property(lambda self: True)


def on_device(a, dev):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.as_subclass(_OnDevice) if str(dev) == "cpu" else t.to(dev)


def check_tail_equals_steps_in_sequence(dev):
    """crop_flip_normalize(..., augment=p, jitter=j, blur=b) == rand_augment, then crop_flip_normalize(jitter=j, blur=b)
    of what it returned, bit for bit in the build's element type; the chain's outputs equal the restatement, and the
    jitter's contrast mean is the one of the AUGMENTED window (colorjit_ref on the restated chain output)."""
    import colorjit_ref as CR
    import gblur_cases as GK
    from semseg_amd.datasets import BlurParams, color_jitter, crop_flip_normalize, rand_augment
    window = (7, 5, TILE_W + 5, TILE_H + 3)
    src, lab = hostile_source(window, TILE_H + 3 + 11, TILE_W + 5 + 16)
    program = [("ShearX", -0.21), ("Equalize", 0.0), ("Sharpness", 1.9)]
    p = params(program, window[2], window[3])
    wi, wl = R.augment(src, lab, program, window, True)
    n = 0
    for jitter in (None, GK.params(GK.JITTER_DRAWS)):
        for blur in (None, BlurParams(0.7)):
            fused, gts = crop_flip_normalize(on_device(src, dev), on_device(lab, dev), window, True, jitter=jitter,
                                             blur=blur, augment=p)
            ai, al = rand_augment(on_device(src, dev), on_device(lab, dev), p, window, True)
            assert np.array_equal(ai.cpu().numpy(), wi) and np.array_equal(al.cpu().numpy(), wl)
            two, gts2 = crop_flip_normalize(on_device(wi, dev), on_device(wl, dev), (0, 0, window[2], window[3]), False,
                                            jitter=jitter, blur=blur)
            assert tuple(fused.shape) == (1, window[3], window[2], 16) and gts.dtype == torch.int64
            assert torch.equal(fused.cpu().view(torch.int16), two.cpu().view(torch.int16)), (jitter, blur)
            assert torch.equal(gts.cpu(), gts2.cpu()) and np.array_equal(gts.cpu().numpy()[0], wl.astype(np.int64))
            if jitter is not None:
                jit = color_jitter(on_device(wi, dev), jitter).cpu().numpy()
                assert np.array_equal(jit, CR.jitter(wi, CR.program_of(GK.JITTER_DRAWS)))
            n += 1
    return n
