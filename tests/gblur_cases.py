"""Cases shared by tests/test_gblur_gpu.py (the kernels on the device) and tests/test_gblur_cpu.py (the same kernel
sources on the CPU emulation): each runs the product on `dev` and compares with the restatements (tests/gblur_ref.py,
tests/colorjit_ref.py), exactly.  Expected values never come from the code under test."""
import ctypes

import numpy as np
import torch

import colorjit_ref as CR
import gblur_ref as R

TILE_H, TILE_W = 16, 64                           # the workgroup's tile of csrc/gblur.hip
# sigma at both sides of every radius threshold of int(4 sigma + 0.5), and the ends of the reference's interval
SIGMAS = [0.15, 0.374, 0.376, 0.624, 0.626, 0.874, 0.876, 1.124, 1.126, 1.2999]
RADII = [1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
ONE_PER_RADIUS = [0.3, 0.5, 0.75, 1.0, 1.2999]
SHAPES = [(1, 1), (1, 9), (3, 2), (37, 53)]
# a program with the contrast step in the middle: brightness runs before the mean is taken, hue after it
JITTER_DRAWS = [("brightness", 1.2), ("contrast", 0.8), ("hue", -0.1), ("saturation", 1.25)]


def image(h, w, seed=0):
    return np.random.RandomState(1000 * h + w + seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def hostile_source(window, H, W, seed=3):
    """A source whose window holds random bytes and whose every pixel OUTSIDE the window is 255 - (the window pixel
    nearest to it): a kernel that clamps to the source image instead of the window, or not at all, reads a byte that
    differs from the right one wherever it looks."""
    x0, y0, w, h = window
    inner = image(h, w, seed)
    yy = np.clip(np.arange(H) - y0, 0, h - 1)
    xx = np.clip(np.arange(W) - x0, 0, w - 1)
    src = np.ascontiguousarray(255 - inner[yy][:, xx], dtype=np.uint8)
    src[y0:y0 + h, x0:x0 + w] = inner
    return src                                    # C-contiguous: also handed to the C ABI as it is


def params(draws):
    from semseg_amd.datasets import JitterParams
    return JitterParams([op for op, _ in draws], **dict(draws))


def run_u8(dev, img, sigma, window=None, flip=False, jitter=None):
    from semseg_amd.datasets import gaussian_blur
    return gaussian_blur(torch.from_numpy(img).to(dev), sigma, window, flip, jitter).cpu().numpy()


def run_fused(dev, img, sigma, window, flip, jitter=None):
    """The image half of crop_flip_normalize(..., jitter=..., blur=...) -> CPU tensor [h, w, 16]."""
    from semseg_amd.datasets.transforms import _image_half
    h, w = img.shape[:2]
    return _image_half(torch.from_numpy(img).to(dev), window or (0, 0, w, h), flip, jitter, sigma)[0].cpu()


def first_difference(got, want):
    if got.shape != want.shape:
        return "shapes %s / %s" % (got.shape, want.shape)
    ys, xs = np.nonzero((got != want).any(-1))
    y, x = int(ys[0]), int(xs[0])
    return "%d of %d pixels differ; first at (y %d, x %d): got %s want %s" % (
        len(ys), got.shape[0] * got.shape[1], y, x, got[y, x].tolist(), want[y, x].tolist())


def check_blur(dev, img, sigma, window=None, flip=False):
    want = R.blur(img, sigma, window, flip)
    got = run_u8(dev, img, sigma, window, flip)
    assert got.dtype == np.uint8 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), (sigma, window, flip, first_difference(got, want))


def check_sigmas_and_shapes(dev):
    """Every sigma of the table on every shape, whole image; 1 x 1, 1 x 9 and 3 x 2 are smaller than every radius > 1."""
    assert [R.taps(s)[0] for s in SIGMAS] == RADII and [R.taps(s)[0] for s in ONE_PER_RADIUS] == [1, 2, 3, 4, 5]
    for sigma in SIGMAS:
        for h, w in SHAPES:
            check_blur(dev, image(h, w), sigma)


def check_small_windows_at_radius_5(dev):
    """Windows smaller than the radius inside a larger source: every tap but the centre is clamped, in one or both axes."""
    for h, w in SHAPES[:3]:
        window = (5, 3, w, h)
        src = hostile_source(window, 9, 17)
        for flip in (False, True):
            check_blur(dev, src, 1.2999, window, flip)


def check_window_over_several_tiles(dev):
    """(TILE_H + 3) x (2 TILE_W + 5) at (7, 5): two rows and three columns of workgroups with partial tiles at the right
    and at the bottom, every radius, both directions."""
    window = (7, 5, 2 * TILE_W + 5, TILE_H + 3)
    src = hostile_source(window, TILE_H + 3 + 11, 2 * TILE_W + 5 + 16)
    for sigma in ONE_PER_RADIUS:
        for flip in (False, True):
            check_blur(dev, src, sigma, window, flip)


def check_levels(dev, sigmas):
    img = R.levels_image()
    for sigma in sigmas:
        check_blur(dev, img, sigma)


def check_fixture_entries(dev):
    inputs, outputs, meta = R.load_golden()
    for e, img, want in zip(meta["entries"], inputs, outputs):
        got = run_u8(dev, img, e["sigma"])
        assert np.array_equal(got, want), (e["seed"], e["sigma"], first_difference(got, want))


def _normalize_through_abi(dev, u8):
    """ssa_image_u8_crop_flip_normalize of a whole uint8 image, through the C ABI (so that it also runs on CPU tensors)."""
    from semseg_amd import _lib, hip_backend as hb
    from semseg_amd.datasets.transforms import MEAN_STD
    h, w = u8.shape[:2]
    t = torch.from_numpy(u8).to(dev)
    two = torch.empty((h, w, 16), dtype=hb.ACT_DTYPE, device=dev)
    mean, std = (ctypes.c_float * 3)(*MEAN_STD[0]), (ctypes.c_float * 3)(*MEAN_STD[1])
    _lib.check(_lib.lib().ssa_image_u8_crop_flip_normalize(hb._p(t), h, w, 0, 0, w, h, 0, mean, std, hb._p(two), 16, hb._s()),
               "ssa_image_u8_crop_flip_normalize")
    return two.cpu()


def check_fused_equals_two_steps(dev):
    """ssa_gblur_crop_flip_normalize == ssa_gblur_u8 followed by today's ssa_image_u8_crop_flip_normalize, with and without
    a jitter program, in the loaded build's element type; the u8 step equals the restatement."""
    from semseg_amd import hip_backend as hb
    window = (7, 5, TILE_W + 5, TILE_H + 3)
    src = hostile_source(window, TILE_H + 3 + 11, TILE_W + 5 + 16)
    for sigma in (0.3, 1.2999):
        for flip in (False, True):
            for draws in (None, JITTER_DRAWS):
                p = None if draws is None else params(draws)
                fused = run_fused(dev, src, sigma, window, flip, p)
                u8 = run_u8(dev, src, sigma, window, flip, p)
                two = _normalize_through_abi(dev, u8)
                assert fused.dtype == hb.ACT_DTYPE and tuple(fused.shape) == (window[3], window[2], 16)
                assert torch.equal(fused.view(torch.int16), two.view(torch.int16)), (sigma, flip, draws)
                pre = src if draws is None else CR.jitter(src, CR.program_of(draws), window, flip)
                want = R.blur(src, sigma, window, flip) if draws is None else R.blur(pre, sigma)
                assert np.array_equal(u8, want), (sigma, flip, draws, first_difference(u8, want))


def check_jitter_then_blur(dev):
    """jitter + blur in one launch == ssa_jitter_apply_u8 followed by ssa_gblur_u8(program = NULL) == the two
    restatements in sequence; the contrast mean is the window's, taken after the brightness step."""
    from semseg_amd.datasets import color_jitter
    window = (7, 5, 2 * TILE_W + 5, TILE_H + 3)
    src = hostile_source(window, TILE_H + 3 + 11, 2 * TILE_W + 5 + 16)
    p = params(JITTER_DRAWS)
    for sigma in (0.5, 1.2999):
        for flip in (False, True):
            one = run_u8(dev, src, sigma, window, flip, p)
            jit = color_jitter(torch.from_numpy(src).to(dev), p, window, flip).cpu().numpy()
            two = run_u8(dev, jit, sigma)
            want_jit = CR.jitter(src, CR.program_of(JITTER_DRAWS), window, flip)
            assert np.array_equal(jit, want_jit)
            assert np.array_equal(one, two), (sigma, flip, first_difference(one, two))
            assert np.array_equal(one, R.blur(want_jit, sigma)), (sigma, flip)
