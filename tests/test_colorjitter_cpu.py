"""ColorJitter without a GPU:
  * the numpy restatement (tests/colorjit_ref.py) against live Pillow -- every per-pixel operation over all 2^24 colours,
    all 24 orders of a four-operation chain -- and against the fixture recorded from the reference
    (tests/golden/colorjitter_golden.npz, make_golden_colorjitter.py);
  * the product's ColorJitter.get_params against the draws recorded from the reference's;
  * the kernels of csrc/color_jitter.hip, compiled for the host (tools/emu), against the restatement, bit for bit;
  * argument validation of the three entry points."""
import ctypes
import hashlib

import numpy as np
import pytest

import colorjit_cases as K
import colorjit_ref as R


@pytest.fixture(scope="module")
def cube():
    return R.all_colours()


def _strips(fn, img, rows=256):
    return np.concatenate([fn(img[i:i + rows]) for i in range(0, img.shape[0], rows)], 0)


def _pillow_hue(pil, byte):
    from PIL import Image
    h, s, v = pil.convert("HSV").split()
    np_h = (np.array(h, dtype=np.uint8).astype(np.int64) + byte).astype(np.uint8)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def _pillow_chain(img, program):
    from PIL import Image, ImageEnhance
    pil = Image.fromarray(img)
    for op, v in program:
        if op == "hue":
            pil = _pillow_hue(pil, v)
        else:
            enh = {"brightness": ImageEnhance.Brightness, "contrast": ImageEnhance.Contrast,
                   "saturation": ImageEnhance.Color}[op]
            pil = enh(pil).enhance(v)
    return np.array(pil)


@pytest.mark.parametrize("op", ["brightness", "saturation"])
def test_restatement_blends_equal_pillow_on_every_colour(cube, op):
    """Truncating factors (short binary fractions and not), the identity, and clipping ones."""
    hashes = R.load_golden()[2]["hashes"]
    assert "%s:0.75" % op in hashes and "%s:1.25" % op in hashes
    for f in (0.75, 0.8123456, 0.9000001, 1.0, 1.1, 1.2499, 1.25):
        want = _pillow_chain(cube, [(op, f)])
        got = _strips(lambda x: R.apply_op(x, op, f), cube)
        assert np.array_equal(got, want), (op, f, K.first_difference(got, want, cube))
        key = "%s:%r" % (op, f)                    # the fixture's hashes (the GPU test's yardstick) are this Pillow's
        if key in hashes:
            assert hashlib.sha256(want.tobytes()).hexdigest() == hashes[key], key


def test_restatement_contrast_equals_pillow_on_every_colour(cube):
    m = R.contrast_mean(cube)
    for f in (0.75, 1.2499):
        want = _pillow_chain(cube, [("contrast", f)])
        got = _strips(lambda x: R.contrast(x, f, mean=m), cube)
        assert np.array_equal(got, want), (f, K.first_difference(got, want, cube))


def test_restatement_rgb_to_hsv_equals_pillow_on_every_colour(cube):
    from PIL import Image
    hsv = _strips(R.rgb_to_hsv, cube)
    want = np.array(Image.fromarray(cube).convert("HSV"))
    assert np.array_equal(hsv, want), K.first_difference(hsv, want, cube)


def test_restatement_hsv_to_rgb_equals_pillow_on_every_hsv(cube):
    """All 2^24 (H, S, V); and the fixture's hash of the shifted round trip is what this Pillow gives."""
    from PIL import Image
    back = _strips(R.hsv_to_rgb, cube)
    want = np.array(Image.frombytes("HSV", (4096, 4096), cube.tobytes()).convert("RGB"))
    assert np.array_equal(back, want), K.first_difference(back, want, cube)
    hashes = R.load_golden()[2]["hashes"]
    assert len(hashes) == 13
    assert hashlib.sha256(np.array(_pillow_hue(Image.fromarray(cube), 193)).tobytes()).hexdigest() == hashes["hue:193"]


def test_restatement_equals_pillow_on_all_24_orders():
    for img in K.images_37x53():
        for order in K.ORDERS24:
            program = R.program_of(K.draws_of(order))
            got, want = R.jitter(img, program), _pillow_chain(img, program)
            assert np.array_equal(got, want), (order, K.first_difference(got, want, img))
        for f in (0.75, 0.8123456, 0.9000001, 1.0, 1.1, 1.2499, 1.25):
            assert np.array_equal(R.contrast(img, f), _pillow_chain(img, [("contrast", f)])), f


def test_restatement_equals_the_reference_fixture():
    images, outputs, meta = R.load_golden()
    assert len(meta["entries"]) >= 32 and any(e["wrapped"] for e in meta["entries"])
    assert any(not e["wrapped"] and any(op == "hue" for op, _ in e["draws"]) for e in meta["entries"])
    for e, want in zip(meta["entries"], outputs):
        got = R.jitter(images[e["image"]], R.program_of(e["draws"]))
        assert np.array_equal(got, want), (e["seed"], K.first_difference(got, want, images[e["image"]]))
    assert np.array_equal(images[1], R.pink_image(37, 53, 12))


def test_get_params_reproduces_the_recorded_draws():
    """The product consumes np.random as the reference does: same factors (to the bit), same shuffled order, same state
    of the generator afterwards."""
    from semseg_amd.datasets import ColorJitter
    for e in R.load_golden()[2]["entries"]:
        np.random.seed(e["seed"])
        p = ColorJitter.get_params(*e["args"])
        after = np.random.random()
        assert list(p.order) == [op for op, _ in e["draws"]], e["seed"]
        for op, v in e["draws"]:
            assert getattr(p, op) == v, (e["seed"], op)
        np.random.seed(e["seed"])
        assert R.get_params(*e["args"]) == [(op, v) for op, v in e["draws"]]
        assert np.random.random() == after
        for op, v in e["draws"]:
            if op == "hue":
                assert p.hue_byte == R.hue_byte(v) == int(np.trunc(v * 255)) % 256


def test_hue_byte_and_adjust_hue_range():
    from semseg_amd.datasets import adjust_hue
    from semseg_amd.datasets.transforms import hue_to_byte
    assert [hue_to_byte(v) for v in (-0.25, 0.25, 0.0, -0.5, 0.5, -0.001, 0.004)] == [193, 63, 0, 129, 127, 0, 1]
    for bad in (0.51, -0.6):
        with pytest.raises(ValueError):
            adjust_hue(None, bad)


# ------------------------------------------------------------------ the kernels on the CPU emulation
@pytest.fixture()
def emu():
    from emu_util import emu_backend
    with emu_backend():
        yield "cpu"


def test_emulated_kernels_all_orders_and_short_programs(emu):
    K.check_all_orders(emu)
    K.check_short_programs(emu)


def test_emulated_kernels_reference_fixture(emu):
    K.check_fixture_entries(emu)


@pytest.mark.parametrize("op,value", [("brightness", 0.75), ("brightness", 1.25), ("saturation", 0.75),
                                      ("saturation", 1.25), ("contrast", 0.8), ("contrast", 1.25), ("hue", 0.25),
                                      ("hue", -0.25), ("hue", 0.004)])
def test_emulated_kernels_on_a_sample_of_the_colour_cube(emu, cube, op, value):
    """4096 colours at stride 4099 (odd, so every channel runs through all its values) + the corners."""
    idx = (np.arange(4096, dtype=np.int64) * 4099) % (1 << 24)
    sample = cube.reshape(-1, 3)[idx].reshape(64, 64, 3).copy()
    sample[0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [1, 0, 255]]
    K.check_chain(emu, sample, [(op, value)])


def test_emulated_kernels_mean_rounding_windows_and_fused_tail(emu):
    K.check_mean_rounding(emu)
    K.check_windows(emu)
    K.check_fused_equals_two_steps(emu)


def test_emulated_normalise_store_at_8_and_24_padded_channels(emu):
    K.check_padded_store(emu)


def test_emulated_luma_sum_over_several_workgroups(emu):
    """1 x 257 (a second workgroup with one pixel) and 40 x 64 (ten workgroups, one atomic each)."""
    rng = np.random.RandomState(3)
    for shape in ((1, 257, 3), (40, 64, 3)):
        img = rng.randint(0, 256, shape).astype(np.uint8)
        K.check_chain(emu, img, K.draws_of(("brightness", "contrast", "saturation")))


# ------------------------------------------------------------------ argument validation (the real library, no device)
def test_entry_points_reject_bad_arguments_without_gpu():
    from semseg_amd import _lib
    L = _lib.lib()
    P = ctypes.c_void_p
    buf = (ctypes.c_ubyte * 4096)()                    # never read: every call below fails validation first
    ptr = P(ctypes.addressof(buf))
    mean, std = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.2, 0.2, 0.2)

    def prog(ops, hue_byte=0, factors=(1.0, 1.0, 1.0)):
        pg = _lib.JitterProgram()
        pg.n_ops = len(ops)
        for k, op in enumerate(ops[:4]):
            pg.op[k] = op
        pg.factor[0], pg.factor[1], pg.factor[2] = factors
        pg.hue_byte = hue_byte
        return pg

    def calls(img, H, W, x0, y0, cw, ch, pg, counter, out):
        pgp = None if pg is None else ctypes.byref(pg)
        return (L.ssa_jitter_luma_sum(img, H, W, x0, y0, cw, ch, pgp, counter, None),
                L.ssa_jitter_apply_u8(img, H, W, x0, y0, cw, ch, 0, pgp, counter, out, None),
                L.ssa_jitter_crop_flip_normalize(img, H, W, x0, y0, cw, ch, 0, pgp, counter, mean, std, out, 16, None))

    ok = prog([0, 1, 2, 3])
    for bad in [(None, 8, 8, 0, 0, 8, 8, ok, ptr, ptr),            # null image
                (ptr, 8, 8, 1, 0, 8, 8, ok, ptr, ptr),             # window beyond the right edge
                (ptr, 8, 8, 0, 2, 8, 7, ok, ptr, ptr),             # ... beyond the bottom
                (ptr, 8, 8, -1, 0, 4, 4, ok, ptr, ptr),
                (ptr, 8, 8, 0, 0, 0, 4, ok, ptr, ptr),             # empty window
                (ptr, 0, 8, 0, 0, 1, 1, ok, ptr, ptr),
                (ptr, 8, 8, 0, 0, 8, 8, None, ptr, ptr),           # null program
                (ptr, 8, 8, 0, 0, 8, 8, prog([0, 7]), ptr, ptr),   # unknown op code
                (ptr, 8, 8, 0, 0, 8, 8, prog([-1]), ptr, ptr),
                (ptr, 8, 8, 0, 0, 8, 8, prog([2, 2]), ptr, ptr),   # a step twice
                (ptr, 8, 8, 0, 0, 8, 8, prog([0, 1, 2, 3, 0]), ptr, ptr),      # five steps
                (ptr, 8, 8, 0, 0, 8, 8, prog([3], hue_byte=256), ptr, ptr),
                (ptr, 8, 8, 0, 0, 8, 8, prog([0], factors=(float("nan"), 1.0, 1.0)), ptr, ptr),    # no finite factor
                (ptr, 8, 8, 0, 0, 8, 8, prog([1, 2], factors=(1.0, 1.0, float("inf"))), ptr, ptr),
                (ptr, 8, 8, 0, 0, 8, 8, prog([3], factors=(1.0, float("-inf"), 1.0)), ptr, ptr),
                (ptr, 8, 8, 0, 0, 8, 8, ok, None, ptr)]:           # contrast and no counter
        assert calls(*bad) == (-1, -1, -1), bad[1:8]
    assert calls(ptr, 8, 8, 0, 0, 8, 8, ok, ptr, None)[1:] == (-1, -1)          # null output
    assert L.ssa_jitter_crop_flip_normalize(ptr, 8, 8, 0, 0, 8, 8, 0, ctypes.byref(ok), ptr, mean, std, ptr, 12, None) == -1
    assert L.ssa_jitter_crop_flip_normalize(ptr, 8, 8, 0, 0, 8, 8, 0, ctypes.byref(ok), ptr, None, std, ptr, 16, None) == -1
    # a program without a contrast step needs no counter: the luma sum is then no launch at all
    before = L.ssa_launch_count(0)
    assert L.ssa_jitter_luma_sum(ptr, 8, 8, 0, 0, 8, 8, ctypes.byref(prog([0, 3])), None, None) == 0
    assert L.ssa_launch_count(0) == before


def test_python_layer_rejects_bad_parameters():
    from semseg_amd.datasets import JitterParams, color_jitter
    import torch
    with pytest.raises(ValueError):
        JitterParams(("brightness", "brightness"))
    with pytest.raises(ValueError):
        JitterParams(("gamma",))
    with pytest.raises(TypeError):
        color_jitter(torch.zeros((4, 4, 3), dtype=torch.uint8), {"order": ()})
    for window in ((0, 0, 0, 4), (1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 4, -4)):
        with pytest.raises(ValueError):
            color_jitter(torch.zeros((4, 4, 3), dtype=torch.uint8), JitterParams(("brightness",)), window=window)
