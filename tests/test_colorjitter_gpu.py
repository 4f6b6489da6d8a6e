"""The device ColorJitter (csrc/color_jitter.hip through semseg_amd.datasets) against the CPU restatement of the reference's
chain (tests/colorjit_ref.py, pinned to Pillow and to the reference by tests/test_colorjitter_cpu.py) and against the
fixture tests/golden/colorjitter_golden.npz.  Every comparison is exact (array equality or a SHA-256); neither Pillow nor
the reference is needed here."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import colorjit_cases as K
import colorjit_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cube():
    return R.all_colours()


@pytest.fixture(scope="module")
def cube_dev(cube):
    return torch.from_numpy(cube).to(DEV)


def _exhaustive_cases():
    return [("brightness", f) for f in (0.75, 1.0, 1.25, 1.9)] + [("saturation", f) for f in (0.75, 1.0, 1.25, 1.9)] + [
        ("hue", b) for b in (0, 1, 63, 193, 255)]


@pytest.mark.parametrize("op,value", _exhaustive_cases())
def test_per_pixel_operations_on_every_colour(cube, cube_dev, op, value):
    """All 2^24 colours through one operation: the SHA-256 of the device output is the one recorded from Pillow."""
    from semseg_amd.datasets import JitterParams, color_jitter
    p = JitterParams(("hue",), hue_byte=value) if op == "hue" else JitterParams((op,), **{op: value})
    got = color_jitter(cube_dev, p).cpu().numpy()
    want_sha = R.load_golden()[2]["hashes"]["%s:%r" % (op, value)]
    if hashlib.sha256(got.tobytes()).hexdigest() != want_sha:
        for i in range(0, 4096, 256):               # which colour: ask the restatement, strip by strip
            want = R.apply_op(cube[i:i + 256], op, value)
            assert np.array_equal(got[i:i + 256], want), (op, value, K.first_difference(got[i:i + 256], want, cube[i:i + 256]))
        raise AssertionError("%s %r: the device output equals the restatement but not the recorded hash" % (op, value))


@pytest.mark.parametrize("op,value", [("brightness", 0.8123456), ("saturation", 0.8123456), ("contrast", 0.8),
                                      ("contrast", 1.1)])
def test_blends_with_inexact_factors_on_every_colour(cube, cube_dev, op, value):
    """Factors that are no short binary fraction: the product f * (x - d) is then inexact, and a multiply-add fused into
    one rounding differs from Pillow's two (0.8 * -145 + 147 = 30.999998 -> 30 instead of 31).  The recorded hashes are at
    0.75, 1.0, 1.25 and 1.9; the expected bytes here come from the restatement.  Contrast: the mean is over the cube."""
    from semseg_amd.datasets import JitterParams, color_jitter
    got = color_jitter(cube_dev, JitterParams((op,), **{op: value})).cpu().numpy()
    mean = R.contrast_mean(cube) if op == "contrast" else None
    for i in range(0, 4096, 512):
        src = cube[i:i + 512]
        want = R.contrast(src, value, mean=mean) if op == "contrast" else R.apply_op(src, op, value)
        assert np.array_equal(got[i:i + 512], want), (op, value, K.first_difference(got[i:i + 512], want, src))


def test_chains_of_the_reference_fixture():
    K.check_fixture_entries(DEV)


def test_chains_in_all_24_orders():
    K.check_all_orders(DEV)


def test_programs_of_zero_to_three_operations_and_contrast_first_and_last():
    K.check_short_programs(DEV)


def test_adjust_functions_and_colorjitter_call():
    """The reference's function names on device images; ColorJitter.__call__ draws from np.random as recorded."""
    from semseg_amd.datasets import ColorJitter, adjust_brightness, adjust_contrast, adjust_hue, adjust_saturation
    images, outputs, meta = R.load_golden()
    img = images[1]
    t = torch.from_numpy(img).to(DEV)
    assert np.array_equal(adjust_brightness(t, 1.1).cpu().numpy(), R.brightness(img, 1.1))
    assert np.array_equal(adjust_contrast(t, 0.9).cpu().numpy(), R.contrast(img, 0.9))
    assert np.array_equal(adjust_saturation(t, 0.0).cpu().numpy(), R.saturation(img, 0.0))
    assert np.array_equal(adjust_hue(t, -0.25).cpu().numpy(), R.hue(img, 193))
    for e, want in list(zip(meta["entries"], outputs))[:4]:
        np.random.seed(e["seed"])
        got = ColorJitter(*e["args"])(torch.from_numpy(images[e["image"]]).to(DEV))
        assert np.array_equal(got.cpu().numpy(), want), e["seed"]


def test_contrast_mean_rounding():
    K.check_mean_rounding(DEV)


def test_reduction_one_row_of_257_and_full_size_frame():
    """1 x 257: a second workgroup holding one pixel.  1024 x 2048: the grid-stride loop (4096 workgroups of 256 cover
    half of it per sweep) and one atomic per workgroup; twice, for the identical result."""
    from semseg_amd.datasets import color_jitter
    rng = np.random.RandomState(2)
    K.check_chain(DEV, rng.randint(0, 256, (1, 257, 3)).astype(np.uint8), K.draws_of(("brightness", "contrast", "hue")))
    big = rng.randint(0, 256, (1024, 2048, 3)).astype(np.uint8)
    draws = K.draws_of(("saturation", "brightness", "contrast", "hue"))
    want = R.jitter(big, R.program_of(draws))
    t = torch.from_numpy(big).to(DEV)
    first = color_jitter(t, K.params(draws))
    second = color_jitter(t, K.params(draws))
    assert np.array_equal(first.cpu().numpy(), want), K.first_difference(first.cpu().numpy(), want, big)
    assert torch.equal(first, second)


def test_luma_sum_beyond_32_bits():
    """All-white 4200 x 4200: the luma sum is 4 498 200 000 > 2^32.  m must be 255 and contrast leave the image white; a
    32-bit accumulator gives m = 12 and 133."""
    from semseg_amd.datasets import color_jitter
    n = 4200 * 4200
    assert 255 * n == 4498200000 > 2 ** 32 and int(float(255 * n) / float(n) + 0.5) == 255
    assert int(float(255 * n % 2 ** 32) / float(n) + 0.5) == 12
    assert R.contrast(np.full((1, 1, 3), 255, np.uint8), 0.5, mean=255).tolist() == [[[255, 255, 255]]]
    white = torch.full((4200, 4200, 3), 255, dtype=torch.uint8, device=DEV)
    out = color_jitter(white, K.params([("contrast", 0.5)]))
    lo = int(out.min())
    assert lo == 255, "contrast mean %s instead of 255" % (2 * lo - 255)


def test_window_and_flip():
    K.check_windows(DEV)


def test_fused_tail_equals_jitter_then_tail():
    """crop_flip_normalize(img, labels, window, flip, jitter=p) == crop_flip_normalize(color_jitter(img, p, window, flip),
    None, (0, 0, w, h), False) bit for bit, in this build's storage format; the labels are today's."""
    from semseg_amd.datasets import color_jitter, crop_flip_normalize
    K.check_fused_equals_two_steps(DEV)
    src = K.window_source()
    lab = np.random.RandomState(8).randint(0, 256, src.shape[:2]).astype(np.uint8)
    t, tl = torch.from_numpy(src).to(DEV), torch.from_numpy(lab).to(DEV)
    p = K.params(K.draws_of(("hue", "contrast", "brightness", "saturation")))
    for window, flip in K.WINDOW_CASES:
        fused, gts = crop_flip_normalize(t, tl, window, flip, jitter=p)
        two, none = crop_flip_normalize(color_jitter(t, p, window, flip), None, (0, 0, window[2], window[3]), False)
        assert none is None and fused.shape == two.shape and fused.dtype == two.dtype
        assert torch.equal(fused.view(torch.int16), two.view(torch.int16)), (window, flip)
        assert torch.equal(gts, crop_flip_normalize(t, tl, window, flip)[1])


def test_normalise_store_at_8_and_24_padded_channels():
    K.check_padded_store(DEV)


def test_fused_tail_on_the_other_storage_build():
    """The same test in a child process on the other build of the library (fp16 storage when this one is bf16)."""
    from semseg_amd import _lib
    other = "fp16" if _lib.ACT == "bf16" else "bf16"
    env = dict(os.environ, SSA_ACT_DTYPE=other)
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_colorjitter_gpu.py"), "-k", "test_fused_tail_equals_jitter_then_tail"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    tail = r.stdout[-3000:]
    assert r.returncode == 0, "fused tail under SSA_ACT_DTYPE=%s:\n%s\n%s" % (other, tail, r.stderr[-2000:])
    assert "1 passed" in tail, tail


def test_jitter_none_is_todays_launches_and_output():
    """jitter=None: the two launches of today (image, labels) and the oracle's values, bit for bit."""
    from oracle.data import crop_flip_normalize as oracle
    from semseg_amd import _lib
    from semseg_amd.datasets.transforms import MEAN_STD, crop_flip_normalize
    from util import ACT_DTYPE
    src = K.window_source()
    lab = np.random.RandomState(8).randint(0, 256, src.shape[:2]).astype(np.uint8)
    t, tl = torch.from_numpy(src).to(DEV), torch.from_numpy(lab).to(DEV)
    for window, flip in K.WINDOW_CASES:
        _lib.lib().ssa_launch_count(1)
        out, gts = crop_flip_normalize(t, tl, window, flip, jitter=None)
        assert _lib.lib().ssa_launch_count(0) == 2
        plain, gts2 = crop_flip_normalize(t, tl, window, flip)
        want_im, want_lab = oracle(src, lab, window, flip, *MEAN_STD)
        want = torch.from_numpy(want_im).permute(1, 2, 0).to(ACT_DTYPE).contiguous()
        assert torch.equal(out.view(torch.int16), plain.view(torch.int16)) and torch.equal(gts, gts2)
        assert torch.equal(out[0].cpu()[..., :3].contiguous().view(torch.int16), want.view(torch.int16)), window
        assert torch.equal(gts[0].cpu(), torch.from_numpy(want_lab))
    _lib.lib().ssa_launch_count(1)
    crop_flip_normalize(t, tl, (3, 5, 37, 29), True, jitter=K.params(K.draws_of(("contrast", "hue"))))
    assert _lib.lib().ssa_launch_count(0) == 4          # clear + luma sum, fused apply, labels
    _lib.lib().ssa_launch_count(1)
    crop_flip_normalize(t, tl, (3, 5, 37, 29), True, jitter=K.params(K.draws_of(("saturation", "hue"))))
    assert _lib.lib().ssa_launch_count(0) == 2          # no contrast step: no luma sum


def test_captured_pair_reads_the_mean_on_the_device():
    """Luma sum + fused apply captured in a graph, replayed after another image was copied into the same buffer: the
    output is that image's, with that image's contrast mean -- the mean never passed through the host."""
    from semseg_amd.datasets.transforms import crop_flip_normalize
    a = K.window_source()
    b = (K.window_source() // 3 + 150).astype(np.uint8)
    window, flip = (3, 5, 37, 29), True
    draws = K.draws_of(("brightness", "contrast", "saturation", "hue"))
    p = K.params(draws)
    crop = lambda im: R.apply_op(im[5:34, 3:40], "brightness", 1.2)         # noqa: E731  (what contrast averages)
    assert R.contrast_mean(crop(a)) != R.contrast_mean(crop(b))
    want_a = crop_flip_normalize(torch.from_numpy(a).to(DEV), None, window, flip, jitter=p)[0].clone()
    want_b = crop_flip_normalize(torch.from_numpy(b).to(DEV), None, window, flip, jitter=p)[0].clone()
    assert not torch.equal(want_a.view(torch.int16), want_b.view(torch.int16))
    buf = torch.from_numpy(a).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        crop_flip_normalize(buf, None, window, flip, jitter=p)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = crop_flip_normalize(buf, None, window, flip, jitter=p)[0]
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), want_a.view(torch.int16))
    buf.copy_(torch.from_numpy(b).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), want_b.view(torch.int16))
