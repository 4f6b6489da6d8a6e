"""RandomGaussianBlur without a GPU:
  * the NumPy restatement (tests/gblur_ref.py) against live scipy.ndimage.gaussian_filter, against scikit-image wherever it
    is installed (the pin of the wrapper assumption), and against the fixture recorded from the reference
    (tests/golden/gblur_golden.npz, make_golden_gblur.py);
  * the product's gaussian_taps / conversion table / RandomGaussianBlur.get_params against SciPy and the recorded draws;
  * the kernels of csrc/gblur.hip, compiled for the host (tools/emu, both storage builds), against the restatement, bit for
    bit.  The emulation build has no FMA target: these tests check indices, clamping, tiling and the order of the sums, NOT
    that the device code is free of contraction -- only tests/test_gblur_gpu.py can show that;
  * argument validation of the two entry points, and a dry run of the host glue on CPU tensors."""
import collections
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import gblur_cases as K
import gblur_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement and the host tables
def _scipy_blur(img, sigma):
    """RandomGaussianBlur.__call__ with skimage.filters.gaussian restated over live SciPy."""
    from scipy import ndimage
    out = ndimage.gaussian_filter(np.multiply(img, 1. / 255, dtype=np.float64), [sigma, sigma, 0], mode="nearest", cval=0,
                                  truncate=4.0)
    out *= 255
    return out.astype(np.uint8)


def test_restatement_equals_live_scipy():
    pytest.importorskip("scipy")
    assert [R.taps(s)[0] for s in K.SIGMAS] == K.RADII
    images = [K.image(h, w) for h, w in K.SHAPES] + [R.levels_image()]
    for sigma in K.SIGMAS + K.ONE_PER_RADIUS:
        for img in images:
            got, want = R.blur(img, sigma), _scipy_blur(img, sigma)
            assert np.array_equal(got, want), (sigma, img.shape, K.first_difference(got, want))


def test_restatement_equals_live_scikit_image():
    """The wrapper assumption, settled wherever scikit-image can be imported: the reference's own three lines."""
    filters = pytest.importorskip("skimage.filters")
    import inspect
    kw = ({"channel_axis": -1} if "channel_axis" in inspect.signature(filters.gaussian).parameters
          else {"multichannel": True})
    for sigma in K.SIGMAS:
        for img in [K.image(h, w) for h, w in K.SHAPES] + [R.levels_image()]:
            blurred = filters.gaussian(img, sigma=sigma, **kw)
            blurred *= 255
            assert np.array_equal(R.blur(img, sigma), blurred.astype(np.uint8)), (sigma, img.shape)


def test_levels_image_is_where_one_ulp_decides():
    """Many constant neighbourhoods leave the reference one grey level darker (the weights sum to 1 - ulp and the product
    is truncated): the pixels a fused multiply-add or another order of the sum moves."""
    img = R.levels_image()
    darker = 0
    for sigma in K.ONE_PER_RADIUS:
        out = R.blur(img, sigma)
        r = R.taps(sigma)[0]
        inner = np.zeros((16, 16), bool)
        inner[r:16 - r, r:16 - r] = True
        inner = np.tile(inner, (16, 16))
        diff = out[inner].astype(int) - img[inner].astype(int)
        assert set(np.unique(diff)) <= {-1, 0}, sigma
        darker += int((diff == -1).sum())
    assert darker > 0


def test_restatement_and_taps_equal_the_reference_fixture():
    from semseg_amd.datasets import gaussian_taps
    inputs, outputs, meta = R.load_golden()
    assert meta["skimage"] is None and "restated" in meta["wrapper"] and meta["scipy"] and meta["numpy"]
    assert len(inputs) >= 6 and sorted({e["radius"] for e in meta["entries"]}) == [1, 2, 3, 4, 5]
    assert any(img.shape[0] == 1 for img in inputs) and any((img == img[0, 0]).all() for img in inputs)
    for e, img, want in zip(meta["entries"], inputs, outputs):
        got = R.blur(img, e["sigma"])
        assert np.array_equal(got, want), (e["seed"], K.first_difference(got, want))
        radius, w = gaussian_taps(e["sigma"])
        assert radius == e["radius"] == R.taps(e["sigma"])[0]
        assert w.dtype == np.float64 and w.tolist() == e["weights"] == R.taps(e["sigma"])[1].tolist()


def test_gaussian_taps_equal_scipy_and_reject_other_radii():
    from semseg_amd.datasets import BlurParams, gaussian_taps
    from semseg_amd.datasets.transforms import byte_to_float64
    filt = pytest.importorskip("scipy.ndimage._filters")
    for sigma in K.SIGMAS + K.ONE_PER_RADIUS:
        radius, w = gaussian_taps(sigma)
        assert radius == int(4.0 * sigma + 0.5)
        assert np.array_equal(w, filt._gaussian_kernel1d(sigma, 0, radius)[::-1][radius:])
        tp = BlurParams(sigma).taps()
        assert tp.radius == radius and list(tp.w)[:radius + 1] == w.tolist() and all(v == 0 for v in list(tp.w)[radius + 1:])
    for bad in (0.12, 1.375, 3.0, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            gaussian_taps(bad)
    lut = byte_to_float64()
    assert lut.dtype == np.float64 and lut.shape == (256,)
    assert np.array_equal(lut, R.to_float64(np.arange(256, dtype=np.uint8))) and lut[255] == 1.0


def test_get_params_reproduces_the_recorded_draws():
    """One random.random() per call, as the reference: the same sigma to the bit, the same generator state afterwards."""
    from semseg_amd.datasets import RandomGaussianBlur
    for e in R.load_golden()[2]["entries"]:
        random.seed(e["seed"])
        p = RandomGaussianBlur.get_params()
        assert p.sigma == e["sigma"] and p.radius == e["radius"]
        assert random.random() == e["random_after"]


# ------------------------------------------------------------------ the kernels on the CPU emulation
@pytest.fixture()
def emu():
    from emu_util import emu_backend
    with emu_backend():
        yield "cpu"


def test_emulated_kernels_every_sigma_and_shape(emu):
    K.check_sigmas_and_shapes(emu)


def test_emulated_kernels_windows_smaller_than_the_radius(emu):
    K.check_small_windows_at_radius_5(emu)


def test_emulated_kernels_window_over_several_tiles(emu):
    K.check_window_over_several_tiles(emu)


def test_emulated_kernels_levels_image(emu):
    K.check_levels(emu, (0.3, 1.2999))


def test_emulated_kernels_reference_fixture(emu):
    K.check_fixture_entries(emu)


def test_emulated_fused_normalise_equals_two_steps(emu):
    K.check_fused_equals_two_steps(emu)


def test_emulated_jitter_then_blur(emu):
    K.check_jitter_then_blur(emu)


def test_emulated_random_gaussian_blur_call(emu):
    from semseg_amd.datasets import RandomGaussianBlur
    inputs, outputs, meta = R.load_golden()
    e = meta["entries"][0]
    random.seed(e["seed"])
    got = RandomGaussianBlur()(torch.from_numpy(inputs[0]))
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), outputs[0])


def test_emulated_kernels_on_the_other_storage_build():
    """The emulation library of the OTHER element type (fp16 storage when this process runs bf16), through the C ABI on
    NumPy buffers: the blur bytes equal the restatement, and the fused normalise equals that build's two steps."""
    from emu_util import _F16
    from semseg_amd import _lib
    subprocess.check_call(["sh", os.path.join(ROOT, "tools", "emu", "build.sh")] + ([] if _F16 else ["f16"]),
                          stdout=subprocess.DEVNULL)
    h = ctypes.CDLL(os.path.join(ROOT, "tools", "emu", "build" if _F16 else "build_f16", "libsemseg_emu.so"))
    for name in ("ssa_elem_type", "ssa_gblur_u8", "ssa_gblur_crop_flip_normalize", "ssa_image_u8_crop_flip_normalize",
                 "ssa_jitter_luma_sum"):
        getattr(h, name).argtypes, getattr(h, name).restype = _lib._SIGS[name]
    assert h.ssa_elem_type() == (0 if _F16 else 1)
    from semseg_amd.datasets import BlurParams
    from semseg_amd.datasets.transforms import MEAN_STD, byte_to_float64
    P = lambda a: ctypes.c_void_p(a.ctypes.data)              # noqa: E731
    lut = byte_to_float64()
    mean, std = (ctypes.c_float * 3)(*MEAN_STD[0]), (ctypes.c_float * 3)(*MEAN_STD[1])
    window = (7, 5, K.TILE_W + 5, K.TILE_H + 3)
    x0, y0, cw, ch = window
    src = K.hostile_source(window, K.TILE_H + 3 + 11, K.TILE_W + 5 + 16)
    H, W = src.shape[:2]
    pg = K.params(K.JITTER_DRAWS).program()
    counter = np.zeros(1, np.uint64)
    assert h.ssa_jitter_luma_sum(P(src), H, W, x0, y0, cw, ch, ctypes.byref(pg), P(counter), None) == 0
    import colorjit_ref as CR
    for sigma in K.ONE_PER_RADIUS:
        tp = BlurParams(sigma).taps()
        for flip in (0, 1):
            for prog in (None, ctypes.byref(pg)):
                u8 = np.zeros((ch, cw, 3), np.uint8)
                fused, two = np.zeros((ch, cw, 16), np.uint16), np.ones((ch, cw, 16), np.uint16)
                assert h.ssa_gblur_u8(P(src), H, W, x0, y0, cw, ch, flip, prog, P(counter), ctypes.byref(tp), P(lut), P(u8),
                                      None) == 0
                pre = src if prog is None else CR.jitter(src, CR.program_of(K.JITTER_DRAWS), window, bool(flip))
                want = R.blur(src, sigma, window, bool(flip)) if prog is None else R.blur(pre, sigma)
                assert np.array_equal(u8, want), (sigma, flip, K.first_difference(u8, want))
                assert h.ssa_gblur_crop_flip_normalize(P(src), H, W, x0, y0, cw, ch, flip, prog, P(counter), ctypes.byref(tp),
                                                       P(lut), mean, std, P(fused), 16, None) == 0
                assert h.ssa_image_u8_crop_flip_normalize(P(u8), ch, cw, 0, 0, cw, ch, 0, mean, std, P(two), 16, None) == 0
                assert np.array_equal(fused, two), (sigma, flip)


# ------------------------------------------------------------------ argument validation (the real library, no device)
def test_entry_points_reject_bad_arguments_without_gpu():
    from semseg_amd import _lib
    L = _lib.lib()
    P = ctypes.c_void_p
    buf = (ctypes.c_double * 1024)()                   # never read: every call below fails validation first
    ptr = P(ctypes.addressof(buf))
    mean, std = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.2, 0.2, 0.2)

    def taps(radius, w=(0.4, 0.2, 0.1, 0.0, 0.0, 0.0)):
        tp = _lib.GblurTaps()
        tp.radius = radius
        for j, v in enumerate(w):
            tp.w[j] = v
        return tp

    def prog(ops, hue_byte=0, factors=(1.0, 1.0, 1.0)):
        pg = _lib.JitterProgram()
        pg.n_ops = len(ops)
        for k, op in enumerate(ops[:4]):
            pg.op[k] = op
        pg.factor[0], pg.factor[1], pg.factor[2] = factors
        pg.hue_byte = hue_byte
        return pg

    def calls(img, H, W, x0, y0, cw, ch, pg, counter, tp, lut, out):
        pgp = None if pg is None else ctypes.byref(pg)
        tpp = None if tp is None else ctypes.byref(tp)
        return (L.ssa_gblur_u8(img, H, W, x0, y0, cw, ch, 0, pgp, counter, tpp, lut, out, None),
                L.ssa_gblur_crop_flip_normalize(img, H, W, x0, y0, cw, ch, 0, pgp, counter, tpp, lut, mean, std, out, 16, None))

    ok, t2 = prog([0, 1, 2, 3]), taps(2)
    before = L.ssa_launch_count(0)
    for bad in [(None, 8, 8, 0, 0, 8, 8, None, None, t2, ptr, ptr),            # null image
                (ptr, 8, 8, 0, 0, 8, 8, None, None, t2, ptr, None),            # null output
                (ptr, 8, 8, 0, 0, 8, 8, None, None, None, ptr, ptr),           # null taps
                (ptr, 8, 8, 0, 0, 8, 8, None, None, t2, None, ptr),            # null table
                (ptr, 8, 8, 1, 0, 8, 8, None, None, t2, ptr, ptr),             # window beyond the right edge
                (ptr, 8, 8, 0, 2, 8, 7, None, None, t2, ptr, ptr),             # ... beyond the bottom
                (ptr, 8, 8, -1, 0, 4, 4, None, None, t2, ptr, ptr),
                (ptr, 8, 8, 0, 0, 0, 4, None, None, t2, ptr, ptr),             # empty window
                (ptr, 0, 8, 0, 0, 1, 1, None, None, t2, ptr, ptr),
                (ptr, 8, 8, 0, 0, 8, 8, None, None, taps(0), ptr, ptr),        # radius outside 1..5
                (ptr, 8, 8, 0, 0, 8, 8, None, None, taps(6), ptr, ptr),
                (ptr, 8, 8, 0, 0, 8, 8, None, None, taps(-1), ptr, ptr),
                (ptr, 8, 8, 0, 0, 8, 8, None, None, taps(1, (float("nan"), 0, 0, 0, 0, 0)), ptr, ptr),
                (ptr, 8, 8, 0, 0, 8, 8, prog([0, 7]), ptr, t2, ptr, ptr),      # invalid programs
                (ptr, 8, 8, 0, 0, 8, 8, prog([2, 2]), ptr, t2, ptr, ptr),
                (ptr, 8, 8, 0, 0, 8, 8, prog([0, 1, 2, 3, 0]), ptr, t2, ptr, ptr),
                (ptr, 8, 8, 0, 0, 8, 8, prog([3], hue_byte=256), ptr, t2, ptr, ptr),
                (ptr, 8, 8, 0, 0, 8, 8, prog([0], factors=(float("nan"), 1.0, 1.0)), ptr, t2, ptr, ptr),
                (ptr, 8, 8, 0, 0, 8, 8, ok, None, t2, ptr, ptr)]:              # contrast and no counter
        assert calls(*bad) == (-1, -1), bad[1:7]
    def fused(cpad=16, mean=mean, std=std):            # otherwise valid arguments: only the fused entry point is called
        return L.ssa_gblur_crop_flip_normalize(ptr, 8, 8, 0, 0, 8, 8, 0, None, None, ctypes.byref(t2), ptr, mean, std, ptr,
                                               cpad, None)
    for cpad in (8, 24, 32, 0):
        assert fused(cpad=cpad) == -1, cpad
    assert fused(mean=None) == -1 and fused(std=None) == -1
    assert fused(std=(ctypes.c_float * 3)(0.2, 0.0, 0.2)) == -1
    assert L.ssa_launch_count(0) == before


def test_python_layer_rejects_bad_parameters():
    from semseg_amd.datasets import BlurParams, gaussian_blur
    img = torch.zeros((4, 4, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        BlurParams(2.0)
    with pytest.raises(ValueError):
        gaussian_blur(img, 1.5)
    with pytest.raises(ValueError):
        gaussian_blur(torch.zeros((4, 4, 3)), 0.5)
    with pytest.raises(TypeError):
        gaussian_blur(img, 0.5, jitter={"order": ()})
    for window in ((0, 0, 0, 4), (1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 4, -4)):
        with pytest.raises(ValueError):
            gaussian_blur(img, 0.5, window=window)


# ------------------------------------------------------------------ dry run of the host glue on CPU tensors
LAUNCHING = ("ssa_image_u8_crop_flip_normalize", "ssa_label_u8_crop_flip", "ssa_jitter_luma_sum", "ssa_jitter_apply_u8",
             "ssa_jitter_crop_flip_normalize", "ssa_gblur_u8", "ssa_gblur_crop_flip_normalize")


class DryLib:
    """The real library with the launching entry points replaced by stand-ins that check every call against the ctypes
    signature declared in semseg_amd/_lib.py, record it and return 0 (the pattern of tests/test_adam_glue_dryrun_cpu.py)."""

    def __init__(self, real):
        self._real = real
        self.order = []
        self.args = collections.defaultdict(list)

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in LAUNCHING:
            return fn
        argtypes = fn.argtypes

        def launch(*args):
            assert len(args) == len(argtypes), "%s: %d arguments for %d parameters" % (name, len(args), len(argtypes))
            for i, (t, a) in enumerate(zip(argtypes, args)):
                try:
                    t.from_param(a)
                except (ctypes.ArgumentError, TypeError) as e:
                    raise AssertionError("%s: argument %d (%r) does not convert to %s: %s" % (name, i, a, t, e))
            self.order.append(name)
            self.args[name].append(args)
            return 0
        return launch


class _OnDevice(torch.Tensor):
    """A CPU tensor that answers is_cuda as a device tensor does: crop_flip_normalize asserts it of its inputs."""
    is_cuda = property(lambda self: True)


@pytest.fixture()
def dry(monkeypatch):
    from semseg_amd import _lib, hip_backend as hb
    d = DryLib(_lib.lib())
    monkeypatch.setattr(_lib, "_LIB", d)
    monkeypatch.setattr(hb, "_s", lambda: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: collections.namedtuple("S", "cuda_stream")(0))
    return d


def _ptr(v):
    return v.value if isinstance(v, ctypes.c_void_p) else v


def test_dry_run_blur_none_launches_what_the_parent_launches(dry):
    from semseg_amd.datasets import crop_flip_normalize
    img = torch.zeros((20, 30, 3), dtype=torch.uint8).as_subclass(_OnDevice)
    lab = torch.zeros((20, 30), dtype=torch.uint8).as_subclass(_OnDevice)
    out, gts = crop_flip_normalize(img, lab, (3, 5, 17, 11), True)
    assert dry.order == ["ssa_image_u8_crop_flip_normalize", "ssa_label_u8_crop_flip"]
    a = dry.args["ssa_image_u8_crop_flip_normalize"][0]
    assert (_ptr(a[0]), *a[1:8]) == (img.data_ptr(), 20, 30, 3, 5, 17, 11, 1) and a[11] == 16
    assert [round(v, 3) for v in a[8]] == [0.485, 0.456, 0.406] and _ptr(a[10]) == out.data_ptr()
    assert tuple(out.shape) == (1, 11, 17, 16) and tuple(gts.shape) == (1, 11, 17)
    dry.order.clear()
    crop_flip_normalize(img, lab, (3, 5, 17, 11), True, jitter=K.params(K.JITTER_DRAWS), blur=None)
    assert dry.order == ["ssa_jitter_luma_sum", "ssa_jitter_crop_flip_normalize", "ssa_label_u8_crop_flip"]
    dry.order.clear()
    crop_flip_normalize(img, None, (3, 5, 17, 11), False, jitter=K.params([("hue", 0.1)]))
    assert dry.order == ["ssa_jitter_crop_flip_normalize"]


def test_dry_run_blur_launches_with_well_formed_arguments(dry):
    from semseg_amd.datasets import BlurParams, RandomGaussianBlur, crop_flip_normalize, gaussian_blur
    from semseg_amd.datasets.transforms import byte_to_float64
    from semseg_amd import hip_backend as hb
    img = torch.zeros((20, 30, 3), dtype=torch.uint8).as_subclass(_OnDevice)
    lab = torch.zeros((20, 30), dtype=torch.uint8).as_subclass(_OnDevice)
    b = BlurParams(0.7)
    out, gts = crop_flip_normalize(img, lab, (3, 5, 17, 11), True, blur=b)
    assert dry.order == ["ssa_gblur_crop_flip_normalize", "ssa_label_u8_crop_flip"]
    a = dry.args["ssa_gblur_crop_flip_normalize"][0]
    assert (_ptr(a[0]), *a[1:8]) == (img.data_ptr(), 20, 30, 3, 5, 17, 11, 1)
    assert a[8] is None and a[9] is None                                       # no program, no counter
    tp = a[10]._obj
    assert tp.radius == 3 == b.radius and list(tp.w)[:4] == b.weights.tolist() and list(tp.w)[4:] == [0.0, 0.0]
    lut = (ctypes.c_double * 256).from_address(_ptr(a[11]))
    assert list(lut) == byte_to_float64().tolist()
    assert [round(v, 3) for v in a[13]] == [0.229, 0.224, 0.225] and _ptr(a[14]) == out.data_ptr() and a[15] == 16
    assert out.dtype == hb.ACT_DTYPE and tuple(out.shape) == (1, 11, 17, 16) and out.data_ptr() % 16 == 0
    assert tuple(gts.shape) == (1, 11, 17) and dry.args["ssa_label_u8_crop_flip"][0][1:8] == (20, 30, 3, 5, 17, 11, 1)
    # with a jitter: the luma sum first, on the same window, its counter handed on; the table is uploaded once
    dry.order.clear()
    p = K.params(K.JITTER_DRAWS)
    crop_flip_normalize(img, lab, (3, 5, 17, 11), False, jitter=p, blur=b)
    assert dry.order == ["ssa_jitter_luma_sum", "ssa_gblur_crop_flip_normalize", "ssa_label_u8_crop_flip"]
    s, a2 = dry.args["ssa_jitter_luma_sum"][-1], dry.args["ssa_gblur_crop_flip_normalize"][-1]
    assert s[1:7] == a2[1:7] == (20, 30, 3, 5, 17, 11) and a2[7] == 0
    assert _ptr(s[8]) == _ptr(a2[9]) and _ptr(a2[9]) % 8 == 0 and _ptr(a2[11]) == _ptr(a[11])
    pg = a2[8]._obj
    assert pg.n_ops == 4 and list(pg.op) == [0, 1, 3, 2]
    # a program without contrast: no luma sum, no counter
    dry.order.clear()
    crop_flip_normalize(img, None, (3, 5, 17, 11), False, jitter=K.params([("hue", 0.1)]), blur=0.3)
    assert dry.order == ["ssa_gblur_crop_flip_normalize"]
    a3 = dry.args["ssa_gblur_crop_flip_normalize"][-1]
    assert a3[9] is None and a3[8]._obj.n_ops == 1 and a3[10]._obj.radius == 1
    # the uint8 form, whole image, and the transform object
    dry.order.clear()
    u8 = gaussian_blur(img, b)
    random.seed(2)
    u8b = RandomGaussianBlur()(img)
    assert dry.order == ["ssa_gblur_u8", "ssa_gblur_u8"]
    g = dry.args["ssa_gblur_u8"]
    assert g[0][1:8] == (20, 30, 0, 0, 30, 20, 0) and _ptr(g[0][12]) == u8.data_ptr() and g[1][10]._obj.radius == 5
    assert u8.dtype == u8b.dtype == torch.uint8 and tuple(u8.shape) == tuple(u8b.shape) == (20, 30, 3)
