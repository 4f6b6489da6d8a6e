"""RandAugment without a GPU:
  * the NumPy restatement (tests/randaug_ref.py) against live Pillow, operation by operation, and against the fixture
    recorded from the reference (tests/golden/randaugment_golden.npz, make_golden_randaugment.py);
  * RandAugment.get_params against the recorded draws and generator states;
  * the kernels of csrc/randaugment.hip, compiled for the host (tools/emu, both storage builds), against the restatement,
    bit for bit.  The emulation build has no FMA target: these tests check indices, clamping, tiling, the tables and the
    order of the sums, NOT that the device code is free of contraction -- only tests/test_randaugment_gpu.py shows that;
  * argument validation of the entry point and of the Python layer, and a dry run of the host glue on CPU tensors.
Everything is compared byte for byte, and every test asserts how many cases it ran."""
import collections
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import randaug_cases as K
import randaug_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement against live Pillow
def _pillow(img, lab, op, v, fill_label=255):
    """The reference's operation with the sign already in v (datasets/randaugment.py:16-142)."""
    from PIL import Image, ImageEnhance, ImageOps
    pi, pl = Image.fromarray(img), Image.fromarray(lab)
    if op in ("ShearX", "ShearY", "TranslateX", "TranslateY"):
        a = R.matrix_of(op, v, *pi.size)
        pi = pi.transform(pi.size, Image.AFFINE, a, resample=Image.BILINEAR, fillcolor=(0, 0, 0))
        pl = pl.transform(pl.size, Image.AFFINE, a, resample=Image.NEAREST, fillcolor=fill_label)
    elif op == "Rotate":
        pi, pl = pi.rotate(v, fillcolor=(0, 0, 0)), pl.rotate(v, resample=Image.NEAREST, fillcolor=fill_label)
    elif op == "AutoContrast":
        pi = ImageOps.autocontrast(pi)
    elif op == "Invert":
        pi = ImageOps.invert(pi)
    elif op == "Equalize":
        pi = ImageOps.equalize(pi)
    elif op == "Solarize":
        pi = ImageOps.solarize(pi, v)
    elif op == "Posterize":
        pi = ImageOps.posterize(pi, int(v))
    elif op == "Color":
        pi = ImageEnhance.Color(pi).enhance(v)
    elif op == "Brightness":
        pi = ImageEnhance.Brightness(pi).enhance(v)
    elif op == "Sharpness":
        pi = ImageEnhance.Sharpness(pi).enhance(v)
    else:
        assert op == "Identity"
    return np.array(pi), np.array(pl)


def _pin(img, lab, program):
    (op, v), = program
    lab = R.label_map(img.shape[0], img.shape[1], 1) if lab is None else lab
    gi, gl = R.apply_op(img, lab, op, v)
    wi, wl = _pillow(img, lab, op, v)
    assert np.array_equal(gi, wi), (op, v, img.shape, K.first_difference(gi, wi))
    assert np.array_equal(gl, wl), (op, v, img.shape, K.first_difference(gl, wl))
    return 1


def test_restatement_equals_live_pillow_on_every_op():
    pytest.importorskip("PIL")
    z, _ = R.load_golden()
    n = 0
    for k in (0, 1):
        for program in K.per_op_programs(53, 37):
            n += _pin(z["images"][k], z["labels"][k], program)
    assert n == 190


def test_restatement_equals_live_pillow_on_the_special_images():
    pytest.importorskip("PIL")
    n = 0
    for img in (K.narrow_image(), K.one_value_band_image(), K.step_zero_image(), K.all_values_image()):
        for program in ([("AutoContrast", 0.0)], [("Equalize", 0.0)], [("Invert", 0.0)], [("Solarize", 33.0)],
                        [("Solarize", 110.0)], [("Posterize", 4)], [("Posterize", 6)], [("Posterize", 8)],
                        [("Color", 0.1)], [("Color", 1.9)], [("Brightness", 0.1)], [("Brightness", 1.9)]):
            n += _pin(img, None, program)
    for img in (R.levels_image(), R.checkerboard(), K.image(37, 53)):
        for v in K.SHARP:
            n += _pin(img, None, [("Sharpness", v)])
    assert n == 4 * 12 + 9
    # and every operation at every magnitude and sign over each of them, the warps included
    n = 0
    for img in (K.narrow_image(), K.one_value_band_image(), K.step_zero_image(), K.all_values_image(), R.levels_image(),
                R.checkerboard()):
        for program in K.per_op_programs(img.shape[1], img.shape[0]):
            n += _pin(img, None, program)
    assert n == 6 * 95


def test_equalize_table_clips_and_the_branches_are_reached():
    """The fixture-sized image reaches table entries above 255 (a wrapping restatement would differ); the special images
    reach the identity branches they were built for."""
    z, _ = R.load_golden()
    h = R.histogram(z["images"][0])
    step = (int(h[0].sum()) - int(h[0][np.nonzero(h[0])[0][-1]])) // 255
    assert step > 0 and (step // 2 + int(h[0][:255].sum())) // step > 255
    assert all(np.array_equal(R.equalize_lut(hh), np.arange(256)) for hh in R.histogram(K.step_zero_image()))
    one = R.histogram(K.one_value_band_image())
    assert np.array_equal(R.equalize_lut(one[1]), np.arange(256)) and np.array_equal(R.autocontrast_lut(one[1]), np.arange(256))
    nar = R.histogram(K.narrow_image())
    assert R.autocontrast_lut(nar[0])[60] == 0 and R.autocontrast_lut(nar[0])[190] == 255
    assert np.array_equal(R.autocontrast_lut(nar[2]), np.arange(256))


def test_label_translations_follow_pillows_scale_routine():
    """Live Pillow sends a matrix with a1 == a3 == 0 to its scale routine under NEAREST (a double running sum, truncated,
    negative = outside), not to the 16.16 fixed-point path: the restatement follows it, and the offsets of the table are
    ones at which the two rules give different label maps."""
    Image = pytest.importorskip("PIL.Image")
    n = disagree = 0
    for w in (53, 64):
        lab = R.label_map(37, w, 7)
        pl = Image.fromarray(lab)
        for off in K.TRANSLATION_OFFSETS:
            for a in ([1, 0, off, 0, 1, 0], [1, 0, 0, 0, 1, off]):
                want = np.array(pl.transform(pl.size, Image.AFFINE, a, resample=Image.NEAREST, fillcolor=255))
                assert np.array_equal(R.warp_nearest(lab, a, 255), want), (w, a)
                disagree += not np.array_equal(R.warp_nearest_fixed(lab, a, 255), want)
                n += 1
    wide = R.label_map(2, 1100, 3)
    pl = Image.fromarray(wide)
    for off in (-300.5 + 1e-9, -0.3 - 2.0 ** -30, 0.7 / 3, 17.123456789, -1.0 - 1e-12):
        a = [1, 0, off, 0, 1, 0]
        want = np.array(pl.transform(pl.size, Image.AFFINE, a, resample=Image.NEAREST, fillcolor=255))
        assert np.array_equal(R.warp_nearest(wide, a, 255), want), off
        n += 1
    assert n == 2 * len(K.TRANSLATION_OFFSETS) * 2 + 5 and disagree >= 16


# ------------------------------------------------------------------ the fixture recorded from the reference
def test_restatement_equals_the_reference_fixture():
    z, meta = R.load_golden()
    assert meta["pillow"] and meta["numpy"] and meta["ignore_label"] == 255
    assert z["images"].shape == (2, 37, 53, 3) and z["labels"].shape == (2, 37, 53) and int(z["labels"].max()) == 18
    assert len(meta["ops"]) == 95 and len(meta["chains"]) == 32
    assert sorted({e["op"] for e in meta["ops"]}) == sorted(R.OPS)
    n = 0
    for e in meta["ops"]:
        assert e["m"] in K.MAGNITUDES
        if e["op"] in R.GEOMETRIC:
            random.seed(e["seed"])
            assert (random.random() > 0.5) == e["negated"]
        program = [(e["op"], K.signed_value(e["op"], e["m"], bool(e["negated"]), 53, 37))]
        gi, gl = R.augment(z["images"][e["image"]], z["labels"][e["image"]], program, fill_label=meta["ignore_label"])
        wi, wl = z["out_images"][e["out_image"]], z["out_labels"][e["out_label"]]
        assert np.array_equal(gi, wi), (e, K.first_difference(gi, wi))
        assert np.array_equal(gl, wl), (e, K.first_difference(gl, wl))
        n += 1
    for e in meta["chains"]:
        assert len(e["program"]) == e["n"]
        gi, gl = R.augment(z["images"][e["image"]], z["labels"][e["image"]], [tuple(s) for s in e["program"]],
                           fill_label=meta["ignore_label"])
        wi, wl = z["out_images"][e["out_image"]], z["out_labels"][e["out_label"]]
        assert np.array_equal(gi, wi), (e["seed"], e["program"], K.first_difference(gi, wi))
        assert np.array_equal(gl, wl), (e["seed"], e["program"], K.first_difference(gl, wl))
        n += 1
    assert n == 127


def test_get_params_reproduces_the_recorded_draws():
    """The same program to the bit and the same generator state afterwards, for every chain of the fixture and for the
    single operations (whose sign draw is the operation's own)."""
    from semseg_amd.datasets import AugmentParams, RandAugment
    _, meta = R.load_golden()
    n = 0
    for e in meta["chains"]:
        random.seed(e["seed"])
        p = RandAugment(e["n"], e["m"]).get_params((53, 37))
        assert isinstance(p, AugmentParams) and p.size == (53, 37)
        assert [[op, v] for op, v in p.ops] == e["program"], (e["seed"], p.ops, e["program"])
        assert random.random() == e["random_after"], e["seed"]
        pg = p.program()
        assert pg.n_ops == e["n"] and [R.OPS[pg.op[k]] for k in range(pg.n_ops)] == [s[0] for s in e["program"]]
        assert [pg.value[k] for k in range(pg.n_ops)] == [float(s[1]) for s in e["program"]]
        n += 1
    assert n == 32
    assert {s[0] for e in meta["chains"] for s in e["program"]} >= set(R.GEOMETRIC)


def test_python_layer_rejects_bad_parameters():
    from semseg_amd.datasets import AugmentParams, RandAugment, crop_flip_normalize, rand_augment
    img = torch.zeros((4, 6, 3), dtype=torch.uint8)
    ok = AugmentParams([("Invert", 0.0)], (6, 4))
    for m in (-1, 30.5, 31):
        with pytest.raises(ValueError):
            RandAugment(2, m).get_params((6, 4))
    state = random.getstate()
    with pytest.raises(ValueError):
        RandAugment(2, 31).get_params((6, 4))
    assert random.getstate() == state                                   # nothing drawn before the refusal
    with pytest.raises(ValueError):
        AugmentParams([("Contrast", 1.0)], (6, 4))
    with pytest.raises(ValueError):
        AugmentParams([("Posterize", 3)], (6, 4))
    with pytest.raises(ValueError):
        AugmentParams([("Invert", 0.0)] * 9, (6, 4))
    with pytest.raises(TypeError):
        rand_augment(img, None, [("Invert", 0.0)])
    with pytest.raises(TypeError):
        rand_augment(img, None, {"ops": ()})
    with pytest.raises(ValueError):
        rand_augment(torch.zeros((4, 6, 3)), None, ok)
    with pytest.raises(ValueError):
        rand_augment(img, torch.zeros((4, 5), dtype=torch.uint8), ok)
    with pytest.raises(ValueError):
        rand_augment(img, None, AugmentParams([("Invert", 0.0)], (5, 4)))    # drawn for another size
    for window in ((0, 0, 0, 4), (1, 0, 6, 4), (0, -1, 6, 4), (0, 0, 6, -4)):
        with pytest.raises(ValueError):
            rand_augment(img, None, ok, window=window)
    with pytest.raises(TypeError):
        crop_flip_normalize(img.as_subclass(_OnDevice), None, (0, 0, 6, 4), False, augment=[("Invert", 0.0)])


# ------------------------------------------------------------------ the kernels on the CPU emulation
@pytest.fixture()
def emu():
    from emu_util import emu_backend
    with emu_backend():
        yield "cpu"


def test_emulated_kernels_every_op(emu):
    assert K.check_every_op_on_the_fixture_images(emu) == 95


def test_emulated_kernels_tables_and_point_ops(emu):
    assert K.check_table_ops_on_special_images(emu) == 20


def test_emulated_kernels_sharpness_images(emu):
    assert K.check_sharpness_images(emu) == 6


def test_emulated_kernels_label_translations(emu):
    assert K.check_label_translations(emu) == 106


def test_emulated_kernels_reference_fixture_chains(emu):
    assert K.check_fixture_chains(emu) == 32


def test_emulated_kernels_window_inside_a_larger_source(emu):
    assert K.check_window_inside_a_larger_source(emu) == 18


def test_emulated_kernels_window_over_several_tiles(emu):
    assert K.check_window_over_several_tiles(emu) == 12


def test_emulated_kernels_tiny_windows(emu):
    assert K.check_tiny_windows(emu) == 36


def test_emulated_kernels_labels_absent(emu):
    assert K.check_labels_absent(emu) == 9


def test_emulated_fused_tail_equals_the_steps_in_sequence(emu, monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: collections.namedtuple("S", "cuda_stream")(0))
    assert K.check_tail_equals_steps_in_sequence(emu) == 4


def test_emulated_rand_augment_call(emu):
    z, meta = R.load_golden()
    from semseg_amd.datasets import RandAugment
    e = meta["chains"][9]
    random.seed(e["seed"])
    gi, gl = RandAugment(e["n"], e["m"])(torch.from_numpy(z["images"][e["image"]]), torch.from_numpy(z["labels"][e["image"]]))
    assert np.array_equal(gi.numpy(), z["out_images"][e["out_image"]])
    assert np.array_equal(gl.numpy(), z["out_labels"][e["out_label"]])
    assert random.random() == e["random_after"]


def test_emulated_kernels_on_the_other_storage_build():
    """The emulation library of the OTHER element type (fp16 storage when this process runs bf16), through the C ABI on
    NumPy buffers: one chain with a warp of both buffers, a table and the stencil, in a window, mirrored."""
    from emu_util import _F16
    from semseg_amd import _lib
    subprocess.check_call(["sh", os.path.join(ROOT, "tools", "emu", "build.sh")] + ([] if _F16 else ["f16"]),
                          stdout=subprocess.DEVNULL)
    h = ctypes.CDLL(os.path.join(ROOT, "tools", "emu", "build" if _F16 else "build_f16", "libsemseg_emu.so"))
    for name in ("ssa_elem_type", "ssa_randaug_u8"):
        getattr(h, name).argtypes, getattr(h, name).restype = _lib._SIGS[name]
    assert h.ssa_elem_type() == (0 if _F16 else 1)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)              # noqa: E731
    window = (7, 5, K.TILE_W + 5, K.TILE_H + 3)
    x0, y0, cw, ch = window
    src, lab = K.hostile_source(window, K.TILE_H + 3 + 11, K.TILE_W + 5 + 16)
    H, W = lab.shape
    n = 0
    for program in ([("Rotate", -17.0), ("Equalize", 0.0), ("Sharpness", 1.9), ("TranslateX", 3.3)],):
        pg = K.params(program, cw, ch).program()
        out, tmp = np.zeros((ch, cw, 3), np.uint8), np.zeros((ch, cw, 3), np.uint8)
        lout, ltmp = np.zeros((ch, cw), np.uint8), np.zeros((ch, cw), np.uint8)
        hist = np.zeros(768, np.uint32)
        assert h.ssa_randaug_u8(P(src), P(lab), H, W, x0, y0, cw, ch, 1, ctypes.byref(pg), 255, P(hist), P(out), P(tmp),
                                P(lout), P(ltmp), None) == 0
        wi, wl = R.augment(src, lab, program, window, True)
        assert np.array_equal(out, wi), K.first_difference(out, wi)
        assert np.array_equal(lout, wl), K.first_difference(lout, wl)
        assert int(hist.sum()) == 3 * cw * ch
        n += 1
    assert n == 1


# ------------------------------------------------------------------ argument validation (the real library, no device)
def test_entry_point_rejects_bad_arguments_without_gpu():
    from semseg_amd import _lib
    L = _lib.lib()
    P = ctypes.c_void_p
    buf = (ctypes.c_double * 1024)()                   # never read: every call below fails validation first
    ptr = P(ctypes.addressof(buf))

    def prog(ops, n_ops=None):
        pg = _lib.RandaugProgram()
        pg.n_ops = len(ops) if n_ops is None else n_ops
        for k, (op, v) in enumerate(ops[:8]):
            pg.op[k], pg.value[k] = op, v
            for j, c in enumerate((1.0, 0.1, 0.0, 0.0, 1.0, 0.0)):
                pg.matrix[k][j] = c
        return pg

    def call(img=ptr, lab=ptr, H=8, W=8, x0=0, y0=0, cw=8, ch=8, pg=None, ignore=255, hist=ptr, out=ptr, tmp=ptr,
             lout=ptr, ltmp=ptr):
        pgp = None if pg is None else ctypes.byref(pg)
        return L.ssa_randaug_u8(img, lab, H, W, x0, y0, cw, ch, 0, pgp, ignore, hist, out, tmp, lout, ltmp, None)

    ok = prog([(7, 0.0)])
    nan_matrix = prog([(1, 0.1)])
    nan_matrix.matrix[0][2] = float("nan")
    before = L.ssa_launch_count(0)
    bad = [dict(img=None, pg=ok), dict(out=None, pg=ok), dict(pg=None),                  # null image, output, program
           dict(lout=None, pg=ok),                                                      # labels and nowhere to put them
           dict(cw=0, pg=ok), dict(ch=0, pg=ok), dict(H=0, pg=ok),                      # empty window
           dict(x0=1, pg=ok), dict(y0=2, ch=7, pg=ok), dict(x0=-1, cw=4, pg=ok),        # window outside
           dict(pg=prog([(14, 0.0)])), dict(pg=prog([(-1, 0.0)])), dict(pg=prog([(7, 0.0), (99, 0.0)])),   # op index
           dict(pg=prog([(7, 0.0)] * 8, n_ops=9)), dict(pg=prog([], n_ops=-1)),         # more than the struct's slots
           dict(pg=prog([(10, 3.0)])), dict(pg=prog([(10, 9.0)])), dict(pg=prog([(10, 4.5)])),   # Posterize bits
           dict(pg=prog([(9, float("nan"))])), dict(pg=prog([(13, float("inf"))])), dict(pg=nan_matrix),
           dict(pg=prog([(6, 0.0)]), hist=None), dict(pg=prog([(8, 0.0)]), hist=P(ctypes.addressof(buf) + 2)),
           dict(pg=prog([(7, 0.0), (7, 0.0)]), tmp=None),                               # two launches, one buffer
           dict(pg=prog([(1, 0.1), (2, 0.1)]), ltmp=None),
           dict(pg=ok, ignore=256), dict(pg=ok, ignore=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert len(bad) == 27 and L.ssa_launch_count(0) == before


# ------------------------------------------------------------------ dry run of the host glue on CPU tensors
PARENT_LAUNCHING = ("ssa_image_u8_crop_flip_normalize", "ssa_label_u8_crop_flip", "ssa_jitter_luma_sum",
                    "ssa_jitter_apply_u8", "ssa_jitter_crop_flip_normalize", "ssa_gblur_u8",
                    "ssa_gblur_crop_flip_normalize")
LAUNCHING = PARENT_LAUNCHING + ("ssa_randaug_u8",)


class DryLib:
    """The real library with the launching entry points replaced by stand-ins that check every call against the ctypes
    signature declared in semseg_amd/_lib.py, record it and return 0 (the pattern of tests/test_gblur_cpu.py)."""

    def __init__(self, real):
        self._real = real
        self.order = []
        self.args = collections.defaultdict(list)

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in LAUNCHING:
            assert not name.startswith("ssa_") or name in ("ssa_launch_count",), "unexpected entry point %s" % name
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
            if name == "ssa_randaug_u8" and args[11] is not None:     # the buffer lives only as long as the call
                pg = args[9]._obj
                nh = sum(pg.op[k] in (6, 8) for k in range(pg.n_ops))
                self.hist_at_call = ctypes.string_at(_ptr(args[11]), nh * 768 * 4)
            return 0
        return launch


_OnDevice = K._OnDevice


def _waits(*a, **k):
    raise AssertionError("the host waited for the device")


@pytest.fixture()
def dry(monkeypatch):
    from semseg_amd import _lib, hip_backend as hb
    d = DryLib(_lib.lib())
    monkeypatch.setattr(_lib, "_LIB", d)
    monkeypatch.setattr(hb, "_s", lambda: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: collections.namedtuple("S", "cuda_stream")(0))
    for name in ("synchronize", "current_stream_synchronize"):
        monkeypatch.setattr(torch.cuda, name, _waits, raising=False)
    for name in ("item", "cpu", "tolist", "numpy", "__bool__", "__int__", "__float__", "nonzero"):
        monkeypatch.setattr(torch.Tensor, name, _waits)
    return d


def _ptr(v):
    return v.value if isinstance(v, ctypes.c_void_p) else v


def _pair():
    return (torch.zeros((20, 30, 3), dtype=torch.uint8).as_subclass(_OnDevice),
            torch.zeros((20, 30), dtype=torch.uint8).as_subclass(_OnDevice))


def test_dry_run_augment_none_launches_what_the_parent_launches(dry):
    """Entry point by entry point and argument by argument: the image half, the label half, for every combination of
    jitter and blur, exactly as without the keyword."""
    import gblur_cases as GK
    from semseg_amd.datasets import BlurParams, crop_flip_normalize
    img, lab = _pair()
    win = (3, 5, 17, 11)
    expected = {(False, False): ["ssa_image_u8_crop_flip_normalize", "ssa_label_u8_crop_flip"],
                (True, False): ["ssa_jitter_luma_sum", "ssa_jitter_crop_flip_normalize", "ssa_label_u8_crop_flip"],
                (False, True): ["ssa_gblur_crop_flip_normalize", "ssa_label_u8_crop_flip"],
                (True, True): ["ssa_jitter_luma_sum", "ssa_gblur_crop_flip_normalize", "ssa_label_u8_crop_flip"]}
    n = 0
    for (with_jitter, with_blur), order in expected.items():
        kw = {}
        if with_jitter:
            kw["jitter"] = GK.params(GK.JITTER_DRAWS)
        if with_blur:
            kw["blur"] = BlurParams(0.7)
        dry.order.clear()
        dry.args.clear()
        crop_flip_normalize(img, lab, win, True, **kw)
        plain_order, plain = list(dry.order), {k: list(v) for k, v in dry.args.items()}
        dry.order.clear()
        dry.args.clear()
        crop_flip_normalize(img, lab, win, True, augment=None, **kw)
        assert dry.order == plain_order == order
        for name in order:
            for a, b in zip(dry.args[name], plain[name]):
                assert a[1:7] == b[1:7] == (20, 30, 3, 5, 17, 11)
                assert name == "ssa_jitter_luma_sum" or a[7] == b[7] == 1
                assert _ptr(a[0]) == _ptr(b[0]) == (lab if name == "ssa_label_u8_crop_flip" else img).data_ptr()
        n += 1
    assert n == 4 and "ssa_randaug_u8" not in dry.args


def test_dry_run_chain_is_one_call_and_the_tail_reads_what_it_wrote(dry):
    import gblur_cases as GK
    from semseg_amd.datasets import BlurParams, crop_flip_normalize, rand_augment
    img, lab = _pair()
    win = (3, 5, 17, 11)
    p = K.params([("Rotate", -17.0), ("Equalize", 0.0), ("AutoContrast", 0.0), ("Sharpness", 1.9)], 17, 11)
    out, gts = crop_flip_normalize(img, lab, win, True, augment=p, jitter=GK.params(GK.JITTER_DRAWS), blur=BlurParams(0.7))
    assert dry.order == ["ssa_randaug_u8", "ssa_jitter_luma_sum", "ssa_gblur_crop_flip_normalize", "ssa_label_u8_crop_flip"]
    a = dry.args["ssa_randaug_u8"][0]
    assert (_ptr(a[0]), _ptr(a[1]), *a[2:9]) == (img.data_ptr(), lab.data_ptr(), 20, 30, 3, 5, 17, 11, 1) and a[10] == 255
    pg = a[9]._obj
    assert pg.n_ops == 4 and list(pg.op)[:4] == [5, 8, 6, 13] and pg.value[0] == -17.0 and pg.value[3] == 1.9
    assert list(pg.matrix[0]) == R.rotate_matrix(-17.0, 17, 11) and list(pg.matrix[1]) == [0.0] * 6
    assert _ptr(a[11]) % 4 == 0 and dry.hist_at_call == bytes(2 * 768 * 4)          # two histograms, zeroed
    ptrs = [_ptr(v) for v in a[12:16]]
    assert all(ptrs) and len(set(ptrs + [img.data_ptr(), lab.data_ptr()])) == 6     # four buffers of their own
    # the later steps read the chain's outputs, whole and not mirrored again; the luma sum is over the augmented window
    s, g, lb = dry.args["ssa_jitter_luma_sum"][0], dry.args["ssa_gblur_crop_flip_normalize"][0], dry.args["ssa_label_u8_crop_flip"][0]
    assert _ptr(s[0]) == _ptr(g[0]) == ptrs[0] and s[1:7] == g[1:7] == (11, 17, 0, 0, 17, 11) and g[7] == 0
    assert _ptr(lb[0]) == ptrs[2] and lb[1:8] == (11, 17, 0, 0, 17, 11, 0) and _ptr(lb[8]) == gts.data_ptr()
    assert tuple(out.shape) == (1, 11, 17, 16) and tuple(gts.shape) == (1, 11, 17)
    # without labels, without histograms: null pointers where nothing is needed
    dry.order.clear()
    gi, gl = rand_augment(img, None, K.params([("Invert", 0.0)], 30, 20))
    a = dry.args["ssa_randaug_u8"][-1]
    assert dry.order == ["ssa_randaug_u8"] and gl is None and a[1] is None and a[11] is None and a[14] is None and a[15] is None
    assert a[2:9] == (20, 30, 0, 0, 30, 20, 0) and _ptr(a[12]) == gi.data_ptr() and tuple(gi.shape) == (20, 30, 3)


def test_launch_budget_on_the_emulation(emu):
    """One launch per operation on the image, one per geometric operation on the labels, one histogram per AutoContrast /
    Equalize, at most one crop / flip copy -- counted by the library itself (ssa_launch_count) around each chain."""
    from semseg_amd import _lib
    window = (5, 3, 53, 37)
    src, lab = K.hostile_source(window, 46, 65)
    geo, hist = set(R.GEOMETRIC), {"AutoContrast", "Equalize"}
    n = 0
    for program in K.PROGRAMS:
        for labels in (lab, None):
            live = [(op, v) for op, v in program if not (op == "Identity" or (op == "Rotate" and v % 360 == 0))]
            on_labels = sum(op in geo for op, _ in live) if labels is not None else 0
            budget = len(live) + on_labels + sum(op in hist for op, _ in live)
            copy = int(not live or (labels is not None and not on_labels))
            before = _lib.lib().ssa_launch_count(0)
            K.run(emu, src, labels, program, window, True)
            assert _lib.lib().ssa_launch_count(0) - before == budget + copy, (program, labels is None)
            n += 1
    assert n == 18
