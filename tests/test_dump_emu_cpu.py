"""The dump-tail kernels (csrc/dump_tail.hip: ssa_dump_tail, ssa_mask_u8) compiled for the host (tools/emu), on both
storage builds, against tests/dump_ref.py byte for byte: the cases of tests/dump_cases.py that tests/test_dump_gpu.py runs
on the device (without the 1024 x 2048 one: a workgroup is 256 fibers here).  Then the argument rejections, on the real
library: they come back before the device is touched."""
import ctypes
import os
import subprocess

import pytest

import dump_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bind(h):
    from semseg_amd import _lib
    for name in ("ssa_elem_type", "ssa_dump_tail", "ssa_mask_u8"):
        getattr(h, name).argtypes, getattr(h, name).restype = _lib._SIGS[name]
    return h


@pytest.fixture(scope="module")
def this_build():
    from emu_util import emu_lib
    return emu_lib()


@pytest.fixture(scope="module")
def other_build():
    """The emulation library of the OTHER element type (fp16 storage when this process runs bf16)."""
    from emu_util import _F16
    subprocess.check_call(["sh", os.path.join(ROOT, "tools", "emu", "build.sh")] + ([] if _F16 else ["f16"]),
                          stdout=subprocess.DEVNULL)
    h = _bind(ctypes.CDLL(os.path.join(ROOT, "tools", "emu", "build" if _F16 else "build_f16", "libsemseg_emu.so")))
    assert h.ssa_elem_type() == (0 if _F16 else 1)
    return h


@pytest.fixture(params=["this", "other"])
def L(request, this_build, other_build):
    return this_build if request.param == "this" else other_build


def test_emulated_all_outputs_at_every_shape(L):
    assert K.check_shapes_all_outputs(L, "cpu") == 21


def test_emulated_subsets_of_outputs(L):
    assert K.check_subsets_of_outputs(L, "cpu") == 10


def test_emulated_unaligned_pointers_take_the_pixel_path(L):
    assert K.check_unaligned_pointers(L, "cpu") == 14


def test_emulated_all_pairs_blend_equals_live_pillow(L):
    assert K.check_all_pairs_blend(L, "cpu") == 3


def test_emulated_all_bytes_denormalise_equals_torch(L):
    assert K.check_all_bytes_denormalise(L, "cpu") == 1


def test_emulated_mask_u8(L):
    assert K.check_mask_u8(L, "cpu") == 10


def test_entry_points_reject_bad_arguments_without_gpu():
    from semseg_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()                      # never read: every call below fails validation first
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    f3 = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    names = ("image", "plane", "inv_mean", "inv_std", "gts", "pred", "pal", "ids", "prob", "err", "alpha", "H", "W",
             "input_rgb", "gt_rgb", "pred_rgb", "comp_rgb", "label_ids", "prob_u8", "err_u8")
    ok = dict(image=ptr, plane=64, inv_mean=f3, inv_std=f3, gts=ptr, pred=ptr, pal=ptr, ids=ptr, prob=ptr, err=ptr,
              alpha=0.4, H=4, W=4, input_rgb=ptr, gt_rgb=ptr, pred_rgb=ptr, comp_rgb=ptr, label_ids=ptr, prob_u8=ptr,
              err_u8=ptr)
    no_out = dict(input_rgb=None, gt_rgb=None, pred_rgb=None, comp_rgb=None, label_ids=None, prob_u8=None, err_u8=None)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.ssa_dump_tail(*[a[n] for n in names], None)

    def only(out, **kw):
        a = dict(no_out)
        a[out] = ptr
        a.update(kw)
        return call(**a)

    before = lib.ssa_launch_count(0)
    bad = [call(**no_out),                                                       # a null set of outputs
           call(H=0), call(W=0), call(H=-3),                                     # no pixels
           only("input_rgb", image=None), only("input_rgb", inv_mean=None), only("input_rgb", inv_std=None),
           only("input_rgb", plane=15),                                          # planes that overlap
           only("gt_rgb", gts=None), only("gt_rgb", pal=None),
           only("pred_rgb", pred=None), only("pred_rgb", pal=None),
           only("comp_rgb", image=None), only("comp_rgb", pred=None), only("comp_rgb", pal=None),
           only("comp_rgb", alpha=1.5), only("comp_rgb", alpha=-0.1), only("comp_rgb", alpha=float("nan")),
           only("label_ids", pred=None), only("label_ids", ids=None),
           only("prob_u8", prob=None), only("err_u8", err=None),
           lib.ssa_mask_u8(None, 4, ptr, None), lib.ssa_mask_u8(ptr, 4, None, None), lib.ssa_mask_u8(ptr, 0, ptr, None)]
    assert bad == [-1] * len(bad), bad
    assert lib.ssa_launch_count(0) == before
