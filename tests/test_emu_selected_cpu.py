"""A fast selection of the GPU-marked kernel tests, run on the CPU EMULATION of the kernels.

`tools/emu` compiles the unchanged kernel sources for the host (workgroups as cooperative fibers; MFMA, the transposing
LDS read and the LDS DMA emulated with the lane maps the probe tests pin on the device), and `SSA_EMU=1` makes the
`-m gpu` kernel tests run against that library with CPU tensors as device memory (tests/conftest.py, tests/emu_util.py).
The whole emulated suite takes hours (a 130x131x192->200 conv is four minutes); this module runs, in a subprocess, the
tests that take seconds and cover the element-wise / loss / resampling kernels and the small conv dispatch classes --
so that index arithmetic, LDS layouts and barrier structure of those kernels are checked by the default CPU suite, not
only on the GPU box.  Test infrastructure: the product never loads the emulation library."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the emulated share of the exact tests: every strip regime once (ragged, image crossing, tiles_x == 1, interior + border,
# one strip over the whole problem, the units < nchunk clamp), every epilogue mode, both filter packings; of the head
# kernels the small wide-GEMM cases and the one 256 x 128 halo-GEMM case that runs in seconds
_EXACT = ("exact_strip and (need_rounding or sliced or grouped or mode0[c48u4-fwd or mode0[c48u64-dgrad or mode0[c48w20-fwd "
          "or mode0[c96u5-fwd or mode0[c192u16-dgrad or mode0[c384u4-fwd or no_stats[c48w16 or mode1[c48u5-dgrad "
          "or mode2[c48u4 or mode2[c192u12 or affine[c48u3-res-mode4relu "
          "or affine[c48w16-res-mode3 or affine[c48u5-nores-mode4relu) or exact_tile_and_tile_aux or exact_wgrad_splitk "
          "or exact_gemm_wide or exact_halo_gemm_1x1[A or exact_dgrad_s2 and (case2 or case4 or case5) "
          "or exact_igemm and 3-out16 or exact_wgrad_tile and 48-1-37-45-strip2")

_EXACT_F16 = ("exact_strip and (need_rounding or mode0[c48u4-fwd or mode1[c48u5-dgrad or mode2[c48u4 "
              "or affine[c48u3-res-mode4relu or no_stats[c48w16) or exact_tile_and_tile_aux and case3 or exact_igemm and 3-out16")

# the exact BatchNorm tests (csrc/bn.hip through the C ABI): the cases of one chunk per workgroup -- VC = 1 with P < RP, the
# ragged last range at 252 of 256 active threads, VC = 31 with a last range of one pixel -- in their full configuration
# matrices, the parameter-gradient casts, the grid mirror, and the evaluation-mode backward (the GPU runs the multi-chunk
# cases of 6 to 26 M elements)
_EXACT_BN = "exact_bn and (c8 or c48 or c248 or param_grads or plan_mirror) or bn_eval_backward"
_EXACT_BN_F16 = "exact_bn and (c48 or param_grads)"

# the exact resampling and pooling tests (csrc/resample.hip, csrc/pool.hip through the C ABI): every case of every route
# table, the bounded cases, the Python dispatch passes, image resize and both pools -- seconds under emulation (the GPU
# adds the grid-stride cases of 2 M threads and more, which skip here).  The fp16-storage build runs one case per 16-bit
# route.
_EXACT_RESAMPLE = "exact_bilinear or exact_image_resize or exact_pool"
_EXACT_RESAMPLE_F16 = ("exact_bilinear_fwd and (v8-4x-ld or px-c19-4x-in16 or el-c40-in16 or el-c40-out16 or el-c19-16-ld) "
                       "or exact_bilinear_bwd[ and (v8-4x-ld or v8-8x-ld or el-c19-16-ld or el-c40-out16 or tile-t8-ld-out16) "
                       "or exact_bilinear_bwd_separable and (v8-4x-ld or v1-16-8x or v1-f32-2x4-out16) "
                       "or exact_bilinear_autograd and (v8-slices or px16-tile16) or exact_bilinear_upsample_cat "
                       "or exact_bilinear_bounded and c48-16-up or exact_image_resize or exact_pool")

# the exact OCR head tests (csrc/ocr_attn.hip, csrc/ocr.hip through the C ABI and through OcrAttnFn / OcrGatherFn): every
# case but the two large ones (131,205 pixels of attention, the re-balanced HW softmax over 16,515 pixels x 256 classes),
# which skip here.  The fp16-storage build runs a tie case per region-block count and two gather cases.
_EXACT_OCR = "exact_ocr"
_EXACT_OCR_F16 = ("exact_ocr_attn_tie and (k19-p300 or k65-p300 or k96-p300) or exact_ocr_hw_softmax[k19-13x21 "
                  "or exact_ocr_gather_autograd[k65")

# (file, -k expression): each entry a few seconds under emulation
SELECTION = [
    ("tests/test_kernels_gpu.py", "bce_rmi or scale_fusion or cross_entropy or sigmoid or softmax"),
    ("tests/test_kernels_gpu.py", "probe or bn_train or bn_eval or bn_deferred or (bilinear and not exact_bilinear) or maxpool or conv_channel_slice"),
    ("tests/test_kernels_gpu.py", "test_conv_fwd_bwd and (case1] or case10] or case19] or case32] or case33])"),
    ("tests/test_group_gpu.py", "upsample_cat or cat_slots"),
    # round 5: the fused object attention (19 / 65 / 96 regions, ragged pixel counts, the three-launch form), a grouped
    # weight-gradient launch of more than 16 layers
    ("tests/test_kernels_gpu.py", "ocr_attention or twenty"),
    # the exact (integer-operand, bit-for-bit) conv tests: the persistent trunk kernel over multi-tile strips in every
    # epilogue mode, and the small cases of the other conv entry points (the GPU runs the full lists)
    ("tests/test_kernels_gpu.py", _EXACT),
    ("tests/test_kernels_gpu.py", _EXACT_BN),
    ("tests/test_kernels_gpu.py", _EXACT_RESAMPLE),
    ("tests/test_exact_ocr_gpu.py", _EXACT_OCR),
]
# how many tests an expression must run: a renamed case id would otherwise silently select fewer
MIN_PASSED = {_EXACT: 47, _EXACT_F16: 10, _EXACT_BN: 27, _EXACT_BN_F16: 8, _EXACT_RESAMPLE: 115, _EXACT_RESAMPLE_F16: 28,
              _EXACT_OCR: 44, _EXACT_OCR_F16: 5}


# (file, -k expression, extra environment): the fp16-storage build of the same kernels (its own rounding helpers)
SELECTION_ENV = [("tests/test_kernels_gpu.py", _EXACT_F16, {"SSA_ACT_DTYPE": "fp16"}),
                 ("tests/test_kernels_gpu.py", _EXACT_BN_F16, {"SSA_ACT_DTYPE": "fp16"}),
                 ("tests/test_kernels_gpu.py", _EXACT_RESAMPLE_F16, {"SSA_ACT_DTYPE": "fp16"}),
                 ("tests/test_exact_ocr_gpu.py", _EXACT_OCR_F16, {"SSA_ACT_DTYPE": "fp16"})]


def _passed_enough(expr, tail):
    import re
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) >= MIN_PASSED.get(expr, 1), "%r ran %s tests, expected >= %d:\n%s" % (
        expr, m.group(1) if m else "no", MIN_PASSED.get(expr, 1), tail)


def test_selected_kernel_tests_pass_on_the_emulated_kernels():
    env = dict(os.environ, SSA_EMU="1")
    env.pop("PYTEST_CURRENT_TEST", None)
    for path, expr, extra in SELECTION_ENV:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, path), "-q", "-x", "-m", "gpu", "-k", expr,
                            "-p", "no:cacheprovider"], cwd=ROOT, env=dict(env, **extra), capture_output=True, text=True, timeout=900)
        tail = "\n".join(r.stdout.splitlines()[-15:])
        assert r.returncode == 0, "%s -k %r under SSA_EMU=1 %r:\n%s\n%s" % (path, expr, extra, tail, r.stderr[-2000:])
        assert " passed" in tail and "failed" not in tail, tail
        _passed_enough(expr, tail)
    for path, expr in SELECTION:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, path), "-q", "-x", "-m", "gpu", "-k", expr,
                            "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        tail = "\n".join(r.stdout.splitlines()[-15:])
        assert r.returncode == 0, "%s -k %r under SSA_EMU=1:\n%s\n%s" % (path, expr, tail, r.stderr[-2000:])
        assert " passed" in tail and "failed" not in tail, tail
        _passed_enough(expr, tail)
