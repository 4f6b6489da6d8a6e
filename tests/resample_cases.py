"""The case tables of the exact / bounded resampling tests (tests/test_kernels_gpu.py test_exact_bilinear_* and
tests/test_resample_ref_cpu.py share them; a plain module).  Every shape is the smallest that reaches the branch named.

dtype flags: True = the 16-bit storage format, False = fp32.  `pads` = (source ld - C, destination ld - C)."""
import torch

from exact_util import ints
from resample_ref import grad_amp
from util import ACT_DTYPE

B = 2                               # every case: the image stride is in play
_F16 = ACT_DTYPE == torch.float16

# ---- 3a forward: (id, C, Hi, Wi, Ho, Wo, in16, out16, pads)
FWD_EXACT = []
for _n, _c, _hi, _wi, _ho, _wo in (("4x", 48, 5, 7, 20, 28), ("8x", 16, 3, 5, 24, 40), ("half", 48, 12, 20, 6, 10),
                                   ("copy", 48, 6, 10, 6, 10)):
    FWD_EXACT.append(("v8-%s" % _n, _c, _hi, _wi, _ho, _wo, True, True, (0, 0)))
    FWD_EXACT.append(("v8-%s-ld" % _n, _c, _hi, _wi, _ho, _wo, True, True, (8, 24)))
FWD_EXACT += [
    # one thread per pixel: <= 32 channels, fp32 out, dense out.  2 * 36 * 84 = 6048 pixels = 23.6 blocks of 256
    ("px-c19-4x", 19, 9, 21, 36, 84, False, False, (0, 0)),
    ("px-c19-4x-in16", 19, 9, 21, 36, 84, True, False, (0, 0)),
    ("px-c1-4x", 1, 9, 21, 36, 84, False, False, (0, 0)),
    ("px-c32-2x4", 32, 9, 37, 18, 148, False, False, (0, 0)),
    ("px-c32-2x4-in16", 32, 9, 37, 18, 148, True, False, (0, 0)),
    ("px-c19-ldx", 19, 9, 21, 36, 84, False, False, (5, 0)),
    ("px-c19-half", 19, 12, 20, 6, 10, False, False, (0, 0)),
    # one thread per element, the four dtype pairs
    ("el-c40-f32", 40, 9, 21, 18, 42, False, False, (0, 0)),                 # above the per-pixel limit
    ("el-c40-in16", 40, 9, 21, 18, 42, True, False, (0, 0)),
    ("el-c40-out16", 40, 9, 21, 18, 42, False, True, (5, 3)),
    ("el-c19-16", 19, 6, 10, 12, 20, True, True, (0, 0)),                    # C % 8 != 0 keeps it off the 8-channel kernel
    ("el-c19-16-ld", 19, 6, 10, 12, 20, True, True, (5, 3)),
    ("el-c19-out16", 19, 6, 10, 12, 20, False, True, (0, 0)),
    ("el-c19-f32-slice", 19, 6, 10, 12, 20, False, False, (0, 5)),           # ldy != C turns the per-pixel route off
    ("el-c19-in16-slice", 19, 6, 10, 12, 20, True, False, (3, 5)),
    ("el-c19-8x", 19, 3, 5, 24, 40, True, True, (0, 0)),
]

# ---- 3a backward through ssa_bilinear_bwd: (id, C, Hi, Wi, Ho, Wo, dy16, dx16, pads = (lddy - C, lddx - C))
BWD_EXACT = []
for _n, _c, _hi, _wi, _ho, _wo in (("2x", 48, 5, 7, 10, 14), ("4x", 48, 5, 7, 20, 28), ("8x", 16, 3, 5, 24, 40),
                                   ("half", 48, 12, 20, 6, 10), ("copy", 48, 6, 10, 6, 10), ("2x4", 48, 5, 7, 10, 28)):
    BWD_EXACT.append(("v8-%s" % _n, _c, _hi, _wi, _ho, _wo, True, True, (0, 0)))      # 2x, 4x: hoisted weights; 8x: recompute
    BWD_EXACT.append(("v8-%s-ld" % _n, _c, _hi, _wi, _ho, _wo, True, True, (16, 8)))
BWD_EXACT += [
    # the per-element gather
    ("el-c1-4x", 1, 9, 21, 36, 84, False, False, (0, 0)),                    # one channel: below the tiled route
    ("el-c40-2x", 40, 9, 21, 18, 42, False, False, (0, 0)),                  # above it
    ("el-c40-2x-ld", 40, 9, 21, 18, 42, False, False, (5, 3)),
    ("el-c40-out16", 40, 9, 21, 18, 42, False, True, (5, 3)),
    ("el-c40-8x", 40, 3, 5, 24, 40, False, False, (0, 0)),                   # recompute branch
    ("el-c19-16", 19, 6, 10, 12, 20, True, True, (0, 0)),
    ("el-c19-16-ld", 19, 6, 10, 12, 20, True, True, (5, 3)),
    ("el-c19-16-4x", 19, 5, 7, 20, 28, True, True, (0, 0)),
    ("el-c19-8x", 19, 3, 5, 24, 40, False, False, (5, 3)),                   # 16 taps > 12: refused by the tiled route
    ("el-c19-8x-out16", 19, 3, 5, 24, 40, False, True, (0, 0)),
    ("el-c19-half", 19, 12, 20, 6, 10, False, False, (5, 3)),                # downsampling: refused by the tiled route
    # the LDS-tiled kernel: fp32 dy, 8 <= C <= 32, upsampling, at most 12 taps
    ("tile-t4", 19, 9, 21, 18, 42, False, False, (0, 0)),
    ("tile-t4-ld", 19, 9, 21, 18, 42, False, False, (5, 3)),
    ("tile-t4-out16", 19, 9, 21, 18, 42, False, True, (5, 3)),
    ("tile-t8", 19, 9, 21, 36, 84, False, False, (0, 0)),
    ("tile-t8-ld-out16", 19, 9, 21, 36, 84, False, True, (5, 3)),
    ("tile-t8-c8-4x2", 8, 9, 37, 36, 74, False, False, (5, 3)),
    ("tile-t8-2x4", 19, 9, 21, 18, 84, False, False, (5, 3)),
    ("tile-c8-2x", 8, 9, 21, 18, 42, False, False, (0, 0)),
    ("tile-c32-2x", 32, 9, 21, 18, 42, False, False, (5, 3)),
    ("tile-c32-4x-out16", 32, 9, 21, 36, 84, False, True, (0, 0)),
    ("tile-full-tile", 19, 4, 16, 8, 32, False, False, (5, 3)),              # exactly one 4 x 16 tile per image
    ("tile-two-tiles", 19, 8, 32, 32, 128, False, False, (0, 0)),            # full tiles only, 4x
    ("tile-copy", 19, 6, 10, 6, 10, False, False, (0, 0)),                   # 1x counts as upsampling: TAPS 4, two taps used
    ("el-c40-copy", 40, 6, 10, 6, 10, False, False, (0, 0)),
    ("tile-1x1", 19, 1, 1, 2, 2, False, False, (5, 3)),
    ("tile-1x1-4x", 19, 1, 1, 4, 4, False, False, (0, 0)),
]

# ---- 3a backward through the separable pair ssa_bilinear_bwd_x / _y: same columns
SEP_EXACT = [
    ("v8-2x", 48, 5, 7, 10, 14, True, True, (0, 0)),                         # 4-tap batch
    ("v8-2x-ld", 48, 5, 7, 10, 14, True, True, (16, 8)),
    ("v8-4x", 48, 5, 7, 20, 28, True, True, (0, 0)),                         # 8-tap batch
    ("v8-4x-ld", 48, 5, 7, 20, 28, True, True, (16, 8)),
    ("v8-8x", 16, 3, 5, 24, 40, True, True, (0, 0)),                         # generic loop
    ("v8-8x-ld", 16, 3, 5, 24, 40, True, True, (16, 8)),
    ("v8-2x4-ld", 48, 5, 7, 10, 28, True, True, (16, 8)),
    ("v1-16-2x", 19, 5, 7, 10, 14, True, True, (5, 3)),
    ("v1-16-4x", 19, 5, 7, 20, 28, True, True, (0, 0)),
    ("v1-16-8x", 19, 3, 5, 24, 40, True, True, (5, 3)),
    ("v1-f32-2x", 19, 5, 7, 10, 14, False, False, (0, 0)),
    ("v1-f32-4x", 19, 5, 7, 20, 28, False, False, (5, 3)),
    ("v1-f32-8x", 19, 3, 5, 24, 40, False, False, (0, 0)),
    ("v1-f32-2x4-out16", 19, 5, 7, 10, 28, False, True, (5, 3)),
]

# ---- 3b: ratios that are not dyadic, within resize_bound: (id, C, Hi, Wi, Ho, Wo, is16)
BOUNDED = [
    ("c19-33x45", 19, 33, 45, 67, 91, False),
    ("c19-8x12", 19, 8, 12, 21, 31, False),               # tiled, TAPS 8, the window from bwd_window
    ("c32-10x3", 32, 10, 3, 27, 35, False),
    ("c8-4x9", 8, 4, 9, 43, 20, False),                   # one axis above 12 taps: falls back to the gather
    ("c8-x5", 8, 4, 6, 20, 30, False),                    # integer factors 5 and 6: the TAPS = 12 instantiations
    ("c8-x6", 8, 3, 4, 18, 24, False),
    ("c19-down", 19, 67, 91, 33, 45, False),
    ("c8-down", 8, 100, 3, 37, 1, False),
    ("c8-wide-up", 8, 7, 1100, 9, 2199, False),           # index magnitudes where the fp32 candidate range is coarsest
    ("c8-wide-down", 8, 3, 4093, 3, 1500, False),
    ("c19-from1", 19, 1, 1, 5, 7, False),
    ("c19-from2", 19, 2, 2, 7, 9, False),
    ("c19-to1", 19, 5, 7, 1, 1, False),
    ("c48-16-up", 48, 13, 17, 40, 60, True),
    ("c48-16-down", 48, 40, 60, 13, 17, True),
    ("c16-16-wide", 16, 3, 700, 7, 2099, True),
]

# the dyadic family the exact cases draw their ratios from, (n_out, n_in) per axis, and the sizes of the grid-stride cases
DYADIC = sorted({(c[4], c[2]) for c in FWD_EXACT + BWD_EXACT + SEP_EXACT} | {(c[5], c[3]) for c in FWD_EXACT + BWD_EXACT + SEP_EXACT}
                | {(1030, 515), (2060, 1030), (515, 1030), (1460, 730)})

_FWD_AMP = 200        # |x| <= 200 < 2^8: the magnitude product of a forward is at most max |x| (rows of weights sum to 1)
_FWD_AMP_HALF_F16 = 2000      # the fp16 build at 0.5x: quarters of 11-bit integers (exact in fp16) need 13 bits, the format has
                              # 11; one fraction bit per axis keeps the premise, 2000 * 2^2 < 2^24


def fwd_operand(case, seed=401):
    _, C, Hi, Wi, Ho, Wo = case[:6]
    half = _F16 and (Ho, Wo) != (Hi, Wi) and Ho <= Hi and Wo <= Wi
    amp = _FWD_AMP_HALF_F16 if half else _FWD_AMP
    return ints((B, Hi, Wi, C), -amp, amp, seed)


def bwd_operand(case, seed=402):
    _, C, Hi, Wi, Ho, Wo = case[:6]
    a = grad_amp(Ho, Hi, Wo, Wi, 200)
    return ints((B, Ho, Wo, C), -a, a, seed)


def bounded_operands(case):
    _, C, Hi, Wi, Ho, Wo = case[:6]
    return ints((B, Hi, Wi, C), -64, 64, 403), ints((B, Ho, Wo, C), -64, 64, 404)


def fwd_rounds(case):
    """Can a forward output of this case need rounding to the storage format at all?  Not the identity resize: its outputs
    are its inputs."""
    _, C, Hi, Wi, Ho, Wo, in16, out16 = case[:8]
    return out16 and (Hi, Wi) != (Ho, Wo)


def bwd_rounds(case):
    """Likewise for the backward: at 1x and 0.5x every input pixel receives ONE gradient value times a power of two."""
    _, C, Hi, Wi, Ho, Wo, dy16, dx16 = case[:8]
    return dx16 and (Ho > Hi or Wo > Wi)
