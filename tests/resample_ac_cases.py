"""The case tables of the exact / bounded resampling tests under align_corners=True (tests/test_exact_resample_ac_gpu.py and
tests/test_resample_ac_ref_cpu.py share them; a plain module).  The format and the routes are those of
tests/resample_cases.py, route for route; every shape is the smallest that reaches the branch named.

Exact family: (n_in - 1) / (n_out - 1) a power of two, i.e. sizes k 2^m + 1 -- 5 -> 9 -> 17 -> 33, 7 -> 13 -> 25, 21 -> 41 -> 81.
Taps per input pixel at those ratios (resample_ac_ref.window_ac): 1 at 1x and 0.5x, 3 at 2x, 7 at 4x, 15 at 8x; the host
sizes its windows with ceil(2 / scale) + 1 = 3 / 5 / 9 / 17, which selects the TAPS = 4 / 8 / 12 instantiations of the
tiled backward and refuses 8x.  scale == 0 (one output or one input pixel on an axis): input 0 receives the whole axis.

dtype flags: True = the 16-bit storage format, False = fp32.  `pads` = (source ld - C, destination ld - C)."""
from exact_util import ints
from resample_ac_ref import grad_amp_ac
import resample_cases as RC

B = 2                               # every case: the image stride is in play

# the scale == 0 regime: both axes from one pixel, both axes to one pixel, one axis only (x at 2x)
_ZERO = (("from1", 1, 1, 4, 6), ("to1", 5, 7, 1, 1), ("from1-y", 1, 7, 4, 13))

# ---- forward: (id, C, Hi, Wi, Ho, Wo, in16, out16, pads)
FWD_EXACT = []
for _n, _c, _hi, _wi, _ho, _wo in (("2x", 48, 5, 7, 9, 13), ("4x", 48, 5, 7, 17, 25), ("8x", 16, 3, 5, 17, 33),
                                   ("half", 48, 9, 13, 5, 7), ("copy", 48, 6, 10, 6, 10)):
    FWD_EXACT.append(("v8-%s" % _n, _c, _hi, _wi, _ho, _wo, True, True, (0, 0)))
    FWD_EXACT.append(("v8-%s-ld" % _n, _c, _hi, _wi, _ho, _wo, True, True, (8, 24)))
FWD_EXACT += [
    # one thread per pixel: <= 32 channels, fp32 out, dense out.  2 * 33 * 81 = 5346 pixels = 20.9 blocks of 256
    ("px-c19-4x", 19, 9, 21, 33, 81, False, False, (0, 0)),
    ("px-c19-4x-in16", 19, 9, 21, 33, 81, True, False, (0, 0)),
    ("px-c1-4x", 1, 9, 21, 33, 81, False, False, (0, 0)),
    ("px-c32-2x4", 32, 9, 37, 17, 145, False, False, (0, 0)),
    ("px-c32-2x4-in16", 32, 9, 37, 17, 145, True, False, (0, 0)),
    ("px-c19-ldx", 19, 9, 21, 33, 81, False, False, (5, 0)),
    ("px-c19-half", 19, 9, 13, 5, 7, False, False, (0, 0)),
    # one thread per element, the four dtype pairs
    ("el-c40-f32", 40, 9, 21, 17, 41, False, False, (0, 0)),                 # above the per-pixel limit
    ("el-c40-in16", 40, 9, 21, 17, 41, True, False, (0, 0)),
    ("el-c40-out16", 40, 9, 21, 17, 41, False, True, (5, 3)),
    ("el-c19-16", 19, 5, 9, 9, 17, True, True, (0, 0)),                      # C % 8 != 0 keeps it off the 8-channel kernel
    ("el-c19-16-ld", 19, 5, 9, 9, 17, True, True, (5, 3)),
    ("el-c19-out16", 19, 5, 9, 9, 17, False, True, (0, 0)),
    ("el-c19-f32-slice", 19, 5, 9, 9, 17, False, False, (0, 5)),             # ldy != C turns the per-pixel route off
    ("el-c19-in16-slice", 19, 5, 9, 9, 17, True, False, (3, 5)),
    ("el-c19-8x", 19, 3, 5, 17, 33, True, True, (0, 0)),
]
for _n, _hi, _wi, _ho, _wo in _ZERO:
    FWD_EXACT += [("v8-%s" % _n, 48, _hi, _wi, _ho, _wo, True, True, (8, 24)),
                  ("px-c19-%s" % _n, 19, _hi, _wi, _ho, _wo, False, False, (5, 0)),
                  ("el-c40-%s" % _n, 40, _hi, _wi, _ho, _wo, False, True, (5, 3)),
                  ("el-c19-16-%s" % _n, 19, _hi, _wi, _ho, _wo, True, True, (5, 3))]

# ---- backward through ssa_resize_bilinear_bwd: (id, C, Hi, Wi, Ho, Wo, dy16, dx16, pads = (lddy - C, lddx - C))
BWD_EXACT = []
for _n, _c, _hi, _wi, _ho, _wo in (("2x", 48, 5, 7, 9, 13), ("4x", 48, 5, 7, 17, 25), ("8x", 16, 3, 5, 17, 33),
                                   ("half", 48, 9, 13, 5, 7), ("copy", 48, 6, 10, 6, 10), ("2x4", 48, 5, 7, 9, 25)):
    # 2x, 4x: 5 and 9 candidate columns, hoisted weights; 8x: 17 candidates (15 taps) > kMaxCand = 12, the recompute branch
    BWD_EXACT.append(("v8-%s" % _n, _c, _hi, _wi, _ho, _wo, True, True, (0, 0)))
    BWD_EXACT.append(("v8-%s-ld" % _n, _c, _hi, _wi, _ho, _wo, True, True, (16, 8)))
BWD_EXACT += [
    # the per-element gather
    ("el-c1-4x", 1, 9, 21, 33, 81, False, False, (0, 0)),                    # one channel: refused by the tiled route
    ("el-c40-2x", 40, 9, 21, 17, 41, False, False, (0, 0)),                  # C > 32: refused by it
    ("el-c40-2x-ld", 40, 9, 21, 17, 41, False, False, (5, 3)),
    ("el-c40-out16", 40, 9, 21, 17, 41, False, True, (5, 3)),
    ("el-c40-8x", 40, 3, 5, 17, 33, False, False, (0, 0)),                   # recompute branch
    ("el-c19-16", 19, 5, 9, 9, 17, True, True, (0, 0)),
    ("el-c19-16-ld", 19, 5, 9, 9, 17, True, True, (5, 3)),
    ("el-c19-16-4x", 19, 5, 7, 17, 25, True, True, (0, 0)),
    ("el-c19-8x", 19, 3, 5, 17, 33, False, False, (5, 3)),                   # 17 taps > 12: refused by the tiled route
    ("el-c19-8x-out16", 19, 3, 5, 17, 33, False, True, (0, 0)),
    ("el-c19-half", 19, 9, 13, 5, 7, False, False, (5, 3)),                  # downsampling: refused by the tiled route
    # the LDS-tiled kernel: fp32 dy, 8 <= C <= 32, upsampling, at most 12 taps
    ("tile-t8", 19, 9, 21, 17, 41, False, False, (0, 0)),                    # 2x: 5 taps, TAPS 8
    ("tile-t8-ld", 19, 9, 21, 17, 41, False, False, (5, 3)),
    ("tile-t8-out16", 19, 9, 21, 17, 41, False, True, (5, 3)),
    ("tile-t12", 19, 9, 21, 33, 81, False, False, (0, 0)),                   # 4x: 9 taps, TAPS 12
    ("tile-t12-ld-out16", 19, 9, 21, 33, 81, False, True, (5, 3)),
    ("tile-t12-c8-4x2", 8, 9, 37, 33, 73, False, False, (5, 3)),
    ("tile-t12-2x4", 19, 9, 21, 17, 81, False, False, (5, 3)),
    ("tile-c8-2x", 8, 9, 21, 17, 41, False, False, (0, 0)),
    ("tile-c32-2x", 32, 9, 21, 17, 41, False, False, (5, 3)),
    ("tile-c32-4x-out16", 32, 9, 21, 33, 81, False, True, (0, 0)),
    ("tile-full-tile", 19, 4, 16, 7, 31, False, False, (5, 3)),              # exactly one 4 x 16 tile per image
    ("tile-two-tiles", 19, 8, 32, 29, 125, False, False, (0, 0)),            # full tiles only, 4x
    ("tile-copy", 19, 6, 10, 6, 10, False, False, (0, 0)),                   # 1x: 3 taps allowed for, TAPS 4, one used
    ("el-c40-copy", 40, 6, 10, 6, 10, False, False, (0, 0)),
    ("tile-1x1", 19, 1, 1, 2, 2, False, False, (5, 3)),                      # scale 0: the window is the axis, TAPS 4
    ("tile-1x1-4x", 19, 1, 1, 4, 4, False, False, (0, 0)),
]
for _n, _hi, _wi, _ho, _wo in _ZERO:
    # from1: tiled (windows 4 and 6: TAPS 8); from1-y: tiled (4 rows, 5 columns); to1: downsampling, the gather
    BWD_EXACT += [("v8-%s" % _n, 48, _hi, _wi, _ho, _wo, True, True, (16, 8)),
                  ("c19-%s" % _n, 19, _hi, _wi, _ho, _wo, False, False, (5, 3)),
                  ("el-c40-%s" % _n, 40, _hi, _wi, _ho, _wo, False, True, (5, 3)),
                  ("el-c19-16-%s" % _n, 19, _hi, _wi, _ho, _wo, True, True, (5, 3))]

# ---- backward through the separable pair ssa_resize_bilinear_bwd_x / _y: same columns
SEP_EXACT = [
    ("v8-2x", 48, 5, 7, 9, 13, True, True, (0, 0)),                          # 3 taps: the 4-tap batch
    ("v8-2x-ld", 48, 5, 7, 9, 13, True, True, (16, 8)),
    ("v8-4x", 48, 5, 7, 17, 25, True, True, (0, 0)),                         # 7 taps: the 8-tap batch
    ("v8-4x-ld", 48, 5, 7, 17, 25, True, True, (16, 8)),
    ("v8-8x", 16, 3, 5, 17, 33, True, True, (0, 0)),                         # 15 taps: the generic loop
    ("v8-8x-ld", 16, 3, 5, 17, 33, True, True, (16, 8)),
    ("v8-2x4-ld", 48, 5, 7, 9, 25, True, True, (16, 8)),
    ("v1-16-2x", 19, 5, 7, 9, 13, True, True, (5, 3)),
    ("v1-16-4x", 19, 5, 7, 17, 25, True, True, (0, 0)),
    ("v1-16-8x", 19, 3, 5, 17, 33, True, True, (5, 3)),
    ("v1-f32-2x", 19, 5, 7, 9, 13, False, False, (0, 0)),
    ("v1-f32-4x", 19, 5, 7, 17, 25, False, False, (5, 3)),
    ("v1-f32-8x", 19, 3, 5, 17, 33, False, False, (0, 0)),
    ("v1-f32-2x4-out16", 19, 5, 7, 9, 25, False, True, (5, 3)),
    ("v8-from1", 48, 1, 1, 4, 6, True, True, (16, 8)),                       # scale 0 on both passes
    ("v1-f32-from1", 19, 1, 1, 4, 6, False, False, (5, 3)),
    ("v8-from1-y", 48, 1, 7, 4, 13, True, True, (0, 0)),                     # scale 0 in pass Y only
    ("v1-16-from1-y", 19, 1, 7, 4, 13, True, True, (5, 3)),
    ("v1-f32-to1", 19, 5, 7, 1, 1, False, False, (0, 0)),                    # (the pair itself takes any ratio)
]

# ---- ratios that are not dyadic, within resample_ac_ref.resize_bound_ac: (id, C, Hi, Wi, Ho, Wo, is16).  The non-dyadic
# shapes of resample_cases.BOUNDED, and the network's own ratios in small: 4x, 8x and 0.5x of even sizes
BOUNDED = list(RC.BOUNDED) + [
    ("net-c19-4x", 19, 8, 8, 32, 32, False),              # scale 7/31: 9 taps, tiled with TAPS 12
    ("net-c48-16-4x", 48, 8, 8, 32, 32, True),
    ("net-c19-8x", 19, 4, 4, 32, 32, False),              # scale 3/31: 21 taps, the gather's recompute branch
    ("net-c48-16-8x", 48, 4, 4, 32, 32, True),
    ("net-c19-half", 19, 16, 16, 8, 8, False),
    ("net-c48-16-half", 48, 16, 16, 8, 8, True),
]

_ALL_EXACT = FWD_EXACT + BWD_EXACT + SEP_EXACT
# the dyadic family the exact cases draw their sizes from, (n_out, n_in) per axis, and the sizes of the grid-stride cases
DYADIC = sorted({(c[4], c[2]) for c in _ALL_EXACT} | {(c[5], c[3]) for c in _ALL_EXACT}
                | {(1029, 515), (2059, 1030), (515, 1029), (1459, 730)})

_FWD_AMP = 200        # |x| <= 200 < 2^8: the magnitude product of a forward is at most max |x| (rows of weights sum to 1)


def fwd_operand(case, seed=401):
    _, C, Hi, Wi, Ho, Wo = case[:6]
    return ints((B, Hi, Wi, C), -_FWD_AMP, _FWD_AMP, seed)


def bwd_operand(case, seed=402):
    _, C, Hi, Wi, Ho, Wo = case[:6]
    a = grad_amp_ac(Ho, Hi, Wo, Wi, 200)
    return ints((B, Ho, Wo, C), -a, a, seed)


def bounded_operands(case):
    _, C, Hi, Wi, Ho, Wo = case[:6]
    return ints((B, Hi, Wi, C), -64, 64, 403), ints((B, Ho, Wo, C), -64, 64, 404)
