"""Cases, operands and float64 references of the exact tests of the 5x5 conv kernel (csrc/conv_halo5.hip), shared by
tests/test_exact_conv5x5_gpu.py (the device) and tests/test_conv5x5_emu_cpu.py (the CPU emulation of both storage
builds).  A plain module, not a conftest.

Each case is the smallest at which one mechanism of the kernel can go wrong (tile 4 rows x 32 pixels x 256 channels,
halo 8 x 36 pixels, K chunks of 64 or 48 channels in two LDS buffers, 8 n-blocks of 32 channels per workgroup):

  id          B x H x W    Cin -> Cout   what it exercises
  c64         2 x 9 x 37    64 -> 256    one chunk; partial tiles both ways (the last tile row has 1 valid row, the last
                                         tile column 5 valid pixels); the 2-pixel halo crosses all four image edges
  c128        same         128 -> 256    two chunks: both halo buffers
  c96         same          96 -> 256    CK = 48: LDS slots 6, 7 of every pixel stay unused
  c320        same         320 -> 256    five chunks, buffer reuse: conv_up2's K
  c288        same         288 -> 256    six chunks of 48: conv_up3's K
  d320        1 x 5 x 33   256 -> 320    DATA GRADIENT of conv_up2 (mode-3 filter, against the float64 transposed conv):
                                         10 n-blocks, the second group of the grid's y dimension holds 2 of 8
  d288        1 x 5 x 33   256 -> 288    the same for conv_up3: 9 n-blocks
  n40         1 x 6 x 20    64 ->  40    a partial n-block (8 of 32 channels), one partial tile
  n40bias     1 x 6 x 20    64 ->  40    the bias (read under the same channel bound)
  sliced      2 x 9 x 37    96 -> 256    ldx = 128 > Cin and ldy = 280 > Cout: the operands are channel slices

Operand ranges: integers, |x| <= xr and |w| <= wr, chosen per case so that (a) the sum of |x w| over the 25 Cin terms
stays below 2^24 (conv_ref64 asserts it) and (b) the sum of y^2 over the case's pixels does -- the kernel adds the
squares of a wave's 128 pixels in fp32 before the fp64 atomics; both are asserted on the reference -- while outputs
beyond 256 occur, so that bf16's rounding decides results (fp16 holds every integer up to 2048: no rounding there,
which is what the format gives at the magnitudes (b) allows)."""
import torch

from exact_util import assert_premise, conv_ref64, ints, to_act

# id, (B, H, W), Cin, Cout, bias, dgrad, (ldx, ldy) or None, (xr, wr)
CASES = [
    ("c64", (2, 9, 37), 64, 256, False, False, None, (3, 2)),
    ("c128", (2, 9, 37), 128, 256, False, False, None, (2, 2)),
    ("c96", (2, 9, 37), 96, 256, False, False, None, (2, 2)),
    ("c320", (2, 9, 37), 320, 256, False, False, None, (2, 1)),
    ("c288", (2, 9, 37), 288, 256, False, False, None, (2, 1)),
    ("d320", (1, 5, 33), 256, 320, False, True, None, (2, 2)),
    ("d288", (1, 5, 33), 256, 288, False, True, None, (2, 2)),
    ("n40", (1, 6, 20), 64, 40, False, False, None, (3, 2)),
    ("n40bias", (1, 6, 20), 64, 40, True, False, None, (3, 2)),
    ("sliced", (2, 9, 37), 96, 256, False, False, (128, 280), (2, 2)),
]
IDS = [c[0] for c in CASES]
# the emulation runs the cases of at most two chunks and the first data-gradient case
EMU_IDS = [c[0] for c in CASES if c[2] // (64 if c[2] % 64 == 0 else 48) <= 2] + ["d320"]

_REF = {}


def case_ref(case):
    """Operands and references of a case, computed once: x [B,H,W,Cin] and the OIHW weight `w` of the conv the kernel
    runs (fp32, integer valued), `pack` = (the OIHW weight ssa_pack_filter takes, its mode), bias or None, y64 / y (NHWC;
    float64 and rounded to the storage type), sums [2][Cout] float64 of the ROUNDED outputs."""
    name, (B, H, W), Cin, Cout, bias, dgrad, _, (xr, wr) = case
    if name in _REF:
        return _REF[name]
    seed = 900 + 10 * IDS.index(name)
    x = ints((B, Cin, H, W), -xr, xr, seed)
    b = ints((Cout,), -5, 5, seed + 2) if bias else None
    if dgrad:
        # forward conv Cout -> Cin channels (conv_up2: 320 -> 256) with weight wf; the kernel computes dx from dy = x
        wf = ints((Cin, Cout, 5, 5), -wr, wr, seed + 1)
        w = wf.flip(2, 3).permute(1, 0, 2, 3).contiguous()
        y64 = conv_ref64(x, w, None, 1, 2, 1)
        t64 = torch.nn.functional.conv_transpose2d(x.double(), wf.double(), None, 1, 2)
        assert torch.equal(y64, t64), "the flipped, transposed filter is not the transposed conv"
        pack = (wf, 3)
    else:
        w = ints((Cout, Cin, 5, 5), -wr, wr, seed + 1)
        y64 = conv_ref64(x, w, b, 1, 2, 1)
        pack = (w, 2)
    y64 = y64.permute(0, 2, 3, 1).contiguous()
    y = to_act(y64)
    r = y.double().view(-1, Cout)
    sums = torch.stack([r.sum(0), (r * r).sum(0)])
    assert_premise("conv5x5 %s: sum of y^2 over the pixels" % name, sums[1])
    _REF[name] = dict(x=x.permute(0, 2, 3, 1).contiguous(), w=w, pack=pack, b=b, y64=y64, y=y, sums=sums)
    return _REF[name]
