"""Cases, operands and float64 references of the exact tests of the rectangular-dilation 3x3 conv family
(csrc/conv_dil.hip), shared by tests/test_exact_dilconv_gpu.py (the device) and tests/test_dilconv_emu_cpu.py (the CPU
emulation of both storage builds).  A plain module, not a conftest.

Each case is the smallest at which one mechanism of the kernels can go wrong (forward / data gradient: a workgroup = 64
consecutive pixels of ONE image x 256 channels, a wave 64 x 64, K chunks of 64 channels through a register double buffer,
a per-tile tap list; weight gradient: a workgroup = one tap x 128 x 128 channels, stages of 64 pixels of one image):

  id        B x H x W     Cin -> Cout   dil (h, w)   what it exercises
  r2x12     2 x 13 x 29    64 ->  64    (2, 12)      H != W, 377 pixels per image = 5 tiles + 57 pixels, TWO images: a tap
                                                     below the last row of image 0 must read zero, not image 1; the builder
                                                     asserts ref(dh, dw) != ref(dw, dh)
  r36x30    1 x 40 x 50    64 ->  64    (36, 30)     off-centre taps valid on 4 rows / 20 columns only: per-pixel validity,
                                                     tiles for which whole taps vanish (31 tiles + 16 pixels)
  r12x42    1 x 20 x 50    64 ->  64    (12, 42)     the other orientation
  edge      1 x 13 x 31    64 ->  64    (12, 30)     H = dil_h + 1, W = dil_w + 1: one valid row / column per off-centre tap
  out       1 x 10 x 12    64 ->  64    (36, 30)     every off-centre tap outside (dil > H, W: clamped); the builder asserts
                                                     the reference equals the centre tap's 1x1 conv; eight taps skipped
  sq        2 x 13 x 29    64 ->  64    (2, 2)       rate d of the cell; equals conv_ref64(pad = 2, dil = 2)
  k192      1 x 5 x 15    192 ->  64    (2, 12)      three K chunks: both register buffers, the odd tail step
  k4096     1 x 5 x 15   4096 ->  64    (2, 12)      the cell's largest K: 64 chunks per tap
  n256      1 x 13 x 15    64 -> 256    (12, 6)      the cell's Cout: all four waves of a workgroup live
  n320      1 x 13 x 15    64 -> 320    (12, 6)      a second group of n-blocks with one live wave of four
  dgrad     1 x 13 x 29   256 ->  64    (2, 12)      DATA GRADIENT: mode-3 filter against the float64 conv_transpose2d of a
                                                     64 -> 256 forward conv; the builder asserts that equals the flipped,
                                                     transposed conv
  sliced    2 x 13 x 29    64 ->  64    (12, 6)      x = channels [0, 64) and y = channels [64, 128) of ONE [B,H,W,320]
                                                     buffer; the channels outside y's slice keep a sentinel

Weight-gradient cases (x [B,H,W,Cin], dy [B,H,W,Cout]):

  wg_r2x12  2 x 13 x 29    64 ->  64    (2, 12)      two images, 6 stages each (the last of 57 pixels), 12 splits
  wg_r36x30 1 x 40 x 50    64 ->  64    (36, 30)     stages for which the tap is outside are skipped
  wg_out    1 x 10 x 12    64 ->  64    (36, 30)     the eight off-centre taps of dW are exactly zero and WRITTEN
  wg_split  1 x 40 x 50   192 -> 128    (12, 6)      32 stages over 16 splits of 2; two ci blocks (the second half full)

Operand ranges: integers, |x| <= xr and |w| <= wr, chosen per case so that (a) the sum of |x w| over the 9 Cin terms
stays below 2^24 (conv_ref64 asserts it) and (b) the sum of y^2 over the case's pixels does -- the kernel adds the
squares of a wave's 64 pixels in fp32 before the fp64 atomics; both are asserted on the reference -- while outputs
beyond 256 occur, so that bf16's rounding decides results (fp16 holds every integer up to 2048: no rounding there)."""
import torch

from exact_util import assert_premise, conv_ref64, ints, to_act, to_f32, wgrad_ref64

BM, BN, CK = 64, 256, 64          # pixels per tile, channels per workgroup, channels per K chunk (csrc/conv_dil.hip)
WG_BP, WG_BC = 64, 128            # weight gradient: pixels per stage, channels per block

# id, (B, H, W), Cin, Cout, (dil_h, dil_w), kind, (xr, wr);  kind: "fwd", "dgrad", "sliced"
CASES = [
    ("r2x12", (2, 13, 29), 64, 64, (2, 12), "fwd", (3, 2)),
    ("r36x30", (1, 40, 50), 64, 64, (36, 30), "fwd", (3, 2)),
    ("r12x42", (1, 20, 50), 64, 64, (12, 42), "fwd", (3, 2)),
    ("edge", (1, 13, 31), 64, 64, (12, 30), "fwd", (3, 2)),
    ("out", (1, 10, 12), 64, 64, (36, 30), "fwd", (5, 4)),
    ("sq", (2, 13, 29), 64, 64, (2, 2), "fwd", (3, 2)),
    ("k192", (1, 5, 15), 192, 64, (2, 12), "fwd", (2, 2)),
    ("k4096", (1, 5, 15), 4096, 64, (2, 12), "fwd", (1, 1)),
    ("n256", (1, 13, 15), 64, 256, (12, 6), "fwd", (3, 2)),
    ("n320", (1, 13, 15), 64, 320, (12, 6), "fwd", (3, 2)),
    ("dgrad", (1, 13, 29), 256, 64, (2, 12), "dgrad", (2, 2)),
    ("sliced", (2, 13, 29), 64, 64, (12, 6), "sliced", (3, 2)),
]
IDS = [c[0] for c in CASES]
SLICED_LD = 320

# id, (B, H, W), Cin, Cout, (dil_h, dil_w)
WG_CASES = [
    ("wg_r2x12", (2, 13, 29), 64, 64, (2, 12)),
    ("wg_r36x30", (1, 40, 50), 64, 64, (36, 30)),
    ("wg_out", (1, 10, 12), 64, 64, (36, 30)),
    ("wg_split", (1, 40, 50), 192, 128, (12, 6)),
]
WG_IDS = [c[0] for c in WG_CASES]

# the three problems of the grouped launch: one shape (r12x42 cropped to r2x12's), three rate pairs
GROUPED = [("r2x12", (2, 12)), ("r12x42", (12, 42)), ("sq", (2, 2))]

_REF = {}


def geometry(case):
    """Mirror of the forward launch geometry (not read from the kernel)."""
    _, (B, H, W), Cin, Cout, _, _, _ = case
    tiles = -(-(H * W) // BM)
    return dict(tiles=tiles, last=H * W - (tiles - 1) * BM, chunks=Cin // CK, groups=-(-Cout // BN),
                last_waves=(Cout - (-(-Cout // BN) - 1) * BN) // 64)


def wg_plan(case):
    """Mirror of plan_wgrad (csrc/conv_dil.hip)."""
    _, (B, H, W), Cin, Cout, _ = case
    ntile = -(-Cin // WG_BC) * -(-Cout // WG_BC) * 9
    stages_img = -(-(H * W) // WG_BP)
    total = B * stages_img
    ns = max(1, min(16, total, 768 // ntile))
    per = -(-total // ns)
    return dict(ntile=ntile, stages_img=stages_img, total=total, nsplit=-(-total // per), per=per)


def tap_valid_counts(H, W, dil):
    """Per off-centre tap offset: (rows, columns) of output pixels for which the tap is inside the image."""
    return max(0, H - dil[0]), max(0, W - dil[1])


def conv(x, w, dil):
    return conv_ref64(x, w, None, 1, tuple(dil), tuple(dil))


def case_ref(case):
    """Operands and references of a case, computed once: x [B,H,W,Cin] (NHWC, fp32 integers), `pack` = (the OIHW weight
    ssa_pack_filter takes, its mode), y64 / y (NHWC; float64 and rounded to the storage type), sums [2][Cout] float64 of
    the ROUNDED outputs."""
    name, (B, H, W), Cin, Cout, dil, kind, (xr, wr) = case
    if name in _REF:
        return _REF[name]
    seed = 4100 + 10 * IDS.index(name)
    x = ints((B, Cin, H, W), -xr, xr, seed)
    if kind == "dgrad":
        # forward conv Cout -> Cin channels (64 -> 256) with weight wf; the kernel computes dx (Cout = 64) from dy = x
        wf = ints((Cin, Cout, 3, 3), -wr, wr, seed + 1)
        w = wf.flip(2, 3).permute(1, 0, 2, 3).contiguous()
        y64 = conv(x, w, dil)
        t64 = torch.nn.functional.conv_transpose2d(x.double(), wf.double(), None, 1, tuple(dil), 0, 1, tuple(dil))
        assert torch.equal(y64, t64), "the flipped, transposed filter is not the transposed conv"
        pack = (wf, 3)
    else:
        w = ints((Cout, Cin, 3, 3), -wr, wr, seed + 1)
        y64 = conv(x, w, dil)
        pack = (w, 2)
    if name == "r2x12":
        assert not torch.equal(y64, conv(x, w, (dil[1], dil[0]))), "the case cannot tell (dh, dw) from (dw, dh)"
    if name == "out":
        assert H <= dil[0] and W <= dil[1]
        assert torch.equal(y64, conv_ref64(x, w[:, :, 1:2, 1:2].contiguous())), "an off-centre tap is inside the image"
    if name == "sq":
        assert torch.equal(y64, conv_ref64(x, w, None, 1, dil[0], dil[0]))
    if name == "edge":
        assert tap_valid_counts(H, W, dil) == (1, 1)
    if name == "r36x30":
        assert tap_valid_counts(H, W, dil) == (4, 20)
    y64 = y64.permute(0, 2, 3, 1).contiguous()
    y = to_act(y64)
    r = y.double().view(-1, Cout)
    sums = torch.stack([r.sum(0), (r * r).sum(0)])
    assert_premise("dilconv %s: sum of y^2 over the pixels" % name, sums[1])
    _REF[name] = dict(x=x.permute(0, 2, 3, 1).contiguous(), w=w, pack=pack, y64=y64, y=y, sums=sums)
    return _REF[name]


def grouped_refs():
    """The three problems of the grouped launch: r2x12's input (b, c, d of the cell read one input) under the three rate
    pairs, each with its own case's filter.  The test compares the grouped launch with the single launches AND with these
    float64 results."""
    if "grouped" in _REF:
        return _REF["grouped"]
    x = case_ref(CASES[IDS.index("r2x12")])["x"]
    out = []
    for cid, dil in GROUPED:
        w = case_ref(CASES[IDS.index(cid)])["w"]
        y64 = conv(x.permute(0, 3, 1, 2), w, dil).permute(0, 2, 3, 1).contiguous()
        out.append(dict(dil=dil, x=x, w=w, y=to_act(y64)))
    _REF["grouped"] = out
    return out


def wg_ref(case):
    """x, dy (NHWC fp32 integers) and dw [Cout][Cin][3][3] fp32 (exact) of a weight-gradient case."""
    name, (B, H, W), Cin, Cout, dil = case
    if name in _REF:
        return _REF[name]
    seed = 4500 + 10 * WG_IDS.index(name)
    x = ints((B, Cin, H, W), -2, 2, seed)
    dy = ints((B, Cout, H, W), -2, 2, seed + 1)
    dw64 = wgrad_ref64(x, dy, 3, 1, tuple(dil), tuple(dil))
    if name == "wg_out":
        off = torch.ones(3, 3, dtype=torch.bool)
        off[1, 1] = False
        assert float(dw64[:, :, off].abs().max()) == 0.0 and float(dw64[:, :, 1, 1].abs().max()) > 0.0
    _REF[name] = dict(x=x.permute(0, 2, 3, 1).contiguous(), dy=dy.permute(0, 2, 3, 1).contiguous(), dw=to_f32(dw64))
    return _REF[name]
