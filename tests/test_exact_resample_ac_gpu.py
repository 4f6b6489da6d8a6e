"""Exact and bounded tests of the align_corners=True bilinear kernels (csrc/resample.hip) through the ssa_resize_* entry
points of the C ABI, through the autograd Functions of semseg_amd/hip_backend.py and through eval_tail.resize_tensor.

Method of tests/test_kernels_gpu.py's exact resampling tests: integer operands at power-of-two ratios -- under this rule
sizes of the form k 2^m + 1 -- so that every partial sum is exact in fp32 (premise asserted on the float64 reference,
tests/resample_ac_ref.py, never on the kernel) and results are compared bit for bit; per element within resize_bound_ac
elsewhere.  Every input sits in a NaN-guarded buffer, every output starts as NaN.  Cases: tests/resample_ac_cases.py.
The file also runs on the CPU emulation of the kernels (tests/test_resample_ac_emu_cpu.py)."""
import os

import pytest
import torch

import resample_ac_cases as AC
from exact_util import (LIMIT, assert_bits_equal, assert_guard_intact, assert_within_bound, guarded, guarded_copy, ints,
                        to_act, to_f32)
from resample_ac_ref import (exact_grad_x_ac, exact_resize_ac, exact_resize_grad_ac, grad_amp_ac, is_dyadic_ac, resize_bound_ac,
                             resize_grad_ref64_ac, resize_ref64_ac)
from util import ACT_DTYPE, nhwc

pytestmark = pytest.mark.gpu

DEV = "cuda"
_GRID_CAP = 8192 * 256            # grid_for of csrc/resample.hip: threads in flight before a kernel's grid-stride loop turns
_TILE_CAP = 16384                 # workgroups of the LDS-tiled backward (4 x 16 input pixels each)
_EINVAL = -1


def _rs():
    from semseg_amd import hip_backend as hb
    from semseg_amd._lib import check
    return hb, hb.lib(), check


def _dt(is16):
    return ACT_DTYPE if is16 else torch.float32


def _want(ref64, is16):
    return to_act(ref64) if is16 else to_f32(ref64)


def _ld4(g):
    return g.view.stride(2)


def _fwd(x, in16, out16, Ho, Wo, pads=(0, 0), ac=1):
    """x [B, Hi, Wi, C] (host) through ssa_resize_bilinear_fwd: (guarded input, guarded output)."""
    hb, L, check = _rs()
    Bn, Hi, Wi, C = x.shape
    xg = guarded_copy(x.to(_dt(in16)), DEV, C + pads[0])
    yg = guarded((Bn, Ho, Wo, C), _dt(out16), DEV, C + pads[1])
    check(L.ssa_resize_bilinear_fwd(hb._p(xg.view), 0 if in16 else 1, Bn, Hi, Wi, C, _ld4(xg), hb._p(yg.view), 0 if out16 else 1,
                                    Ho, Wo, _ld4(yg), ac, hb._s()), "ssa_resize_bilinear_fwd")
    return xg, yg


def _bwd(dy, dy16, dx16, Hi, Wi, pads=(0, 0), ac=1):
    hb, L, check = _rs()
    Bn, Ho, Wo, C = dy.shape
    dyg = guarded_copy(dy.to(_dt(dy16)), DEV, C + pads[0])
    dxg = guarded((Bn, Hi, Wi, C), _dt(dx16), DEV, C + pads[1])
    check(L.ssa_resize_bilinear_bwd(hb._p(dyg.view), 0 if dy16 else 1, Bn, Ho, Wo, C, _ld4(dyg), hb._p(dxg.view), 0 if dx16 else 1,
                                    Hi, Wi, _ld4(dxg), ac, hb._s()), "ssa_resize_bilinear_bwd")
    return dyg, dxg


def _bwd_sep(dy, dy16, dx16, Hi, Wi, pads=(0, 0), ac=1):
    """The separable pair: (guarded dy, guarded fp32 tmp [B, Ho, Wi, C], guarded dx)."""
    hb, L, check = _rs()
    Bn, Ho, Wo, C = dy.shape
    dyg = guarded_copy(dy.to(_dt(dy16)), DEV, C + pads[0])
    tg = guarded((Bn, Ho, Wi, C), torch.float32, DEV)
    dxg = guarded((Bn, Hi, Wi, C), _dt(dx16), DEV, C + pads[1])
    check(L.ssa_resize_bilinear_bwd_x(hb._p(dyg.view), 0 if dy16 else 1, Bn, Ho, Wo, C, _ld4(dyg), hb._p(tg.view), Wi, ac, hb._s()),
          "ssa_resize_bilinear_bwd_x")
    check(L.ssa_resize_bilinear_bwd_y(hb._p(tg.view), Bn, Ho, Wi, C, hb._p(dxg.view), 0 if dx16 else 1, Hi, _ld4(dxg), ac, hb._s()),
          "ssa_resize_bilinear_bwd_y")
    return dyg, tg, dxg


@pytest.fixture()
def flag_on():
    """cfg.MODEL.ALIGN_CORNERS = True for one test, restored whatever happens."""
    from semseg_amd.config import cfg
    prev = cfg.MODEL.ALIGN_CORNERS
    cfg.MODEL.ALIGN_CORNERS = True
    try:
        yield cfg
    finally:
        cfg.MODEL.ALIGN_CORNERS = prev


# ---- exact by route
@pytest.mark.parametrize("case", AC.FWD_EXACT, ids=[c[0] for c in AC.FWD_EXACT])
def test_exact_ac_fwd(case):
    """ssa_resize_bilinear_fwd(align_corners=1) bit for bit on its three kernels (8 channels per thread, per pixel, per
    element in the four dtype pairs), dense and with leading dimensions that differ from C, scale 0 included."""
    name, C, Hi, Wi, Ho, Wo, in16, out16, pads = case
    x = AC.fwd_operand(case)
    ref = exact_resize_ac(name, x, Ho, Wo)
    xg, yg = _fwd(x, in16, out16, Ho, Wo, pads)
    torch.cuda.synchronize()
    assert_bits_equal("resize_bilinear_fwd %s" % name, yg.view.cpu(), _want(ref, out16))
    assert_guard_intact("resize_bilinear_fwd %s" % name, xg, yg)


@pytest.mark.parametrize("case", AC.BWD_EXACT, ids=[c[0] for c in AC.BWD_EXACT])
def test_exact_ac_bwd(case):
    """ssa_resize_bilinear_bwd(align_corners=1) bit for bit: the vectorised gather (hoisted and recomputed weights), the
    per-element gather and the LDS-tiled kernel (TAPS 4, 8 and 12; 8 and 32 channels; ragged, full and one-pixel tiles)."""
    name, C, Hi, Wi, Ho, Wo, dy16, dx16, pads = case
    dy = AC.bwd_operand(case)
    ref = exact_resize_grad_ac(name, dy, Hi, Wi)
    dyg, dxg = _bwd(dy, dy16, dx16, Hi, Wi, pads)
    torch.cuda.synchronize()
    assert_bits_equal("resize_bilinear_bwd %s" % name, dxg.view.cpu(), _want(ref, dx16))
    assert_guard_intact("resize_bilinear_bwd %s" % name, dyg, dxg)


@pytest.mark.parametrize("case", AC.SEP_EXACT, ids=[c[0] for c in AC.SEP_EXACT])
def test_exact_ac_bwd_separable(case):
    """ssa_resize_bilinear_bwd_x then _y: the fp32 intermediate AND the result bit for bit (a failure is located to a
    pass), and the one-launch form of the same problem equal to the same reference."""
    name, C, Hi, Wi, Ho, Wo, dy16, dx16, pads = case
    dy = AC.bwd_operand(case)
    ref = exact_resize_grad_ac(name, dy, Hi, Wi)
    tref = exact_grad_x_ac(name, dy, Wi)
    dyg, tg, dxg = _bwd_sep(dy, dy16, dx16, Hi, Wi, pads)
    torch.cuda.synchronize()
    assert_bits_equal("resize_bilinear_bwd_x %s" % name, tg.view.cpu(), to_f32(tref))
    assert_bits_equal("resize_bilinear_bwd_y %s" % name, dxg.view.cpu(), _want(ref, dx16))
    assert_guard_intact("resize_bilinear_bwd_x/_y %s" % name, dyg, tg, dxg)
    if dy16 == dx16 or not dy16:                          # (the one-launch form has no 16-bit -> fp32 pair)
        dyg2, dxg2 = _bwd(dy, dy16, dx16, Hi, Wi, pads)
        torch.cuda.synchronize()
        assert_bits_equal("resize_bilinear_bwd (one launch) %s" % name, dxg2.view.cpu(), _want(ref, dx16))
        assert_guard_intact("resize_bilinear_bwd (one launch) %s" % name, dyg2, dxg2)


# the Python dispatch: (id, C, Hi, Wi, Ho, Wo, x 16-bit, output fp32, layout)
_AUTOGRAD = [
    ("v8-separable", 48, 5, 7, 17, 25, True, False, "dense"),          # separable() true: bwd_x / bwd_y
    ("v8-separable-2x4", 48, 5, 7, 9, 25, True, False, "dense"),       # Ho = 9 < 2 * 5: under this rule the gather
    ("v8-separable-8x", 16, 3, 5, 17, 33, True, False, "dense"),
    ("v8-gather-down", 48, 9, 13, 5, 7, True, False, "dense"),
    ("v8-slices", 48, 5, 7, 17, 25, True, False, "slices"),            # x a channel slice; dy a slice with ld % 8 != 0: re-packed
    ("px-tile", 19, 9, 21, 33, 81, False, True, "dense"),
    ("px16-tile16", 19, 9, 21, 33, 81, True, True, "dense"),
    ("px-tile-slices", 19, 9, 21, 17, 41, False, True, "slices"),
    ("el-f32", 40, 9, 21, 17, 41, False, True, "dense"),
    ("el-16", 19, 5, 9, 9, 17, True, False, "slices"),
    ("v8-from1", 48, 1, 1, 4, 6, True, False, "dense"),                # scale 0 through the separable pair
    ("px-to1", 19, 5, 7, 1, 1, False, True, "dense"),
]


@pytest.mark.parametrize("case", _AUTOGRAD, ids=[c[0] for c in _AUTOGRAD])
def test_exact_ac_autograd(case):
    """One pass per route through BilinearFn with the flag given explicitly; the backward runs under the forward's rule
    (kept in ctx) although cfg.MODEL.ALIGN_CORNERS is off all along."""
    hb = _rs()[0]
    from semseg_amd.config import cfg
    assert not cfg.MODEL.ALIGN_CORNERS
    name, C, Hi, Wi, Ho, Wo, x16, out_f32, layout = case
    x, dy = AC.fwd_operand(case), AC.bwd_operand(case)
    ref, gref = exact_resize_ac(name, x, Ho, Wo), exact_resize_grad_ac(name, dy, Hi, Wi)
    out16 = x16 and not out_f32
    if layout == "dense":
        xd = x.to(_dt(x16)).to(DEV).requires_grad_(True)
        dyd = dy.to(_dt(out16)).to(DEV)
    else:
        xg = guarded_copy(x.to(_dt(x16)), DEV, C + 8)
        dyg = guarded_copy(dy.to(_dt(out16)), DEV, C + 4)
        xd, dyd = xg.view.detach().requires_grad_(True), dyg.view
    yd = hb.BilinearFn.apply(xd, Ho, Wo, out_f32, True)
    yd.backward(dyd)
    torch.cuda.synchronize()
    assert_bits_equal("BilinearFn %s forward" % name, yd.detach().cpu(), _want(ref, out16))
    assert_bits_equal("BilinearFn %s backward" % name, xd.grad.cpu(), _want(gref, x16))
    if layout != "dense":
        assert_guard_intact("BilinearFn %s" % name, xg, dyg)


def test_exact_ac_backend_reads_the_flag(flag_on):
    """ops.HipBackend.bilinear / upsample_cat / image_to_nhwc read cfg.MODEL.ALIGN_CORNERS when called: an identity copy,
    a 2x and a 4x resize written into channel slices of one buffer (ldy = 80), the backward reading its slices of the
    gradient in place; a grouped bilinear of two problems; the image resize."""
    from semseg_amd import ops
    be = ops.HipBackend()
    shapes = [(16, 17, 25), (48, 9, 13), (16, 5, 7)]
    Ho, Wo = 17, 25
    xs = [ints((AC.B, H, W, C), -200, 200, 420 + i) for i, (C, H, W) in enumerate(shapes)]
    amps = [grad_amp_ac(Ho, H, Wo, W, 200) for C, H, W in shapes]
    dys = [ints((AC.B, Ho, Wo, C), -a, a, 430 + i) for i, ((C, H, W), a) in enumerate(zip(shapes, amps))]
    want = torch.cat([to_act(exact_resize_ac("cat %d" % i, x, Ho, Wo)) for i, x in enumerate(xs)], 3)
    gwant = [to_act(exact_resize_grad_ac("cat %d" % i, dy, H, W)) for i, (dy, (C, H, W)) in enumerate(zip(dys, shapes))]
    xgs = [guarded_copy(x.to(ACT_DTYPE), DEV) for x in xs]
    leaves = [g.view.detach().requires_grad_(True) for g in xgs]
    dyg = guarded_copy(torch.cat(dys, 3).to(ACT_DTYPE), DEV)
    (y,) = be.upsample_cat([leaves])
    y.backward(dyg.view)
    torch.cuda.synchronize()
    assert_bits_equal("upsample_cat forward", y.detach().cpu(), want)
    for i, leaf in enumerate(leaves):
        assert_bits_equal("upsample_cat backward %d" % i, leaf.grad.cpu(), gwant[i])
    assert_guard_intact("upsample_cat", dyg, *xgs)
    # grouped: two problems of different ratios in one call
    ls = [x.to(ACT_DTYPE).to(DEV).requires_grad_(True) for x in xs[1:]]
    ys = be.bilinear(ls, [(Ho, Wo), (Ho, Wo)])
    torch.autograd.backward(ys, [dy.to(ACT_DTYPE).to(DEV) for dy in dys[1:]])
    torch.cuda.synchronize()
    for i in (0, 1):
        assert_bits_equal("bilinear group forward %d" % i, ys[i].detach().cpu(), to_act(exact_resize_ac("g", xs[i + 1], Ho, Wo)))
        assert_bits_equal("bilinear group backward %d" % i, ls[i].grad.cpu(), gwant[i + 1])
    # the image resize
    img = ints((AC.B, 3, 9, 21), -250, 250, 450)
    iw = torch.zeros((AC.B, 17, 81, 16), dtype=ACT_DTYPE)
    iw[..., :3] = to_act(exact_resize_ac("image", nhwc(img), 17, 81))
    got = be.image_to_nhwc(img.to(DEV), (17, 81))
    torch.cuda.synchronize()
    assert_bits_equal("image_to_nhwc", got.cpu(), iw)


def test_exact_ac_eval_tail_resize_tensor(flag_on):
    """utils/eval_tail.resize_tensor (the evaluation's resize of the logits, NCHW in and out) with the flag on -- and off
    again afterwards, where the same call gives the other rule's result."""
    import importlib
    from resample_ref import exact_resize
    eval_tail = importlib.import_module("semseg_amd.utils.eval_tail")      # (the package re-exports a function of that name)
    x = ints((AC.B, 9, 21, 19), -200, 200, 460)
    xd = x.permute(0, 3, 1, 2).contiguous().to(DEV)
    y = eval_tail.resize_tensor(xd, (33, 81))
    torch.cuda.synchronize()
    assert tuple(y.shape) == (AC.B, 19, 33, 81)
    assert_bits_equal("resize_tensor", y.permute(0, 2, 3, 1).contiguous().cpu(), to_f32(exact_resize_ac("eval", x, 33, 81)))
    flag_on.MODEL.ALIGN_CORNERS = False
    y0 = eval_tail.resize_tensor(xd, (36, 84))
    torch.cuda.synchronize()
    assert_bits_equal("resize_tensor, flag off", y0.permute(0, 2, 3, 1).contiguous().cpu(), to_f32(exact_resize("eval", x, 36, 84)))


# ---- bounded by route
def _bounded(tag, got, ref, bound):
    def over(e, b):                                         # e / b per element; a zero bound allows no error at all
        return torch.where(b > 0, e / b.clamp_min(1e-300), torch.where(e > 0, torch.full_like(e, float("inf")), torch.zeros_like(e)))
    err = (got.detach().double().cpu() - ref).abs()
    print("[resize_bound_ac] %-36s worst error / bound = %.3g" % (tag, float(over(err, bound.expand_as(err)).max())))
    assert_within_bound("resize_bound_ac " + tag, got, ref, bound)           # NaN-safe: an unwritten output is a violation


@pytest.mark.parametrize("case", AC.BOUNDED, ids=[c[0] for c in AC.BOUNDED])
def test_exact_ac_bounded(case):
    """Ratios that are not dyadic: every element of forward and backward within resize_bound_ac of the float64 reference,
    dense and sliced; the 16-bit upsampling cases through the separable pair as well."""
    name, C, Hi, Wi, Ho, Wo, is16 = case
    x, dy = AC.bounded_operands(case)
    ref, _ = resize_ref64_ac(x, Ho, Wo)
    gref, _ = resize_grad_ref64_ac(dy, Hi, Wi)
    bf = resize_bound_ac(x, Ho, Wo, Hi, Wi, False, is16, ref)
    bb = resize_bound_ac(dy, Ho, Wo, Hi, Wi, True, is16, gref)
    for pads in ((0, 0), (16, 8) if is16 else (5, 3)):
        tag = "%s %s" % (name, "dense" if pads == (0, 0) else "sliced")
        xg, yg = _fwd(x, is16, is16, Ho, Wo, pads)
        dyg, dxg = _bwd(dy, is16, is16, Hi, Wi, pads)
        torch.cuda.synchronize()
        _bounded("fwd " + tag, yg.view, ref, bf)
        _bounded("bwd " + tag, dxg.view, gref, bb)
        assert_guard_intact("bilinear bounded " + tag, xg, yg, dyg, dxg)
        if is16 and Ho >= 2 * Hi and Wo >= 2 * Wi:
            dyg, tg, dxg = _bwd_sep(dy, True, True, Hi, Wi, pads)
            torch.cuda.synchronize()
            _bounded("bwd separable " + tag, dxg.view, gref, bb)
            assert_guard_intact("bilinear bounded separable " + tag, dyg, tg, dxg)


# ---- the grid-stride loops (GPU only)
def _dev_ints(shape, amp, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-amp, amp + 1, shape, generator=g, device=DEV, dtype=torch.int32)


def _dev_resize64(x, Ho, Wo):
    """torch's own float64 interpolate on the device, NHWC in and out (any correct float64 bilinear is THE reference at a
    dyadic ratio); with it the same of |x| for the premise."""
    F = torch.nn.functional
    xd = x.permute(0, 3, 1, 2).double()
    y = F.interpolate(xd, size=(Ho, Wo), mode="bilinear", align_corners=True)
    mag = float(F.interpolate(xd.abs(), size=(Ho, Wo), mode="bilinear", align_corners=True).max())
    return y.permute(0, 2, 3, 1).contiguous(), mag


def _dev_grad64(dy, Hi, Wi):
    """The float64 gradient of that interpolate (ATen's own backward), image by image to bound the memory."""
    Bn, Ho, Wo, C = dy.shape
    out, mag = [], 0.0
    for b in range(Bn):
        g = dy[b:b + 1].permute(0, 3, 1, 2).double().contiguous()
        out.append(torch.ops.aten.upsample_bilinear2d_backward(g, [Ho, Wo], [1, C, Hi, Wi], True, None, None).permute(0, 2, 3, 1))
        mag = max(mag, float(torch.ops.aten.upsample_bilinear2d_backward(g.abs(), [Ho, Wo], [1, C, Hi, Wi], True, None, None).max()))
        del g
    return torch.cat(out).contiguous(), mag


def _dev_want(tag, ref64, mag, is16, sizes):
    """The premise of the exact tests, asserted on the device reference; the reference in the output's format."""
    for n_out, n_in in sizes:
        assert is_dyadic_ac(n_out, n_in), (tag, n_out, n_in)
    assert mag * 65536.0 < LIMIT, "%s: exactness premise violated: the magnitude product reaches %g" % (tag, mag)
    f = ref64.float()
    assert torch.equal(f.double(), ref64), "%s: the reference is not exact in fp32" % tag
    return f.to(ACT_DTYPE) if is16 else f


def _dev_bits_equal(tag, got, want):
    it = torch.int16 if got.element_size() == 2 else torch.int32
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = got.contiguous().view(it) != want.contiguous().view(it)
    n = int(bad.sum())
    if n:
        b, h = (int(v) for v in bad.nonzero()[0][:2])
        assert_bits_equal("%s: %d elements differ in all, first in image %d row %d" % (tag, n, b, h),
                          got[b, h].cpu(), want[b, h].cpu())


def _dev_operand(shape, amp, seed, is16, ld):
    v = _dev_ints(shape, amp, seed)
    g = guarded(shape, _dt(is16), DEV, ld)
    g.view.copy_(v)
    assert torch.equal(g.view.to(torch.int32), v), "operand not representable"
    return g


_GS_KERNELS = ["fwd-v8", "fwd-px", "fwd-el", "bwd-v8-and-separable", "bwd-el", "bwd-tile"]


@pytest.mark.skipif(bool(os.environ.get("SSA_EMU")), reason="2 M threads and more: GPU only")
@pytest.mark.parametrize("kernel", _GS_KERNELS)
def test_exact_ac_grid_stride(kernel):
    """One exact 2x (0.5x) case per kernel just past its grid cap -- 8192 x 256 threads, 16384 tiles for the tiled
    backward -- at sizes that are no multiple of 256 or of the tile, so that the grid-stride loop turns and its last
    turn is ragged.  Reference and comparison on the device."""
    hb, L, check = _rs()
    Bn, C = AC.B, 8
    if kernel.startswith("fwd"):
        Hi = Wi = 515
        Ho = Wo = 1029
        in16, out16, pads = {"fwd-v8": (True, True, (8, 24)), "fwd-px": (False, False, (5, 0)), "fwd-el": (False, True, (5, 3))}[kernel]
        threads = Bn * Ho * Wo * (C if kernel == "fwd-el" else 1)
        assert threads > _GRID_CAP and threads % 256
        xg = _dev_operand((Bn, Hi, Wi, C), 200, 440, in16, C + pads[0])
        yg = guarded((Bn, Ho, Wo, C), _dt(out16), DEV, C + pads[1])
        check(L.ssa_resize_bilinear_fwd(hb._p(xg.view), 0 if in16 else 1, Bn, Hi, Wi, C, _ld4(xg), hb._p(yg.view), 0 if out16 else 1,
                                        Ho, Wo, _ld4(yg), 1, hb._s()), "ssa_resize_bilinear_fwd")
        ref, mag = _dev_resize64(xg.view, Ho, Wo)
        want = _dev_want(kernel, ref, mag, out16, [(Ho, Hi), (Wo, Wi)])
        if out16 and ACT_DTYPE == torch.bfloat16:
            assert int((want.double() != ref).sum()) > 0, "no output needs rounding"
        torch.cuda.synchronize()
        _dev_bits_equal("grid stride " + kernel, yg.view, want)
        assert_guard_intact("grid stride " + kernel, xg, yg)
        return
    if kernel == "bwd-v8-and-separable":
        Hi = Wi = 1030
        Ho = Wo = 2059
        assert Bn * Hi * Wi > _GRID_CAP and Bn * Ho * Wi > _GRID_CAP and (Bn * Hi * Wi) % 256        # pass Y / the gather; pass X
        dyg = _dev_operand((Bn, Ho, Wo, C), grad_amp_ac(Ho, Hi, Wo, Wi), 441, True, C + 8)
        tg = guarded((Bn, Ho, Wi, C), torch.float32, DEV)
        dxg, dxg2 = (guarded((Bn, Hi, Wi, C), ACT_DTYPE, DEV, C + 8) for _ in range(2))
        check(L.ssa_resize_bilinear_bwd_x(hb._p(dyg.view), 0, Bn, Ho, Wo, C, _ld4(dyg), hb._p(tg.view), Wi, 1, hb._s()),
              "ssa_resize_bilinear_bwd_x")
        check(L.ssa_resize_bilinear_bwd_y(hb._p(tg.view), Bn, Ho, Wi, C, hb._p(dxg.view), 0, Hi, _ld4(dxg), 1, hb._s()),
              "ssa_resize_bilinear_bwd_y")
        check(L.ssa_resize_bilinear_bwd(hb._p(dyg.view), 0, Bn, Ho, Wo, C, _ld4(dyg), hb._p(dxg2.view), 0, Hi, Wi, _ld4(dxg2), 1,
                                        hb._s()), "ssa_resize_bilinear_bwd")
        tref, tmag = _dev_grad64(dyg.view, Ho, Wi)                                                   # the X pass alone: a 1x resize in y
        twant = _dev_want(kernel + " pass X", tref, tmag, False, [(Wo, Wi)])
        del tref
        ref, mag = _dev_grad64(dyg.view, Hi, Wi)
        want = _dev_want(kernel, ref, mag, True, [(Ho, Hi), (Wo, Wi)])
        torch.cuda.synchronize()
        _dev_bits_equal("grid stride bwd_x", tg.view, twant)
        _dev_bits_equal("grid stride bwd_y", dxg.view, want)
        _dev_bits_equal("grid stride vectorised gather", dxg2.view, want)
        assert_guard_intact("grid stride " + kernel, dyg, tg, dxg, dxg2)
        return
    if kernel == "bwd-el":                                   # 0.5x: a downsampling gradient never takes the tiled route
        Hi = Wi = 1029
        Ho = Wo = 515
        assert Bn * Hi * Wi * C > _GRID_CAP
    else:                                                    # 2 * 183 * 46 tiles of 4 x 16; 730 = 182 * 4 + 2 = 45 * 16 + 10
        Hi = Wi = 730
        Ho = Wo = 1459
        assert Bn * (-(-Hi // 4)) * (-(-Wi // 16)) > _TILE_CAP and Hi % 4 and Wi % 16
    dyg = _dev_operand((Bn, Ho, Wo, C), grad_amp_ac(Ho, Hi, Wo, Wi, 200), 442, False, C + 5)
    dxg = guarded((Bn, Hi, Wi, C), torch.float32, DEV, C + 3)
    check(L.ssa_resize_bilinear_bwd(hb._p(dyg.view), 1, Bn, Ho, Wo, C, _ld4(dyg), hb._p(dxg.view), 1, Hi, Wi, _ld4(dxg), 1, hb._s()),
          "ssa_resize_bilinear_bwd")
    ref, mag = _dev_grad64(dyg.view, Hi, Wi)
    want = _dev_want(kernel, ref, mag, False, [(Ho, Hi), (Wo, Wi)])
    torch.cuda.synchronize()
    _dev_bits_equal("grid stride " + kernel, dxg.view, want)
    assert_guard_intact("grid stride " + kernel, dyg, dxg)


# ---- the image resize
def _image_resize(x, Ho, Wo, cpad=16, ac=1):
    hb, L, check = _rs()
    Bn, C, Hi, Wi = x.shape
    xg = guarded_copy(x, DEV)
    yg = guarded((Bn, Ho, Wo, cpad), ACT_DTYPE, DEV)
    check(L.ssa_image_resize_to_nhwc(hb._p(xg.view), Bn, C, Hi, Wi, hb._p(yg.view), Ho, Wo, cpad, ac, hb._s()),
          "ssa_image_resize_to_nhwc")
    return xg, yg


@pytest.mark.parametrize("Hi,Wi,Ho,Wo", [(9, 13, 5, 7), (9, 21, 9, 21), (9, 21, 17, 41), (9, 21, 33, 41), (1, 7, 4, 13), (5, 7, 1, 1)],
                         ids=["half", "copy", "2x", "4x-by-2x", "from1-y", "to1"])
def test_exact_ac_image_resize(Hi, Wi, Ho, Wo):
    """ssa_image_resize_to_nhwc(align_corners=1) of an integer image: the three channels bit for bit, the thirteen
    padding channels exactly zero, nothing written around the output; and hip_backend.image_to_nhwc with the flag."""
    x = ints((AC.B, 3, Hi, Wi), -250, 250, 450)
    ref = exact_resize_ac("image", nhwc(x), Ho, Wo)
    want = torch.zeros((AC.B, Ho, Wo, 16), dtype=ACT_DTYPE)
    want[..., :3] = to_act(ref)
    xg, yg = _image_resize(x, Ho, Wo)
    torch.cuda.synchronize()
    assert_bits_equal("image_resize", yg.view.cpu(), want)
    assert_guard_intact("image_resize", xg, yg)
    through = _rs()[0].image_to_nhwc(xg.view, None if (Hi, Wi) == (Ho, Wo) else (Ho, Wo), align_corners=True)
    torch.cuda.synchronize()
    assert_bits_equal("image_to_nhwc", through.cpu(), want)


def test_exact_ac_image_resize_bounded():
    """A size that is not dyadic: every element within resize_bound_ac, the padding exactly zero."""
    Hi, Wi, Ho, Wo = 13, 17, 40, 27
    x = ints((AC.B, 3, Hi, Wi), -64, 64, 451)
    ref, _ = resize_ref64_ac(nhwc(x), Ho, Wo)
    bound = resize_bound_ac(nhwc(x), Ho, Wo, Hi, Wi, False, True, ref)
    xg, yg = _image_resize(x, Ho, Wo)
    torch.cuda.synchronize()
    _bounded("image_resize 13x17 -> 40x27", yg.view[..., :3], ref, bound)
    assert_bits_equal("image_resize padding", yg.view[..., 3:].cpu(), torch.zeros((AC.B, Ho, Wo, 13), dtype=ACT_DTYPE))
    assert_guard_intact("image_resize bounded", xg, yg)


# ---- the interface
def test_exact_ac_argument_checks():
    """align_corners outside {0, 1} is SSA_EINVAL on all five entry points, and so is everything their elders refuse;
    nothing is written."""
    hb, L, _ = _rs()
    x = guarded_copy(ints((AC.B, 5, 7, 8), -9, 9, 1).to(ACT_DTYPE), DEV)
    y = guarded((AC.B, 9, 13, 8), ACT_DTYPE, DEV)
    t = guarded((AC.B, 9, 7, 8), torch.float32, DEV)
    img = guarded_copy(ints((AC.B, 3, 5, 7), -9, 9, 2), DEV)
    yi = guarded((AC.B, 9, 13, 16), ACT_DTYPE, DEV)
    p, s = hb._p, hb._s()
    for ac in (2, -1, 256):
        assert L.ssa_resize_bilinear_fwd(p(x.view), 0, AC.B, 5, 7, 8, 8, p(y.view), 0, 9, 13, 8, ac, s) == _EINVAL
        assert L.ssa_resize_bilinear_bwd(p(y.view), 0, AC.B, 9, 13, 8, 8, p(x.view), 0, 5, 7, 8, ac, s) == _EINVAL
        assert L.ssa_resize_bilinear_bwd_x(p(y.view), 0, AC.B, 9, 13, 8, 8, p(t.view), 7, ac, s) == _EINVAL
        assert L.ssa_resize_bilinear_bwd_y(p(t.view), AC.B, 9, 7, 8, p(x.view), 0, 5, 8, ac, s) == _EINVAL
        assert L.ssa_image_resize_to_nhwc(p(img.view), AC.B, 3, 5, 7, p(yi.view), 9, 13, 16, ac, s) == _EINVAL
    for ac in (0, 1):
        assert L.ssa_resize_bilinear_fwd(None, 0, AC.B, 5, 7, 8, 8, p(y.view), 0, 9, 13, 8, ac, s) == _EINVAL
        assert L.ssa_resize_bilinear_fwd(p(x.view), 0, AC.B, 0, 7, 8, 8, p(y.view), 0, 9, 13, 8, ac, s) == _EINVAL
        assert L.ssa_resize_bilinear_fwd(p(x.view), 0, AC.B, 5, 7, 8, 8, p(y.view), 0, 9, 0, 8, ac, s) == _EINVAL
        assert L.ssa_resize_bilinear_fwd(p(x.view), 2, AC.B, 5, 7, 8, 8, p(y.view), 0, 9, 13, 8, ac, s) == _EINVAL      # no such dtype
        assert L.ssa_resize_bilinear_bwd(p(y.view), 0, AC.B, 9, 13, 8, 8, None, 0, 5, 7, 8, ac, s) == _EINVAL
        assert L.ssa_resize_bilinear_bwd(p(y.view), 0, AC.B, 9, 13, 8, 8, p(t.view), 1, 5, 7, 8, ac, s) == _EINVAL      # 16-bit -> fp32
        assert L.ssa_resize_bilinear_bwd_x(p(y.view), 0, AC.B, 9, 13, 0, 8, p(t.view), 7, ac, s) == _EINVAL
        assert L.ssa_resize_bilinear_bwd_x(p(y.view), 0, AC.B, 9, 13, 8, 8, t.view.data_ptr() + 4, 7, ac, s) == _EINVAL  # tmp not aligned
        assert L.ssa_resize_bilinear_bwd_y(None, AC.B, 9, 7, 8, p(x.view), 0, 5, 8, ac, s) == _EINVAL
        assert L.ssa_image_resize_to_nhwc(p(img.view), AC.B, 3, 5, 7, p(yi.view), 9, 13, 12, ac, s) == _EINVAL          # cpad % 8
        assert L.ssa_image_resize_to_nhwc(p(img.view), AC.B, 3, 5, 7, p(yi.view), 9, 13, 0, ac, s) == _EINVAL           # cpad < C
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.view.float()).all()) and bool(torch.isnan(t.view).all()) and bool(torch.isnan(yi.view.float()).all())
    assert_guard_intact("argument checks", x, y, t, img, yi)


def test_exact_ac_flag_off_is_the_old_entry_point():
    """The old entry points and the new ones with align_corners=0 give identical bytes (a non-dyadic 4x problem on the
    8-channel, the tiled and the separable routes, and the image resize)."""
    hb, L, check = _rs()
    p, s = hb._p, hb._s()
    Bn, Hi, Wi, Ho, Wo = AC.B, 8, 12, 32, 47
    for C, is16 in ((48, True), (19, False)):
        g = torch.Generator().manual_seed(470 + C)
        x = torch.randn(Bn, Hi, Wi, C, generator=g).to(_dt(is16))
        dy = torch.randn(Bn, Ho, Wo, C, generator=g).to(_dt(is16))
        code = 0 if is16 else 1
        xg, yg = _fwd(x, is16, is16, Ho, Wo, ac=0)
        dyg, dxg = _bwd(dy, is16, is16, Hi, Wi, ac=0)
        _, tg, sxg = _bwd_sep(dy, is16, is16, Hi, Wi, ac=0)
        y0, dx0, sx0 = guarded((Bn, Ho, Wo, C), _dt(is16), DEV), guarded((Bn, Hi, Wi, C), _dt(is16), DEV), guarded((Bn, Hi, Wi, C), _dt(is16), DEV)
        t0 = guarded((Bn, Ho, Wi, C), torch.float32, DEV)
        check(L.ssa_bilinear_fwd(p(xg.view), code, Bn, Hi, Wi, C, C, p(y0.view), code, Ho, Wo, C, s), "ssa_bilinear_fwd")
        check(L.ssa_bilinear_bwd(p(dyg.view), code, Bn, Ho, Wo, C, C, p(dx0.view), code, Hi, Wi, C, s), "ssa_bilinear_bwd")
        check(L.ssa_bilinear_bwd_x(p(dyg.view), code, Bn, Ho, Wo, C, C, p(t0.view), Wi, s), "ssa_bilinear_bwd_x")
        check(L.ssa_bilinear_bwd_y(p(t0.view), Bn, Ho, Wi, C, p(sx0.view), code, Hi, C, s), "ssa_bilinear_bwd_y")
        torch.cuda.synchronize()
        for tag, a, b in (("fwd", yg, y0), ("bwd", dxg, dx0), ("bwd_x", tg, t0), ("bwd_y", sxg, sx0)):
            assert_bits_equal("align_corners=0 %s C=%d" % (tag, C), a.view.cpu(), b.view.cpu())
        # ... and align_corners=1 is another result
        _, y1 = _fwd(x, is16, is16, Ho, Wo, ac=1)
        torch.cuda.synchronize()
        assert not torch.equal(y1.view.cpu(), y0.view.cpu())
    img = torch.randn(Bn, 3, Hi, Wi, generator=torch.Generator().manual_seed(471))
    xg, yg = _image_resize(img, Ho, Wo, ac=0)
    y0 = guarded((Bn, Ho, Wo, 16), ACT_DTYPE, DEV)
    check(L.ssa_image_resize_to_nhwc_bf16(p(xg.view), Bn, 3, Hi, Wi, p(y0.view), Ho, Wo, 16, s), "ssa_image_resize_to_nhwc_bf16")
    torch.cuda.synchronize()
    assert_bits_equal("align_corners=0 image", yg.view.cpu(), y0.view.cpu())
