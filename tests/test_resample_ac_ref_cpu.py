"""The float64 align_corners=True resampling reference (tests/resample_ac_ref.py) anchored to the public
F.interpolate(mode="bilinear", align_corners=True), float32, on the CPU -- bit for bit on the exact family, forward and
autograd backward, within resize_bound_ac on the bounded family -- and the properties the exact / bounded GPU tests of the
ssa_resize_* entry points take from it.  It differs from the align_corners=False reference on every case that is not a
copy: a kernel left on the other rule cannot pass."""
import pytest
import torch
import torch.nn.functional as F

import resample_ac_cases as AC
from exact_util import ints, not_representable
from resample_ac_ref import (exact_grad_x_ac, exact_resize_ac, exact_resize_grad_ac, frac_bits_ac, is_dyadic_ac, resize_bound_ac,
                             resize_grad_ref64_ac, resize_ref64_ac, taps_ac, window_ac)
from resample_ref import resize_grad_ref64, resize_ref64, taps
from util import ACT_DTYPE, nchw, nhwc


def _interp(x, dy, Ho, Wo, **how):
    """F.interpolate(align_corners=True) and its autograd on NHWC float32 tensors."""
    xr = nchw(x).requires_grad_(True)
    y = F.interpolate(xr, mode="bilinear", align_corners=True, **(how or {"size": (Ho, Wo)}))
    assert tuple(y.shape[2:]) == (Ho, Wo)
    y.backward(nchw(dy))
    return nhwc(y.detach()), nhwc(xr.grad)


# the shapes the issue of this feature lists, and every shape of the exact tables
_LISTED = [(5, 7, 9, 13), (3, 5, 9, 17), (5, 3, 17, 9), (9, 13, 5, 7), (6, 10, 6, 10), (3, 2, 17, 9), (1, 1, 4, 6), (5, 7, 1, 1),
           (2, 2, 9, 5), (9, 21, 17, 41), (9, 21, 33, 81)]
_EXACT_SHAPES = sorted({(3,) + s for s in _LISTED} | {c[1:6] for c in AC.FWD_EXACT + AC.BWD_EXACT + AC.SEP_EXACT})


@pytest.mark.parametrize("C,Hi,Wi,Ho,Wo", _EXACT_SHAPES)
def test_reference_equals_interpolate_bit_for_bit(C, Hi, Wi, Ho, Wo):
    case = ("", C, Hi, Wi, Ho, Wo)
    x, dy = AC.fwd_operand(case), AC.bwd_operand(case)
    y, dx = _interp(x, dy, Ho, Wo)
    ref = exact_resize_ac("fwd", x, Ho, Wo)
    gref = exact_resize_grad_ac("bwd", dy, Hi, Wi)
    assert torch.equal(y.double(), ref)
    assert torch.equal(dx.double(), gref)
    # pass X then pass Y of the separable form is the same product
    tmp = exact_grad_x_ac("bwd x", dy, Wi)
    assert torch.equal(torch.einsum("oh,bowc->bhwc", taps_ac(Ho, Hi), tmp), gref)


@pytest.mark.parametrize("case", AC.BOUNDED, ids=[c[0] for c in AC.BOUNDED])
def test_reference_within_bound_of_interpolate(case):
    _, C, Hi, Wi, Ho, Wo, _ = case
    x, dy = AC.bounded_operands(case)
    y, dx = _interp(x, dy, Ho, Wo)
    ref, _ = resize_ref64_ac(x, Ho, Wo)
    gref, _ = resize_grad_ref64_ac(dy, Hi, Wi)
    bf = resize_bound_ac(x, Ho, Wo, Hi, Wi, False, False)
    bb = resize_bound_ac(dy, Ho, Wo, Hi, Wi, True, False)
    assert bool(((y.double() - ref).abs() <= bf).all())
    assert bool(((dx.double() - gref).abs() <= bb).all())


@pytest.mark.parametrize("factor", [1.5, 2.0])
def test_scale_factor_is_size(factor):
    """The scale depends on the sizes only: scale_factor=, with or without recompute_scale_factor, is size=."""
    Hi, Wi = 9, 13
    Ho, Wo = int(Hi * factor), int(Wi * factor)
    x, dy = ints((2, Hi, Wi, 3), -200, 200, 5), ints((2, Ho, Wo, 3), -50, 50, 6)
    want = _interp(x, dy, Ho, Wo)
    for how in ({"scale_factor": factor}, {"scale_factor": factor, "recompute_scale_factor": True}):
        got = _interp(x, dy, Ho, Wo, **how)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    ref, _ = resize_ref64_ac(x, Ho, Wo)
    assert bool(((want[0].double() - ref).abs() <= resize_bound_ac(x, Ho, Wo, Hi, Wi, False, False)).all())


def _is_copy(n_out, n_in):
    return n_out == n_in


@pytest.mark.parametrize("case", AC.FWD_EXACT + AC.BWD_EXACT + AC.SEP_EXACT + [c + (None,) for c in AC.BOUNDED],
                         ids=lambda c: "%s-%dx%d-%dx%d" % (c[0], c[2], c[3], c[4], c[5]))
def test_differs_from_the_other_rule(case):
    """Every case that is not a copy has other weights, another forward and another backward than align_corners=False --
    from one pixel the two rules agree (a broadcast), on that axis only."""
    _, C, Hi, Wi, Ho, Wo = case[:6]
    same_y = _is_copy(Ho, Hi) or Hi == 1
    same_x = _is_copy(Wo, Wi) or Wi == 1
    assert torch.equal(taps_ac(Ho, Hi), taps(Ho, Hi)) == same_y
    assert torch.equal(taps_ac(Wo, Wi), taps(Wo, Wi)) == same_x
    x, dy = AC.bounded_operands(case)
    assert torch.equal(resize_ref64_ac(x, Ho, Wo)[0], resize_ref64(x, Ho, Wo)[0]) == (same_y and same_x)
    assert torch.equal(resize_grad_ref64_ac(dy, Hi, Wi)[0], resize_grad_ref64(dy, Hi, Wi)[0]) == (same_y and same_x)


@pytest.mark.parametrize("n_out,n_in", AC.DYADIC + [(c[4], c[2]) for c in AC.BOUNDED] + [(c[5], c[3]) for c in AC.BOUNDED])
def test_taps_properties(n_out, n_in):
    m = taps_ac(n_out, n_in)
    assert m.shape == (n_out, n_in) and m.dtype == torch.float64
    assert bool((m >= 0).all()) and bool((m <= 1).all())
    assert int((m > 0).sum(1).max()) <= 2
    assert float((m.sum(1) - 1).abs().max()) <= 2.0 ** -23
    nz = (m > 0).nonzero()
    for o in range(n_out):                                  # the two taps of a row are neighbours
        cols = nz[nz[:, 0] == o][:, 1]
        assert int(cols.max() - cols.min()) <= 1
    assert float(m[0, 0]) == 1.0                            # the corners are aligned
    if n_out > 1 and n_in > 1:
        assert float(m[n_out - 1, n_in - 1]) > 1 - 2.0 ** -10
    if n_out > 1 and n_in > 1:                              # the window the host sizes for: ceil(2 / scale) + 1 covers it
        import math
        assert window_ac(n_out, n_in) <= math.ceil(2.0 * (n_out - 1) / (n_in - 1)) + 1


def test_taps_degenerate_sizes():
    """scale == 0: one input pixel is a broadcast, one output pixel reads input 0 (NOT the centre, as the other rule does)."""
    assert torch.equal(taps_ac(5, 1), torch.ones(5, 1, dtype=torch.float64))
    assert torch.equal(taps_ac(1, 1), torch.ones(1, 1, dtype=torch.float64))
    assert torch.equal(taps_ac(1, 2), torch.tensor([[1.0, 0]], dtype=torch.float64))
    assert torch.equal(taps_ac(1, 5), torch.tensor([[1.0, 0, 0, 0, 0]], dtype=torch.float64))
    assert torch.equal(taps_ac(2, 2), torch.eye(2, dtype=torch.float64))
    assert torch.equal(taps_ac(3, 2), torch.tensor([[1, 0], [0.5, 0.5], [0, 1.0]], dtype=torch.float64))
    assert torch.equal(taps_ac(3, 3), torch.eye(3, dtype=torch.float64))
    assert torch.equal(taps_ac(3, 5), torch.eye(5, dtype=torch.float64)[::2])
    x = ints((2, 1, 1, 3), -9, 9, 1)
    assert torch.equal(resize_ref64_ac(x, 5, 7)[0], x.double().expand(2, 5, 7, 3))
    g = ints((2, 5, 7, 3), -9, 9, 2)
    assert torch.equal(resize_grad_ref64_ac(g, 1, 1)[0], g.double().sum((1, 2), keepdim=True))
    # to one pixel: the output is input (0, 0); in the backward input (0, 0) receives everything, the others zero
    x = ints((2, 5, 7, 3), -9, 9, 3)
    assert torch.equal(resize_ref64_ac(x, 1, 1)[0], x.double()[:, :1, :1])
    g1 = ints((2, 1, 1, 3), -9, 9, 4)
    want = torch.zeros(2, 5, 7, 3, dtype=torch.float64)
    want[:, 0, 0] = g1.double()[:, 0, 0]
    assert torch.equal(resize_grad_ref64_ac(g1, 5, 7)[0], want)


def test_dyadic_family():
    for n_out, n_in in AC.DYADIC:
        assert is_dyadic_ac(n_out, n_in), (n_out, n_in)
    for n_out, n_in in ((10, 5), (20, 5), (256, 64), (1024, 128), (32, 8), (8, 16), (7, 5)):    # the network's own ratios are not
        assert not is_dyadic_ac(n_out, n_in), (n_out, n_in)
    ratios = {(o - 1) / (i - 1) for o, i in AC.DYADIC if o > 1 and i > 1}
    assert ratios == {0.5, 1.0, 2.0, 4.0, 8.0}, ratios


def test_fraction_bits_and_windows_of_the_dyadic_family():
    """Per axis: 0 bits at 1x, 0.5x and scale 0; 1 / 2 / 3 at 2x / 4x / 8x.  Windows: 1, 1, the axis; 3 / 7 / 15."""
    bits = {0.5: 0, 1.0: 0, 2.0: 1, 4.0: 2, 8.0: 3}
    wins = {0.5: 1, 1.0: 1, 2.0: 3, 4.0: 7, 8.0: 15}
    for n_out, n_in in AC.DYADIC:
        if n_out == 1 or n_in == 1:
            assert frac_bits_ac(n_out, n_in) == 0 and window_ac(n_out, n_in) == n_out
        else:
            r = (n_out - 1) / (n_in - 1)
            assert frac_bits_ac(n_out, n_in) == bits[r] and window_ac(n_out, n_in) == wins[r], (n_out, n_in)
    assert (window_ac(256, 64), window_ac(1024, 128), window_ac(33, 5)) == (9, 17, 15)
    with pytest.raises(AssertionError):
        frac_bits_ac(21, 8)


@pytest.mark.skipif(ACT_DTYPE != torch.bfloat16, reason="fp16 holds every half and quarter of integers up to 200")
def test_exact_cases_need_rounding():
    """Every exact case with a 16-bit output and fractional weights has outputs bf16 cannot hold: the rounding mode decides
    bits.  Without fractional weights (1x, 0.5x, scale 0 in the forward) the outputs are inputs."""
    for case in AC.FWD_EXACT:
        if case[7]:
            frac = frac_bits_ac(case[4], case[2]) + frac_bits_ac(case[5], case[3]) > 0
            n = not_representable(exact_resize_ac(case[0], AC.fwd_operand(case), case[4], case[5]))
            assert (n > 0) == frac, (case[0], n)
    for case in AC.BWD_EXACT + AC.SEP_EXACT:           # (a scale-0 axis caps the gradient's magnitude: small sums, nothing to round)
        if case[7] and 1 not in case[2:6] and frac_bits_ac(case[4], case[2]) + frac_bits_ac(case[5], case[3]) > 0:
            assert not_representable(exact_resize_grad_ac(case[0], AC.bwd_operand(case), case[2], case[3])) > 0, case[0]


def test_case_tables_mirror_the_other_rule():
    """Unique ids; every route id of resample_cases has its counterpart here (TAPS 4 / 8 become 8 / 12 under this rule)."""
    import resample_cases as RC
    for table in (AC.FWD_EXACT, AC.BWD_EXACT, AC.SEP_EXACT, AC.BOUNDED):
        ids = [c[0] for c in table]
        assert len(ids) == len(set(ids))
    ren = {"tile-t4": "tile-t8", "tile-t4-ld": "tile-t8-ld", "tile-t4-out16": "tile-t8-out16", "tile-t8": "tile-t12",
           "tile-t8-ld-out16": "tile-t12-ld-out16", "tile-t8-c8-4x2": "tile-t12-c8-4x2", "tile-t8-2x4": "tile-t12-2x4"}
    for mine, theirs in ((AC.FWD_EXACT, RC.FWD_EXACT), (AC.BWD_EXACT, RC.BWD_EXACT), (AC.SEP_EXACT, RC.SEP_EXACT),
                         (AC.BOUNDED, RC.BOUNDED)):
        have = {c[0]: c for c in mine}
        for c in theirs:
            m = have[ren.get(c[0], c[0])]
            assert m[1] == c[1] and m[6:] == c[6:], (c[0], m)            # same channels, dtypes and leading dimensions
    assert all(c[0] != "" and AC.B == 2 for c in AC.FWD_EXACT)
