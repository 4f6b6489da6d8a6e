"""The float64 resampling reference (tests/resample_ref.py) anchored to the public F.interpolate, float32, on the CPU --
and the properties the exact / bounded GPU tests take from it."""
import pytest
import torch
import torch.nn.functional as F

import resample_cases as RC
from exact_util import ints, not_representable
from resample_ref import (exact_grad_x, exact_resize, exact_resize_grad, frac_bits, is_dyadic, resize_bound, resize_grad_ref64,
                          resize_ref64, taps)
from util import nchw, nhwc


def _interp(x, dy, Ho, Wo):
    """F.interpolate and its autograd on NHWC float32 tensors."""
    xr = nchw(x).requires_grad_(True)
    y = F.interpolate(xr, size=(Ho, Wo), mode="bilinear", align_corners=False)
    y.backward(nchw(dy))
    return nhwc(y.detach()), nhwc(xr.grad)


_DYADIC_SHAPES = sorted({c[1:6] for c in RC.FWD_EXACT + RC.BWD_EXACT + RC.SEP_EXACT})


@pytest.mark.parametrize("C,Hi,Wi,Ho,Wo", _DYADIC_SHAPES)
def test_reference_equals_interpolate_bit_for_bit(C, Hi, Wi, Ho, Wo):
    case = ("", C, Hi, Wi, Ho, Wo)
    x, dy = RC.fwd_operand(case), RC.bwd_operand(case)
    y, dx = _interp(x, dy, Ho, Wo)
    ref = exact_resize("fwd", x, Ho, Wo)
    gref = exact_resize_grad("bwd", dy, Hi, Wi)
    assert torch.equal(y.double(), ref)
    assert torch.equal(dx.double(), gref)
    # pass X then pass Y of the separable form is the same product
    tmp = exact_grad_x("bwd x", dy, Wi)
    assert torch.equal(torch.einsum("oh,bowc->bhwc", taps(Ho, Hi), tmp), gref)


@pytest.mark.parametrize("case", RC.BOUNDED, ids=[c[0] for c in RC.BOUNDED])
def test_reference_within_bound_of_interpolate(case):
    _, C, Hi, Wi, Ho, Wo, _ = case
    x, dy = RC.bounded_operands(case)
    y, dx = _interp(x, dy, Ho, Wo)
    ref, _ = resize_ref64(x, Ho, Wo)
    gref, _ = resize_grad_ref64(dy, Hi, Wi)
    bf, _ = resize_bound(x, Ho, Wo, Hi, Wi, False, False)
    bb, _ = resize_bound(dy, Ho, Wo, Hi, Wi, True, False)
    assert bool(((y.double() - ref).abs() <= bf).all())
    assert bool(((dx.double() - gref).abs() <= bb).all())


@pytest.mark.parametrize("n_out,n_in", RC.DYADIC + [(c[4], c[2]) for c in RC.BOUNDED] + [(c[5], c[3]) for c in RC.BOUNDED])
def test_taps_properties(n_out, n_in):
    m = taps(n_out, n_in)
    assert m.shape == (n_out, n_in) and m.dtype == torch.float64
    assert bool((m >= 0).all()) and bool((m <= 1).all())
    assert int((m > 0).sum(1).max()) <= 2
    assert float((m.sum(1) - 1).abs().max()) <= 2.0 ** -23
    nz = (m > 0).nonzero()
    for o in range(n_out):                                  # the two taps of a row are neighbours
        cols = nz[nz[:, 0] == o][:, 1]
        assert int(cols.max() - cols.min()) <= 1


def test_taps_degenerate_sizes():
    assert torch.equal(taps(5, 1), torch.ones(5, 1, dtype=torch.float64))                     # n_in = 1: a broadcast
    assert torch.equal(taps(1, 1), torch.ones(1, 1, dtype=torch.float64))
    assert torch.equal(taps(1, 2), torch.tensor([[0.5, 0.5]], dtype=torch.float64))           # n_out = 1: the centre
    assert torch.equal(taps(1, 5), torch.tensor([[0, 0, 1.0, 0, 0]], dtype=torch.float64))
    assert torch.equal(taps(1, 4), torch.tensor([[0, 0.5, 0.5, 0]], dtype=torch.float64))
    assert torch.equal(taps(2, 2), torch.eye(2, dtype=torch.float64))
    assert torch.equal(taps(4, 2), torch.tensor([[1, 0], [0.75, 0.25], [0.25, 0.75], [0, 1.0]], dtype=torch.float64))
    assert torch.equal(taps(3, 3), torch.eye(3, dtype=torch.float64))
    x = ints((2, 1, 1, 3), -9, 9, 1)
    assert torch.equal(resize_ref64(x, 5, 7)[0], x.double().expand(2, 5, 7, 3))
    assert torch.equal(resize_grad_ref64(ints((2, 5, 7, 3), -9, 9, 2), 1, 1)[0],
                       ints((2, 5, 7, 3), -9, 9, 2).double().sum((1, 2), keepdim=True))


def test_dyadic_family():
    for n_out, n_in in RC.DYADIC:
        assert is_dyadic(n_out, n_in), (n_out, n_in)
    for f in (2, 4, 8):                                     # 2x, 4x, 8x, 1x, 0.5x of an odd size
        assert is_dyadic(7 * f, 7)
    assert is_dyadic(7, 7) and is_dyadic(7, 14)
    for n_out, n_in in ((21, 8), (31, 12), (20, 4), (18, 3), (7, 5)):                  # integer factors 5 and 6 are not
        assert not is_dyadic(n_out, n_in), (n_out, n_in)
    ratios = {o / i for o, i in RC.DYADIC}
    assert ratios == {0.5, 1.0, 2.0, 4.0, 8.0}, ratios


def test_fraction_bits_of_the_dyadic_family():
    """The bits the premise counts per axis: 0 at 1x and from one pixel, 1 at 0.5x, 2 / 3 / 4 at 2x / 4x / 8x."""
    want = {0.5: 1, 1.0: 0, 2.0: 2, 4.0: 3, 8.0: 4}
    for n_out, n_in in RC.DYADIC:
        assert frac_bits(n_out, n_in) == (0 if n_in == 1 else want[n_out / n_in]), (n_out, n_in)
    with pytest.raises(AssertionError):
        frac_bits(21, 8)


def test_exact_cases_need_rounding():
    """Every exact case whose output is 16-bit has outputs the format cannot hold: the rounding mode decides bits.  The
    exceptions are arithmetic -- the identity resize, and a 1x or 0.5x gradient, where a pixel receives one value times a
    power of two (RC.fwd_rounds / RC.bwd_rounds) -- and are asserted to BE exceptions."""
    for case in RC.FWD_EXACT:
        if case[7]:
            n = not_representable(exact_resize(case[0], RC.fwd_operand(case), case[4], case[5]))
            assert (n > 0) == RC.fwd_rounds(case), (case[0], n)
    for case in RC.BWD_EXACT + RC.SEP_EXACT:
        if case[7]:
            n = not_representable(exact_resize_grad(case[0], RC.bwd_operand(case), case[2], case[3]))
            assert (n > 0) == RC.bwd_rounds(case), (case[0], n)


def test_case_ids_are_unique():
    for table in (RC.FWD_EXACT, RC.BWD_EXACT, RC.SEP_EXACT, RC.BOUNDED):
        ids = [c[0] for c in table]
        assert len(ids) == len(set(ids))
