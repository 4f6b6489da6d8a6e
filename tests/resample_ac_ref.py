"""float64 reference of the bilinear resize under align_corners=True on NHWC tensors, for the exact and the bounded tests
of the ssa_resize_* entry points of csrc/resample.hip (a plain module, not a conftest).  The align_corners=False reference
is tests/resample_ref.py; this module has the same structure with the other weight matrices.

THE RULE (ATen's upsample_bilinear2d with align_corners=True; every step ONE fp32 operation):
    scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f
    s  = scale * (float)o
    i0 = min((int)s, n_in - 1);  i1 = i0 + (i0 < n_in - 1)
    l1 = s - (float)i0;          l0 = 1.f - l1
`taps_ac` restates it with numpy float32 for the index steps and float64 for the matrix.  The index steps must be fp32: a
float64 index moves results by up to 3e-2 at (3, 4093) -> (3, 1500).

EXACT.  When (n_in - 1) / (n_out - 1) is a power of two -- sizes of the form k 2^m + 1 -- every weight is dyadic (a multiple
of 2^-3 at 8x, asserted on the matrix: is_dyadic_ac), so with integer operands every product weight_y * weight_x * value is
a multiple of 2^-(k_y + k_x), and when the same sum over the ABSOLUTE values (`mag`) times 2^(k_y + k_x) stays below 2^24
every partial sum, in any order, x first or y first, with or without FMA contraction, is exact in fp32.  The only
rounding left is the one to the 16-bit storage format.  The premise is asserted on the reference (exact_resize_ac /
exact_resize_grad_ac / exact_grad_x_ac), never on the kernel.

BOUNDED (resize_bound_ac), for ratios that are not dyadic; per element, two terms:
  arithmetic   (T + 4) 2^-24 A.  A = sum of weight |value| at the element, T = its taps with a non-zero weight (4 in the
               forward, window_y * window_x of THESE matrices in the backward).  As in resample_ref: a term weight_y *
               weight_x * value carries at most four roundings before it is added (l0 = 1 - l1 per axis -- l1 = s - i0 is
               exact: i0 = floor(s) --, the product of the two weights, the product with the value), a sum
               of T terms in any order adds at most T - 1.
  storage      a 16-bit output adds half a unit of the storage format at |ref| + the arithmetic term.
There is NO source-index term: s is a single fp32 product of two values the rule fixes (scale is one fp32 division of two
exactly converted integers, o converts exactly), so there is nothing a compiler could contract and the device computes
the very s of taps_ac.  (Under align_corners=False, s = scale * (o + 0.5) - 0.5 may become one FMA: resample_ref's d term.)
"""
import numpy as np
import torch

from exact_util import assert_integers, assert_premise
from resample_ref import half_ulp_act


def scale_ac(n_out, n_in):
    f = np.float32
    return f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)


def taps_ac(n_out, n_in):
    """[n_out, n_in] float64 bilinear weights under align_corners=True, built like resample_ref.taps."""
    f = np.float32
    scale = scale_ac(n_out, n_in)
    s = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (s - i0.astype(np.float32)).astype(np.float32)
    l0 = (f(1) - l1).astype(np.float32)
    m = np.zeros((n_out, n_in), np.float64)
    r = np.arange(n_out)
    np.add.at(m, (r, i0), l0.astype(np.float64))
    np.add.at(m, (r, i1), l1.astype(np.float64))
    return torch.from_numpy(m)


def is_dyadic_ac(n_out, n_in):
    """Every weight of taps_ac(n_out, n_in) is a multiple of 2^-8 -- read off the matrix."""
    m = taps_ac(n_out, n_in) * 256.0
    return bool(torch.equal(m, m.round()))


def frac_bits_ac(n_out, n_in):
    """The smallest k with every weight a multiple of 2^-k (asserted dyadic): 0 at 1x, 0.5x and scale 0, 1 / 2 / 3 at 2x / 4x / 8x."""
    assert is_dyadic_ac(n_out, n_in), "%d <- %d is not dyadic under align_corners=True" % (n_out, n_in)
    m = taps_ac(n_out, n_in)
    return next(k for k in range(9) if torch.equal(m * 2.0 ** k, (m * 2.0 ** k).round()))


def window_ac(n_out, n_in):
    """The widest window of the backward: most outputs any input pixel receives from (read off the matrix)."""
    return int((taps_ac(n_out, n_in) > 0).sum(0).max())


def _mats(Ho, Hi, Wo, Wi):
    return taps_ac(Ho, Hi), taps_ac(Wo, Wi)


def _pz(t):
    """Zeros of a matrix product as +0.0.  A pixel no output reads (every input but the first at scale 0) is a sum of
    0 * value terms only, which float64 may give as -0.0; an fp32 accumulator that starts at +0.0 -- the kernels', and
    ATen's zero-initialised gradient -- never ends at -0.0 (+0 + -0 = +0, and an exact cancellation rounds to +0), nor
    does the forward's l0 * a + l1 * b with l0 + l1 = 1 on operands without negative zeros."""
    return t + 0.0


def resize_ref64_ac(x, Ho, Wo):
    """x [B, Hi, Wi, C] -> (My x Mx^T, the same product of |x|), float64 [B, Ho, Wo, C]."""
    x = x.detach().double().cpu()
    my, mx = _mats(Ho, x.shape[1], Wo, x.shape[2])
    return _pz(torch.einsum("oh,bhwc,pw->bopc", my, x, mx)), torch.einsum("oh,bhwc,pw->bopc", my, x.abs(), mx)


def resize_grad_ref64_ac(dy, Hi, Wi):
    """dy [B, Ho, Wo, C] -> (My^T dy Mx, the same product of |dy|), float64 [B, Hi, Wi, C]."""
    dy = dy.detach().double().cpu()
    my, mx = _mats(dy.shape[1], Hi, dy.shape[2], Wi)
    return _pz(torch.einsum("oh,bopc,pw->bhwc", my, dy, mx)), torch.einsum("oh,bopc,pw->bhwc", my, dy.abs(), mx)


def grad_x_ref64_ac(dy, Wi):
    """Pass X of the separable backward alone: tmp[b, oy, ix, c] = sum_ox wx dy, and the same of |dy|."""
    dy = dy.detach().double().cpu()
    mx = taps_ac(dy.shape[2], Wi)
    return _pz(torch.einsum("bopc,pw->bowc", dy, mx)), torch.einsum("bopc,pw->bowc", dy.abs(), mx)


def grad_amp_ac(Ho, Hi, Wo, Wi, cap=64):
    """Largest |dy| <= cap at which the backward's magnitude product stays below 2^8 (from the matrices)."""
    my, mx = _mats(Ho, Hi, Wo, Wi)
    return max(1, min(cap, int(255.0 / (float(my.sum(0).max()) * float(mx.sum(0).max())))))


def _premise(name, v, Ho, Hi, Wo, Wi, ref, mag):
    assert_integers(name, v)
    assert_premise(name, mag * 2.0 ** (frac_bits_ac(Ho, Hi) + frac_bits_ac(Wo, Wi)))
    assert torch.equal(ref.float().double(), ref), "%s: the reference is not exact in fp32" % name


def exact_resize_ac(name, x, Ho, Wo):
    """The float64 forward with the exactness premise asserted on it."""
    ref, mag = resize_ref64_ac(x, Ho, Wo)
    _premise(name, x, Ho, x.shape[1], Wo, x.shape[2], ref, mag)
    return ref


def exact_resize_grad_ac(name, dy, Hi, Wi):
    ref, mag = resize_grad_ref64_ac(dy, Hi, Wi)
    _premise(name, dy, dy.shape[1], Hi, dy.shape[2], Wi, ref, mag)
    return ref


def exact_grad_x_ac(name, dy, Wi):
    ref, mag = grad_x_ref64_ac(dy, Wi)
    _premise(name, dy, 1, 1, dy.shape[2], Wi, ref, mag)
    return ref


def resize_bound_ac(v, Ho, Wo, Hi, Wi, backward, out16, ref=None):
    """Per-element bound (see the module docstring) of the forward of v = x [B, Hi, Wi, C] or of the backward of
    v = dy [B, Ho, Wo, C]: the arithmetic term, and the storage term for a 16-bit output."""
    v = v.detach().double().cpu().abs()
    my, mx = _mats(Ho, Hi, Wo, Wi)
    if backward:
        a = torch.einsum("oh,bopc,pw->bhwc", my, v, mx)
        t = ((my > 0).sum(0).double()[:, None] * (mx > 0).sum(0).double()[None, :])[None, :, :, None]
    else:
        a = torch.einsum("oh,bhwc,pw->bopc", my, v, mx)
        t = 4.0
    bound = (t + 4.0) * 2.0 ** -24 * a
    if out16:
        bound = bound + half_ulp_act(ref.abs() + bound)
    return bound
