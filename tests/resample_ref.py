"""float64 reference of the bilinear resize (align_corners=False) on NHWC tensors, for the exact and the bounded tests of
csrc/resample.hip (a plain module, not a conftest).

EXACT.  With power-of-two resize ratios every weight is a multiple of 2^-8 (is_dyadic asserts it on the matrix), so with
integer operands every product weight_y * weight_x * value is a multiple of 2^-16.  When the same sum over the ABSOLUTE
values (`mag`) stays below 2^8, every partial sum -- in any order, x first or y first, with or without FMA contraction
-- is a multiple of 2^-16 below 2^8: 24 bits, exact in fp32.  The only rounding left is the one to the 16-bit storage
format.  The premise is asserted on the reference (exact_resize / exact_resize_grad), never on the kernel.  It is
asserted with the bits the matrices really use (frac_bits: 1 per axis at 0.5x, 2 at 2x, 3 at 4x, 4 at 8x, never more than
8): mag * 2^(k_y + k_x) < 2^24.  At 0.5x that leaves room for operands of eleven bits, which the fp16 build needs for
an average of four values to fall between two of its numbers.

BOUNDED (resize_bound), for ratios that are not dyadic; per element, three terms:
  arithmetic   (T + 4) 2^-24 A.  A = sum of weight |value| at the element, T = its taps with a non-zero weight (4 in
               the forward, window_y * window_x in the backward).  A term weight_y * weight_x * value carries at most
               four roundings before it is added (l0 = 1 - l1 per axis -- l1 = s - i0 is exact --, the product of the two
               weights, the product with the value; the forward's nested form has no more), and a sum of T terms in any
               order adds at most T - 1: (1 + 2^-24)^(T+3) - 1 < (T + 4) 2^-24.  The separable forms round fewer times.
  source index (d_y + d_x) A', d = 2^(ceil(log2 n_in) - 23) per axis.  `taps` rounds scale * (o + 0.5) - 0.5 twice; a
               compiler may contract it into one FMA.  Both results lie within one unit in the last place of s < n_in <=
               2^ceil(log2 n_in), i.e. within 2^(ceil(log2 n_in) - 24), of each other; d allows two.  A bilinear weight is
               a hat function of s, continuous with slope 1 also where the tap moves to the neighbouring source pixel, so
               every weight moves by at most d and only on the reference's taps widened by one source pixel per side.
               With w'w' - ww = (w_y' - w_y) w_x' + w_y (w_x' - w_x) and weights <= 1 the result moves by at most
               (d_y + d_x) A', A' = the UNWEIGHTED sum of |value| over the widened taps.
  storage      a 16-bit output adds half a unit of the storage format at |ref| + the two terms above.
"""
import math

import numpy as np
import torch

from exact_util import assert_integers, assert_premise, to_act, to_f32  # noqa: F401  (re-exported for the tests)
from util import ACT_DTYPE

_MANT = 10 if ACT_DTYPE == torch.float16 else 7          # explicit mantissa bits of the storage format
_EMIN = -14 if ACT_DTYPE == torch.float16 else -126


def taps(n_out, n_in, fma=False):
    """[n_out, n_in] float64 bilinear weights, from the fp32 steps of src_index (csrc/resample.hip) and ATen's
    upsample_bilinear2d, each rounded to fp32 on its own.  fma: scale * (o + 0.5) - 0.5 rounded ONCE, what a contracted
    multiply-add gives (the 48-bit product is exact in float64) -- for the printed diagnosis of the bounded tests only."""
    f = np.float32
    scale = f(n_in) / f(n_out)
    if fma:
        s = (np.float64(scale) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5).astype(np.float32)
    else:
        s = scale * (np.arange(n_out, dtype=np.float32) + f(0.5))
        s = s - f(0.5)
    s = np.where(s < 0, f(0), s).astype(np.float32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (s - i0.astype(np.float32)).astype(np.float32)
    l0 = (f(1) - l1).astype(np.float32)
    m = np.zeros((n_out, n_in), np.float64)
    r = np.arange(n_out)
    np.add.at(m, (r, i0), l0.astype(np.float64))
    np.add.at(m, (r, i1), l1.astype(np.float64))
    return torch.from_numpy(m)


def is_dyadic(n_out, n_in):
    """Every weight of taps(n_out, n_in) is a multiple of 2^-8 -- read off the matrix."""
    m = taps(n_out, n_in) * 256.0
    return bool(torch.equal(m, m.round()))


def frac_bits(n_out, n_in):
    """The smallest k with every weight of taps(n_out, n_in) a multiple of 2^-k (asserted dyadic: k <= 8)."""
    assert is_dyadic(n_out, n_in), "%d <- %d is not dyadic" % (n_out, n_in)
    m = taps(n_out, n_in)
    return next(k for k in range(9) if torch.equal(m * 2.0 ** k, (m * 2.0 ** k).round()))


def _wide(m):
    """0/1 matrix of the taps of m widened by one source pixel on each side."""
    nz = (m > 0).double()
    w = nz.clone()
    w[:, 1:] += nz[:, :-1]
    w[:, :-1] += nz[:, 1:]
    return (w > 0).double()


def _mats(Ho, Hi, Wo, Wi, fma=(False, False)):
    return taps(Ho, Hi, fma[0]), taps(Wo, Wi, fma[1])


def resize_ref64(x, Ho, Wo, fma=(False, False)):
    """x [B, Hi, Wi, C] -> (My x Mx^T, the same product of |x|), float64 [B, Ho, Wo, C]."""
    x = x.detach().double().cpu()
    my, mx = _mats(Ho, x.shape[1], Wo, x.shape[2], fma)
    return torch.einsum("oh,bhwc,pw->bopc", my, x, mx), torch.einsum("oh,bhwc,pw->bopc", my, x.abs(), mx)


def resize_grad_ref64(dy, Hi, Wi, fma=(False, False)):
    """dy [B, Ho, Wo, C] -> (My^T dy Mx, the same product of |dy|), float64 [B, Hi, Wi, C]."""
    dy = dy.detach().double().cpu()
    my, mx = _mats(dy.shape[1], Hi, dy.shape[2], Wi, fma)
    return torch.einsum("oh,bopc,pw->bhwc", my, dy, mx), torch.einsum("oh,bopc,pw->bhwc", my, dy.abs(), mx)


def grad_x_ref64(dy, Wi):
    """Pass X of the separable backward alone: tmp[b, oy, ix, c] = sum_ox wx dy, and the same of |dy|."""
    dy = dy.detach().double().cpu()
    mx = taps(dy.shape[2], Wi)
    return torch.einsum("bopc,pw->bowc", dy, mx), torch.einsum("bopc,pw->bowc", dy.abs(), mx)


def grad_amp(Ho, Hi, Wo, Wi, cap=64):
    """Largest |dy| <= cap at which the backward's magnitude product stays below 2^8 (from the matrices)."""
    my, mx = _mats(Ho, Hi, Wo, Wi)
    return max(1, min(cap, int(255.0 / (float(my.sum(0).max()) * float(mx.sum(0).max())))))


def _premise(name, v, Ho, Hi, Wo, Wi, ref, mag):
    assert_integers(name, v)
    assert_premise(name, mag * 2.0 ** (frac_bits(Ho, Hi) + frac_bits(Wo, Wi)))
    assert torch.equal(ref.float().double(), ref), "%s: the reference is not exact in fp32" % name


def exact_resize(name, x, Ho, Wo):
    """The float64 forward with the exactness premise asserted on it."""
    ref, mag = resize_ref64(x, Ho, Wo)
    _premise(name, x, Ho, x.shape[1], Wo, x.shape[2], ref, mag)
    return ref


def exact_resize_grad(name, dy, Hi, Wi):
    ref, mag = resize_grad_ref64(dy, Hi, Wi)
    _premise(name, dy, dy.shape[1], Hi, dy.shape[2], Wi, ref, mag)
    return ref


def exact_grad_x(name, dy, Wi):
    ref, mag = grad_x_ref64(dy, Wi)
    _premise(name, dy, 1, 1, dy.shape[2], Wi, ref, mag)
    return ref


def half_ulp_act(v):
    """Half a unit in the last place of the 16-bit storage format at |v| (float64 tensor)."""
    tiny = torch.tensor(2.0 ** _EMIN, dtype=torch.float64)
    a = torch.maximum(v.abs(), tiny)
    e = torch.floor(torch.log2(a))
    e = torch.where(2.0 ** e > a, e - 1, e)
    return 2.0 ** (e - _MANT - 1)


def _delta(n_in):
    return 2.0 ** (math.ceil(math.log2(n_in)) - 23) if n_in > 1 else 2.0 ** -23


def resize_bound(v, Ho, Wo, Hi, Wi, backward, out16, ref=None, fma=(False, False)):
    """Per-element bound (see the module docstring) of the forward of v = x [B, Hi, Wi, C] or of the backward of
    v = dy [B, Ho, Wo, C].  Returns (bound, index term) -- the index term is part of the bound."""
    v = v.detach().double().cpu().abs()
    my, mx = _mats(Ho, Hi, Wo, Wi, fma)
    wy, wx = _wide(my), _wide(mx)
    if backward:
        a = torch.einsum("oh,bopc,pw->bhwc", my, v, mx)
        aw = torch.einsum("oh,bopc,pw->bhwc", wy, v, wx)
        t = ((my > 0).sum(0).double()[:, None] * (mx > 0).sum(0).double()[None, :])[None, :, :, None]
    else:
        a = torch.einsum("oh,bhwc,pw->bopc", my, v, mx)
        aw = torch.einsum("oh,bhwc,pw->bopc", wy, v, wx)
        t = 4.0
    idx = (_delta(Hi) + _delta(Wi)) * aw
    bound = (t + 4.0) * 2.0 ** -24 * a + idx
    if out16:
        bound = bound + half_ulp_act(ref.abs() + bound)
    return bound, idx
