"""Helpers for the EXACT kernel tests (a plain module, not a conftest).

The argument: with integer-valued operands every product of a convolution is an integer, and as long as the sum of
the ABSOLUTE products stays below 2^24 every partial sum -- in any order, over any tile shape, split or ring depth --
is an integer an fp32 accumulator holds exactly.  The only rounding left is the single round-to-nearest-even to the
16-bit storage format, which a float64 reference reproduces bit for bit: the tolerance of these tests is zero by
derivation.  The premise is asserted on the REFERENCE (conv_ref64), never on the kernel under test.
"""
import torch

from util import ACT_DTYPE

LIMIT = float(2 ** 24)

# a NaN bit pattern per element type (quiet NaN with a payload: no kernel produces it by arithmetic).  The integer types
# (sign-mask bytes, num_batches_tracked) have no NaN: a fill value stands in for it -- a test must not depend on it
# (compare inside the view only, check the surroundings with assert_guard_intact).
_NAN_BITS = {torch.bfloat16: (torch.int16, 0x7FC1), torch.float16: (torch.int16, 0x7E01),
             torch.float32: (torch.int32, 0x7FC00001), torch.float64: (torch.int64, 0x7FF8000000000001),
             torch.uint8: (torch.uint8, 0xA5), torch.int64: (torch.int64, 0x7FF8000000000001)}


def ints(shape, lo, hi, seed):
    """Integer-valued fp32 tensor, uniform in [lo, hi]."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(torch.float32)


def assert_integers(name, *ts):
    """The operands of an exact test: integer valued and representable in the 16-bit storage format."""
    for t in ts:
        t = t.detach().double().cpu()
        assert torch.equal(t, t.round()), "%s: operand is not integer valued" % name
        assert torch.equal(t.float().to(ACT_DTYPE).double(), t), "%s: operand not representable in %s" % (name, ACT_DTYPE)


def assert_premise(name, mag, limit=LIMIT):
    """`mag`: sums of absolute terms.  Every partial sum of the kernel is exact in fp32 when they stay below 2^24."""
    m = float(mag.max()) if mag.numel() else 0.0
    assert m < limit, "%s: exactness premise violated: sum of |terms| reaches %.0f >= 2^24 = %.0f" % (name, m, limit)


def conv_ref64(x, w, b=None, stride=1, pad=0, dil=1):
    """conv2d in float64 of integer-valued NCHW x and OIHW w (exact: fp64 holds integers to 2^53).  Beside it the same
    conv of |x| and |w| (+ |b|) bounds every partial sum any kernel can form; it must stay below 2^24."""
    F = torch.nn.functional
    assert_integers("conv_ref64", x, w, *([] if b is None else [b]))
    xd, wd = x.double(), w.double()
    bd = None if b is None else b.double()
    y = F.conv2d(xd, wd, bd, stride, pad, dil)
    mag = F.conv2d(xd.abs(), wd.abs(), None if bd is None else bd.abs(), stride, pad, dil)
    assert_premise("conv_ref64", mag)
    return y


def wgrad_ref64(x, dy, ksize, stride=1, pad=0, dil=1):
    """Weight gradient [Cout][Cin][KH][KW] in float64 of integer-valued NCHW x and dy; the premise bound is
    sum |x| |dy| over ALL pixels < 2^24 (the split of the pixel axis over workgroups is the kernel's business)."""
    assert_integers("wgrad_ref64", x, dy)

    def grad(xx, gg):
        w = torch.zeros(dy.shape[1], x.shape[1], ksize, ksize, dtype=torch.float64, requires_grad=True)
        torch.nn.functional.conv2d(xx, w, None, stride, pad, dil).backward(gg)
        return w.grad
    assert_premise("wgrad_ref64", grad(x.double().abs(), dy.double().abs()))
    return grad(x.double(), dy.double())


def to_act(ref64):
    """float64 -> fp32 (asserted exact) -> the 16-bit storage format (torch rounds to nearest even)."""
    f = ref64.to(torch.float32)
    assert torch.equal(f.double(), ref64), "reference is not exact in fp32"
    return f.to(ACT_DTYPE)


def to_f32(ref64):
    """float64 -> fp32, asserted exact (the reference of an fp32 output of an exact test)."""
    f = ref64.to(torch.float32)
    assert torch.equal(f.double(), ref64), "reference is not exact in fp32"
    return f


def not_representable(ref64):
    """How many reference values the 16-bit format cannot hold, i.e. where the rounding mode decides the result."""
    return int((to_act(ref64).double() != ref64).sum())


def _bits(t):
    t = t.detach()
    if t.dtype in _NAN_BITS:
        return t.contiguous().view(_NAN_BITS[t.dtype][0]).cpu()
    return t.contiguous().cpu()


def assert_bits_equal(name, got, ref, tile=None):
    """Bitwise equality of two tensors of one dtype (NaNs and signed zeros included).  On failure: the mismatch count,
    the first mismatching index (for NHWC activations (b, h, w, c)), got and ref there.  tile = (tile_h, tile_w,
    tiles_per_wg) of a persistent tile kernel adds the tile's index and its position in its strip."""
    assert got.dtype == ref.dtype, "%s: dtype %s != %s" % (name, got.dtype, ref.dtype)
    assert tuple(got.shape) == tuple(ref.shape), "%s: shape %s != %s" % (name, tuple(got.shape), tuple(ref.shape))
    gb, rb = _bits(got), _bits(ref)
    bad = gb != rb
    n = int(bad.sum())
    if n == 0:
        return
    idx = tuple(int(v) for v in bad.nonzero()[0])
    g, r = got.detach().cpu()[idx], ref.detach().cpu()[idx]
    mask = (1 << (8 * got.element_size())) - 1          # the element's own width: a negative integer view prints as its bits
    msg = "%s: %d of %d elements differ; first at %s: got %r (bits %#x) ref %r (bits %#x)" % (
        name, n, bad.numel(), idx, float(g), int(gb[idx]) & mask, float(r), int(rb[idx]) & mask)
    if tile is not None and got.dim() == 4:
        th, tw, tpw = tile
        B, H, W, _ = got.shape
        tiles_x, tiles_y = -(-W // tw), -(-H // th)
        t = (idx[0] * tiles_y + idx[1] // th) * tiles_x + idx[2] // tw
        total = B * tiles_x * tiles_y
        msg += "; tile %d of %d (image %d, tile row %d, tile column %d) = tile %d of strip %d (%d tiles per strip)" % (
            t, total, idx[0], idx[1] // th, idx[2] // tw, t % tpw, t // tpw, tpw)
    raise AssertionError(msg)


def assert_within_bound(name, got, ref64, bound):
    """|got - ref| <= bound at EVERY element, counted as `not (err <= bound)`: a NaN (an output the kernel never wrote, a
    result poisoned by a read of a NaN guard) or an infinity is a violation, never a pass.  bound: a float64 tensor that
    broadcasts against ref (a zero bound allows no error at all).  Returns the errors."""
    g, r = got.detach().double().cpu(), ref64.detach().double().cpu()
    assert tuple(g.shape) == tuple(r.shape), "%s: shape %s != %s" % (name, tuple(g.shape), tuple(r.shape))
    err = (g - r).abs()
    bad = ~(err <= bound)
    n = int(bad.sum())
    if n:
        idx = tuple(int(v) for v in bad.nonzero()[0])
        b = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
        raise AssertionError("%s: %d of %d elements exceed their bound (%d of them not finite); first at %s: got %r ref %r "
                             "error %.3g bound %.3g" % (name, n, err.numel(), int((~torch.isfinite(g)).sum()), idx, float(g[idx]),
                                                        float(r[idx]), float(err[idx]), float(b[idx])))
    return err


class Guarded:
    """`view`: the tensor a kernel reads or writes; `buf`: the flat buffer around it; `inside`: which elements of buf
    belong to the view."""

    def __init__(self, view, buf, inside, pattern):
        self.view, self.buf, self.inside, self.pattern = view, buf, inside, pattern


def guarded(shape, dtype, dev, ld=None, guard_bytes=4096):
    """A tensor of `shape` inside a larger buffer pre-filled with a NaN bit pattern: dense (ld None) or a channel
    slice of rows of `ld` > shape[-1] elements (the slice starts at a 16-byte aligned channel, its neighbours on both
    sides keep the pattern when ld - C allows).  The view is 16-byte aligned with at least 4 KB of guard on either
    side.  The view itself starts out as the pattern too: an element the kernel does not write stays NaN."""
    itype, pat = _NAN_BITS[dtype]
    isz = torch.empty((), dtype=dtype).element_size()
    C = shape[-1]
    rows = 1
    for s in shape[:-1]:
        rows *= s
    ld = C if ld is None else ld
    assert ld >= C
    per16 = 16 // isz
    c0 = ((ld - C) // 2) // per16 * per16
    guard = (max(guard_bytes, 4096) + 15) // 16 * 16 // isz
    n = guard + rows * ld + guard + per16
    raw = torch.full((n,), pat, dtype=itype, device=dev)
    off = guard + (-(raw.data_ptr() + guard * isz) % 16) // isz        # first element of row 0 on a 16-byte boundary
    buf = raw.view(dtype)
    assert (buf.data_ptr() + (off + c0) * isz) % 16 == 0 and off >= guard and n - (off + rows * ld) >= guard
    strides = [1] * len(shape)
    for i in range(len(shape) - 2, -1, -1):
        strides[i] = ld if i == len(shape) - 2 else strides[i + 1] * shape[i + 1]
    view = torch.as_strided(buf, tuple(shape), tuple(strides), off + c0)
    inside = torch.zeros(n, dtype=torch.bool)
    inside[off:off + rows * ld].view(rows, ld)[:, c0:c0 + C] = True
    assert view.data_ptr() % 16 == 0
    return Guarded(view, buf, inside, pat)


def guarded_copy(t, dev, ld=None):
    """`t` copied into a guarded buffer on `dev` (an INPUT whose surroundings are NaN: a stray read poisons the result)."""
    g = guarded(tuple(t.shape), t.dtype, dev, ld)
    g.view.copy_(t)
    return g


def assert_guard_intact(name, *gs):
    """The guard around every view, and the neighbouring channels of a slice, still hold the fill pattern bit for bit."""
    for g in gs:
        itype, pat = _NAN_BITS[g.buf.dtype]
        raw = g.buf.view(itype)                     # compared where the buffer lives: a device buffer may be hundreds of MB
        bad = (raw != torch.tensor(pat, dtype=itype, device=raw.device)) & ~g.inside.to(raw.device)
        n = int(bad.sum())
        if n:
            i = int(bad.nonzero()[0])
            first_in = int(g.inside.nonzero()[0])
            raise AssertionError("%s: %d guard elements overwritten; first at buffer element %d (the view starts at %d): "
                                 "bits %#x" % (name, n, i, first_in, int(raw[i]) & ((1 << (8 * g.buf.element_size())) - 1)))


# ---- helpers of the exact BatchNorm tests
def pow2(shape, lo, hi, seed, signed=False):
    """fp32 tensor of powers of two 2^k, k uniform in [lo, hi]; signed: with both signs."""
    g = torch.Generator().manual_seed(seed)
    v = 2.0 ** torch.randint(lo, hi + 1, tuple(shape), generator=g).float()
    if signed:
        v = v * (torch.randint(0, 2, tuple(shape), generator=g).float() * 2 - 1)
    return v


def choice(shape, values, seed):
    """fp32 tensor drawn uniformly from `values`."""
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), tuple(shape), generator=g)]


def sign_bytes(z):
    """The BatchNorm sign mask of z [P, C]: uint8 [P, C / 8], bit j of byte [p][c / 8] = z[p][8 (c / 8) + j] > 0."""
    P, C = z.shape
    assert C % 8 == 0
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=z.device)
    return ((z > 0).view(P, C // 8, 8).to(torch.int32) * w).sum(2).to(torch.uint8)


def split_replicas(total, nrep, seed, amp=2 ** 40):
    """`total` (integer-valued float64 [..]) split over nrep replicas [nrep, ..]: integer-valued float64 pieces, large and
    of mixed sign (|piece| up to `amp` against totals of a few thousand), whose sum -- in ANY order, every partial sum is
    an integer far below 2^53 -- is exactly `total`."""
    total = total.double()
    assert torch.equal(total, total.round()) and float(total.abs().max()) < 2.0 ** 40
    g = torch.Generator().manual_seed(seed)
    pieces = torch.randint(-amp, amp + 1, (nrep,) + tuple(total.shape), generator=g).double()
    pieces[nrep - 1] = total - pieces[:nrep - 1].sum(0)
    assert torch.equal(pieces.sum(0), total) and nrep * float(amp) < 2.0 ** 52
    if nrep > 1:        # large and of mixed sign: a replica left out or counted twice is off by far more than a rounding
        assert float(pieces.abs().max()) > 2.0 ** 30 and bool((pieces > 0).any()) and bool((pieces < 0).any())
    return pieces


def split_replicas_real(total, nrep, seed, amp=2 ** 20):
    """Real-valued float64 sums split over nrep replicas.  Returns (pieces [nrep, ..], the float64 sum of the pieces in
    replica order 0 .. nrep-1 from 0.0 -- the order the kernels add them in, which is therefore the value the
    reference has to start from: it differs from `total` by an fp64 rounding or two)."""
    total = total.double()
    g = torch.Generator().manual_seed(seed)
    pieces = torch.randint(-amp, amp + 1, (nrep,) + tuple(total.shape), generator=g).double()
    pieces[nrep - 1] = total - pieces[:nrep - 1].sum(0)
    acc = torch.zeros_like(total)
    for r in range(nrep):
        acc = acc + pieces[r]
    return pieces, acc


def ulp_err32(got, ref64):
    """|got - ref| in units of the fp32 spacing at |ref| (per element, float64): 0.5 is a correctly rounded cast.  ref = 0
    counts the spacing of the smallest normal number."""
    got, ref = got.detach().double().cpu(), ref64.detach().double().cpu()
    tiny = torch.tensor(2.0 ** -126, dtype=torch.float64)
    e = torch.floor(torch.log2(torch.maximum(ref.abs(), tiny)))
    # log2 of an fp64 just below a power of two may round up to it: put the exponent right
    e = torch.where(2.0 ** e > torch.maximum(ref.abs(), tiny), e - 1, e)
    return (got - ref).abs() / 2.0 ** (e - 23)
