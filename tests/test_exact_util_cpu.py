"""Self-test of the exact comparator (tests/exact_util.py): it must SEE a 1-ulp change of one element, one overwritten
guard element and a violated 2^24 premise -- a comparator that cannot fail proves nothing."""
import pytest
import torch

from util import ACT_DTYPE
from exact_util import (assert_bits_equal, assert_guard_intact, assert_integers, conv_ref64, guarded, guarded_copy, ints,
                        not_representable, to_act, wgrad_ref64)


def test_ints_are_integers_in_range_and_seeded():
    a, b = ints((3, 5, 7), -3, 4, seed=1), ints((3, 5, 7), -3, 4, seed=1)
    assert a.dtype == torch.float32 and torch.equal(a, b) and torch.equal(a, a.round())
    assert a.min() == -3 and a.max() == 4
    assert not torch.equal(a, ints((3, 5, 7), -3, 4, seed=2))


@pytest.mark.parametrize("dtype", [ACT_DTYPE, torch.float32, torch.float64])
def test_one_ulp_of_one_element_is_reported(dtype):
    ref = ints((2, 9, 40, 16), -300, 300, seed=3).to(dtype)
    ref[1, 6, 37, 5] = -300.0                              # a negative value: its integer view is negative
    got = ref.clone()
    assert_bits_equal("same", got, ref)
    itype = {2: torch.int16, 4: torch.int32, 8: torch.int64}[ref.element_size()]
    got.view(itype)[1, 6, 37, 5] += 1                       # the neighbouring value of the format: one ulp
    with pytest.raises(AssertionError) as e:
        assert_bits_equal("ulp", got, ref, tile=(4, 32, 3))
    msg = str(e.value)
    assert "1 of %d elements differ" % ref.numel() in msg and "(1, 6, 37, 5)" in msg
    # image 1, tile row 1, tile column 1 of a 3 x 2 tile grid: tile 6 + 2 + 1 = 9 -> strip 3, position 0
    assert "tile 9 of 12" in msg and "tile 0 of strip 3" in msg
    want_bits = int(got.view(itype)[1, 6, 37, 5]) & ((1 << (8 * ref.element_size())) - 1)
    assert "(bits %#x)" % want_bits in msg                    # printed at the element's own width, negative patterns too


def test_signed_zero_and_nan_payload_are_bits():
    a = torch.zeros(4, dtype=ACT_DTYPE)
    with pytest.raises(AssertionError):
        assert_bits_equal("zero", -a, a)
    n = torch.full((4,), float("nan"), dtype=torch.float32)
    assert_bits_equal("nan", n, n.clone())


def test_rounding_is_to_nearest_even():
    # 257 and 259 lie half way between bf16 neighbours (256, 258, 260): ties go to the even mantissa; fp16 holds both
    r = to_act(torch.tensor([257.0, 259.0, 2049.0, 2051.0], dtype=torch.float64)).double().tolist()
    assert r == ([256.0, 260.0, 2048.0, 2048.0] if ACT_DTYPE == torch.bfloat16 else [257.0, 259.0, 2048.0, 2052.0])
    assert not_representable(torch.tensor([255.0, 257.0, 2049.0], dtype=torch.float64)) == (2 if ACT_DTYPE == torch.bfloat16 else 1)
    with pytest.raises(AssertionError):
        to_act(torch.tensor([2.0 ** 24 + 1], dtype=torch.float64))


@pytest.mark.parametrize("ld", [None, 40])
@pytest.mark.parametrize("dtype", [ACT_DTYPE, torch.float64])
def test_guard_reports_one_overwritten_element(dtype, ld):
    g = guarded((2, 3, 5, 24), dtype, "cpu", ld)
    assert g.view.shape == (2, 3, 5, 24) and g.view.data_ptr() % 16 == 0
    assert torch.isnan(g.view).all()                           # an element nobody writes stays NaN
    first = int(g.inside.nonzero()[0])
    last = int(g.inside.nonzero()[-1])
    assert first * g.buf.element_size() >= 4096 and (g.buf.numel() - 1 - last) * g.buf.element_size() >= 4096
    g.view.copy_(ints((2, 3, 5, 24), -9, 9, seed=4).to(dtype))
    assert_guard_intact("clean", g)
    assert int(g.inside.sum()) == g.view.numel()
    for where in ([first - 1, last + 1] + ([first + 24] if ld else [])):      # in front, behind, the slice's neighbour
        saved = g.buf[where].clone()
        g.buf[where] = 1.0
        with pytest.raises(AssertionError) as e:
            assert_guard_intact("dirty", g)
        assert "1 guard elements overwritten" in str(e.value) and "element %d" % where in str(e.value)
        g.buf[where] = saved
        assert_guard_intact("restored", g)
    # a NaN of another payload is not the pattern
    g.buf[first - 1] = float("nan")
    if not torch.equal(g.buf[first - 1:first].view(torch.int16 if dtype == ACT_DTYPE else torch.int64),
                       torch.tensor([g.pattern], dtype=torch.int16 if dtype == ACT_DTYPE else torch.int64)):
        with pytest.raises(AssertionError):
            assert_guard_intact("nan", g)


def test_guarded_copy_of_a_slice_keeps_nan_neighbours():
    t = ints((1, 4, 6, 48), -3, 3, seed=5).to(ACT_DTYPE)
    g = guarded_copy(t, "cpu", ld=96)
    assert torch.equal(g.view, t) and g.view.stride() == (4 * 6 * 96, 6 * 96, 96, 1)
    assert int(torch.isnan(g.buf.float()).sum()) == g.buf.numel() - t.numel()


def test_violated_premise_is_reported():
    x = ints((1, 8, 6, 6), 200, 200, seed=0)
    w = ints((8, 8, 3, 3), 200, 200, seed=0)
    conv_ref64(x, w, None, 1, 1, 1)                            # 72 * 40000 = 2.88e6
    x6 = ints((1, 48, 6, 6), 200, 200, seed=0)
    w6 = ints((8, 48, 3, 3), 200, 200, seed=0)
    with pytest.raises(AssertionError, match="premise violated"):
        conv_ref64(x6, w6, None, 1, 1, 1)                      # 432 * 40000 = 1.728e7 >= 2^24
    with pytest.raises(AssertionError, match="premise violated"):   # the products cancel: the bound is on |x| |w|
        conv_ref64(x6, w6 * torch.tensor([1.0, -1.0]).repeat(24).view(1, 48, 1, 1), None, 1, 1, 1)
    with pytest.raises(AssertionError, match="not integer"):
        conv_ref64(x * 0.5 + 0.25, w, None, 1, 1, 1)
    with pytest.raises(AssertionError, match="not representable"):
        assert_integers("big", torch.tensor([4097.0 if ACT_DTYPE == torch.float16 else 257.0]))
    dy = ints((1, 8, 6, 6), 100, 100, seed=0)
    wgrad_ref64(x, dy, 3, 1, 1, 1)                             # 36 * 20000
    with pytest.raises(AssertionError, match="premise violated"):
        wgrad_ref64(x.repeat(1, 1, 6, 6), dy.repeat(1, 1, 6, 6), 3, 1, 1, 1)     # 1296 * 20000 = 2.6e7


def test_references_against_a_direct_sum():
    x, w = ints((2, 3, 5, 4), -3, 3, seed=6), ints((4, 3, 3, 3), -2, 2, seed=7)
    y = conv_ref64(x, w, None, 1, 1, 1)
    xp = torch.nn.functional.pad(x.double(), (1, 1, 1, 1))
    want = sum(float(xp[1, c, 2 + kh, 1 + kw] * w[2, c, kh, kw]) for c in range(3) for kh in range(3) for kw in range(3))
    assert float(y[1, 2, 2, 1]) == want
    dy = ints((2, 4, 5, 4), -2, 2, seed=8)
    dw = wgrad_ref64(x, dy, 3, 1, 1, 1)
    want = sum(float(xp[b, 1, oy + 0, ox + 2] * dy[b, 3, oy, ox]) for b in range(2) for oy in range(5) for ox in range(4))
    assert float(dw[3, 1, 0, 2]) == want


# ---- the helpers of the exact BatchNorm tests
from exact_util import choice, pow2, sign_bytes, split_replicas, split_replicas_real, to_f32, ulp_err32  # noqa: E402


@pytest.mark.parametrize("dtype,shape", [(torch.uint8, (7, 6)), (torch.int64, (1,)), (torch.float32, (4, 24))])
def test_guard_of_the_integer_buffers_reports_one_overwritten_element(dtype, shape):
    """The sign-mask bytes and num_batches_tracked have no NaN: the guard is a fill value, reported all the same."""
    g = guarded(shape, dtype, "cpu")
    assert g.view.shape == shape and g.view.data_ptr() % 16 == 0 and int(g.inside.sum()) == g.view.numel()
    g.view.copy_(torch.arange(g.view.numel()).view(shape).to(dtype))
    assert_guard_intact("clean", g)
    first, last = int(g.inside.nonzero()[0]), int(g.inside.nonzero()[-1])
    for where in (first - 1, last + 1):
        saved = g.buf[where].clone()
        g.buf[where] = 1
        with pytest.raises(AssertionError, match="1 guard elements overwritten"):
            assert_guard_intact("dirty", g)
        g.buf[where] = saved
    assert_guard_intact("restored", g)
    got = g.view.clone()
    assert_bits_equal("same", got, g.view)
    got.view(-1)[got.numel() - 1] += 1
    with pytest.raises(AssertionError, match="1 of %d elements differ" % got.numel()):
        assert_bits_equal("one off", got, g.view)


def test_pow2_and_choice_draw_what_they_say():
    p = pow2((500,), -2, 2, seed=1, signed=True)
    assert set(p.abs().tolist()) == {0.25, 0.5, 1.0, 2.0, 4.0} and (p > 0).any() and (p < 0).any()
    assert (pow2((50,), -2, 1, seed=2) > 0).all() and torch.equal(pow2((50,), -2, 1, seed=2), pow2((50,), -2, 1, seed=2))
    c = choice((3, 200), [0.0, 0.5, 1.0, 2.0], seed=3)
    assert c.shape == (3, 200) and set(c.flatten().tolist()) == {0.0, 0.5, 1.0, 2.0}


def test_sign_bytes_bit_order():
    z = torch.zeros(2, 16)
    z[0, 0], z[0, 3], z[0, 15], z[1, 8], z[1, 9] = 1.0, 0.5, 2.0, -1.0, 3.0          # negative and zero: bit clear
    z[1, 1] = -0.0
    assert sign_bytes(z).tolist() == [[0b00001001, 0b10000000], [0, 0b00000010]]
    assert sign_bytes(z.to(ACT_DTYPE)).dtype == torch.uint8


def test_split_replicas_sums_exactly_in_any_order():
    total = ints((2, 40), -3000, 3000, seed=9).double() * 1024
    assert torch.equal(split_replicas(total, 1, seed=1)[0], total)
    for nrep in (4, 11):
        p = split_replicas(total, nrep, seed=nrep)
        assert p.shape == (nrep, 2, 40) and torch.equal(p, p.round())
        assert torch.equal(p.sum(0), total) and torch.equal(p.flip(0).sum(0), total)
        acc = torch.zeros_like(total)
        for r in torch.randperm(nrep).tolist():
            acc = acc + p[r]
        assert torch.equal(acc, total)
        assert float(p.abs().max()) > 2.0 ** 30 and (p > 0).any() and (p < 0).any()
    with pytest.raises(AssertionError):
        split_replicas(total + 0.5, 4, seed=0)
    real = torch.rand(2, 40, dtype=torch.float64) * 1e5
    p, acc = split_replicas_real(real, 11, seed=5)
    want = torch.zeros_like(real)
    for r in range(11):
        want = want + p[r]
    assert torch.equal(acc, want) and float(((acc - real).abs() / real).max()) < 1e-9


def test_ulp_err32_counts_fp32_spacings():
    ref = torch.tensor([1.0, 1.5, -3.0, 0.3, 2.0 ** -3, 1e-3], dtype=torch.float64)
    f = ref.float()
    assert float(ulp_err32(f, f.double()).max()) == 0.0
    up = (f.view(torch.int32) + 1).view(torch.float32)                  # the next fp32 away from zero
    e = ulp_err32(up, f.double())
    assert torch.equal(e, torch.ones_like(e)), e
    # a correctly rounded cast is at most half a spacing off; just below a power of two the spacing is the smaller one
    r64 = torch.tensor([0.1, 1.0 / 3.0, 2.0 - 2.0 ** -30], dtype=torch.float64)
    e = ulp_err32(r64.float(), r64)
    assert float(e.max()) <= 0.5 and float(e.min()) > 0.0
    assert float(ulp_err32(torch.tensor([2.0]), torch.tensor([2.0 - 2.0 ** -30], dtype=torch.float64))) == pytest.approx(2.0 ** -7)
    with pytest.raises(AssertionError):
        to_f32(torch.tensor([0.1], dtype=torch.float64))
    assert to_f32(torch.tensor([0.375], dtype=torch.float64)).dtype == torch.float32



from exact_util import assert_within_bound  # noqa: E402


def test_within_bound_counts_nan_and_infinity_as_violations():
    """The comparator of the bounded tests: outputs start as a NaN pattern, so an element the kernel never wrote -- or one
    poisoned by a read of an input's NaN guard -- must FAIL, although `nan > bound` is False."""
    ref = torch.arange(12, dtype=torch.float64).view(3, 4)
    bound = torch.full((3, 4), 0.5, dtype=torch.float64)
    got = ref.float() + 0.25
    assert torch.equal(assert_within_bound("ok", got, ref, bound), torch.full((3, 4), 0.25, dtype=torch.float64))
    assert_within_bound("at the bound", ref + 0.5, ref, bound)
    for poison in (float("nan"), float("inf"), -float("inf")):
        bad = got.clone()
        bad[1, 2] = poison
        with pytest.raises(AssertionError, match=r"1 of 12 elements exceed their bound \(1 of them not finite\); first at \(1, 2\)"):
            assert_within_bound("poisoned", bad, ref, bound)
    guarded_out = guarded((3, 4), torch.float32, "cpu")                  # as a kernel's output buffer starts out
    with pytest.raises(AssertionError, match="12 of 12 elements"):
        assert_within_bound("unwritten", guarded_out.view, ref, bound)
    over = got.clone()
    over[2, 3] += 0.5
    with pytest.raises(AssertionError, match=r"1 of 12 elements exceed their bound \(0 of them not finite\); first at \(2, 3\)"):
        assert_within_bound("over", over, ref, bound)
    zero = torch.zeros(3, 4, dtype=torch.float64)                        # a zero bound allows no error at all
    assert_within_bound("exact", ref, ref, zero)
    with pytest.raises(AssertionError):
        assert_within_bound("zero bound", ref + 1e-9, ref, zero)
    with pytest.raises(AssertionError, match="shape"):
        assert_within_bound("shape", got[:2], ref, bound)
