"""Float64 restatement of the Dense Prediction Cell (network/utils.py:249-298 of the reference) for the tests: a plain
module (not a conftest), torch only, NCHW.  Written from the paper's cell and the reference's constructor arguments, tap
by tap over index ranges -- no library convolution -- so that a transposed rate pair, a wrong wiring or a wrong
concatenation order cannot hide behind a shared implementation.  tests/test_dpc_wiring_cpu.py checks it against the
golden vectors of the real module (tests/golden/make_golden_dpc.py).

Also the deterministic inputs the golden generator and the tests share (the golden stores seeds, not the tensors)."""
import torch

RATES = ((1, 6), (18, 15), (6, 21), (1, 1), (6, 3))       # (dil_h, dil_w) at output stride 16
NAMES = ("a", "b", "c", "d", "e")
EPS, MOMENTUM = 1e-5, 0.1

# the module-alone records of the golden: output stride -> (B, in_dim, reduction_dim, H, W); H != W, and for every rate
# pair of that stride H > dil_h and W > dil_w (off-centre taps inside the image on both axes)
MODULE_CASES = {16: (2, 6, 4, 24, 28), 8: (1, 6, 4, 48, 52)}
NET_BATCH = (2, 384, 416, 4321)                           # B, H, W, seed of the network record: 48 x 52 at stride 8


def rates_for(output_stride):
    if output_stride == 8:
        return tuple((2 * h, 2 * w) for h, w in RATES)
    if output_stride == 16:
        return RATES
    raise ValueError("output stride of {} not supported".format(output_stride))


def assert_taps_inside(H, W, output_stride):
    for dh, dw in rates_for(output_stride):
        assert H > dh and W > dw, "a %d x %d map is blind to the rate pair (%d, %d)" % (H, W, dh, dw)


def module_shapes(in_dim, red):
    """State-dict keys and shapes of DPC(in_dim, red), in order (`drop` has none)."""
    out = []
    for n in NAMES:
        cin = in_dim if n == "a" else red
        out += [("%s.0.weight" % n, (red, cin, 3, 3)), ("%s.1.weight" % n, (red,)), ("%s.1.bias" % n, (red,)),
                ("%s.1.running_mean" % n, (red,)), ("%s.1.running_var" % n, (red,)), ("%s.1.num_batches_tracked" % n, ())]
    return out


def pattern(shape, mul, mod):
    """A deterministic tensor in [-0.5, 0.5) from integer arithmetic only (identical on every machine)."""
    n = 1
    for s in shape:
        n *= s
    return (((torch.arange(n, dtype=torch.int64) * mul) % mod).double() / mod - 0.5).reshape(shape)


def module_inputs(output_stride):
    """x [B,in_dim,H,W] and the weights `gy` of the scalar loss sum(out * gy), float64."""
    B, cin, red, H, W = MODULE_CASES[output_stride]
    return pattern((B, cin, H, W), 7919, 1013) * 4.0, pattern((B, 5 * red, H, W), 104729, 2003)


def synth_batch(B, H, W, C=19, seed=1234):
    """tests/golden/make_golden.py's synthetic batch: N(0,1) image, block-constant labels with ~10 % ignore."""
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(B, 3, H, W, generator=g)
    bs = 16
    blocks = torch.randint(0, C, (B, (H + bs - 1) // bs, (W + bs - 1) // bs), generator=g)
    gts = blocks.repeat_interleave(bs, 1).repeat_interleave(bs, 2)[:, :H, :W].clone()
    gts[torch.rand(B, H, W, generator=g) < 0.1] = 255
    return images, gts.long()


# ---- the cell
def _tap(n, d, k):
    """Output and input indices along one axis for tap k (0..2) of a 3-tap conv, stride 1, padding = dilation = d."""
    o = torch.arange(n)
    i = o + (k - 1) * d
    m = (i >= 0) & (i < n)
    return o[m], i[m]


def dil_conv(x, w, dil_h, dil_w):
    """3x3 conv, stride 1, padding = dilation = (dil_h, dil_w), no bias.  x [B,Cin,H,W], w [Cout,Cin,3,3]."""
    B, _, H, W = x.shape
    y = x.new_zeros(B, w.shape[0], H, W)
    for kh in range(3):
        oy, iy = _tap(H, dil_h, kh)
        for kw in range(3):
            ox, ix = _tap(W, dil_w, kw)
            if len(oy) and len(ox):
                xs = x[:, :, iy[:, None], ix[None, :]]
                y[:, :, oy[:, None], ox[None, :]] += torch.einsum("bihw,oi->bohw", xs, w[:, :, kh, kw])
    return y


def _bn_relu(y, sd, name, training, new_stats):
    g, b = sd[name + ".1.weight"], sd[name + ".1.bias"]
    if training:
        n = y.numel() // y.shape[1]
        mean = y.mean((0, 2, 3))
        var = y.var((0, 2, 3), unbiased=False)
        new_stats[name + ".1.running_mean"] = (1 - MOMENTUM) * sd[name + ".1.running_mean"] + MOMENTUM * mean.detach()
        new_stats[name + ".1.running_var"] = (1 - MOMENTUM) * sd[name + ".1.running_var"] + MOMENTUM * var.detach() * n / (n - 1)
    else:
        mean, var = sd[name + ".1.running_mean"], sd[name + ".1.running_var"]
    z = (y - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + EPS)
    return torch.relu(z * g[None, :, None, None] + b[None, :, None, None])


def dpc(x, sd, output_stride, training, swap_axes=False):
    """The cell: a(x), b(a), c(a), d(a), e(b), concatenated a, b, c, d, e.  sd: the module's state dict (float64; the
    conv weights may require grad).  Returns (out, the running statistics after this pass -- empty in evaluation).
    swap_axes: every rate pair transposed, (dil_w, dil_h) -- the mistake the tests must be able to see."""
    rates = rates_for(output_stride)
    if swap_axes:
        rates = tuple((w, h) for h, w in rates)
    new_stats = {}

    def layer(name, t, r):
        return _bn_relu(dil_conv(t, sd[name + ".0.weight"], r[0], r[1]), sd, name, training, new_stats)
    a = layer("a", x, rates[0])
    b = layer("b", a, rates[1])
    c = layer("c", a, rates[2])
    d = layer("d", a, rates[3])
    e = layer("e", b, rates[4])
    return torch.cat((a, b, c, d, e), 1), new_stats
