"""The seeded cases of the label relaxation tests (tests/test_relaxloss_cpu.py, tests/test_relaxloss_gpu.py and, under
the CPU emulation, tests/test_relaxloss_emu_cpu.py) and of tests/golden/make_golden_relaxloss.py.

Label maps are 4 x 4 constant blocks with 5 % scattered ignore labels (which never make a pixel without a real class: a
neighbour always has one), one ignore rectangle of (2b+3)^2 (its core of 3 x 3 sees nothing but ignore labels) and one
full ignore column.  Cases 1-7 have golden data from the real reference; case 8 is for tile seams and is compared with
tests/relaxloss_ref.py only: 70 x 299 spans 9 x 10 label tiles of the stencil kernel (8 rows x 32 columns) with a ragged
last tile in both directions (70 = 8 * 8 + 6, 299 = 9 * 32 + 11), and 82 tiles of 256 pixels of the loss kernel, the last
one of 194."""
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "relaxloss_golden.pt")

# id: C, ignore, (B, H, W), border, strict, batch weights, upper bound, logit sigma, upstream
CASES = {
    1: dict(C=19, ignore=255, shape=(1, 13, 18), border=1, strict=None, batch=False, ub=1.0, sigma=2.0, up=1.0),
    2: dict(C=19, ignore=255, shape=(2, 13, 18), border=1, strict=None, batch=False, ub=1.0, sigma=2.0, up=1.7),
    3: dict(C=19, ignore=255, shape=(2, 17, 23), border=1, strict=[3, 7], batch=True, ub=0.5, sigma=3.0, up=1.7),
    4: dict(C=19, ignore=255, shape=(3, 17, 23), border=2, strict=None, batch=False, ub=1.0, sigma=3.0, up=1.0),
    5: dict(C=65, ignore=65, shape=(2, 15, 18), border=1, strict=[0], batch=False, ub=1.0, sigma=2.0, up=1.0),
    6: dict(C=19, ignore=255, shape=(2, 17, 23), border=1, strict=None, batch=False, ub=1.0, sigma=12.0, up=1.0),
    7: dict(C=19, ignore=255, shape=(2, 9, 11), border=1, strict=None, batch=False, ub=1.0, sigma=2.0, up=1.0,
            all_ignore_image=0),
    8: dict(C=19, ignore=255, shape=(1, 70, 299), border=1, strict=None, batch=False, ub=1.0, sigma=2.0, up=1.0),
}
GOLDEN_CASES = (1, 2, 3, 4, 5, 6, 7)
SLICED_CASES = (2, 5)          # also run with the logits as a channel slice of a wider NHWC buffer (ld > C)


def inputs(n):
    """(logits fp32 [B,C,H,W], labels uint8 [B,H,W]) of case n, from its seed"""
    k = CASES[n]
    C, (B, H, W), b = k["C"], k["shape"], k["border"]
    g = torch.Generator().manual_seed(7100 + n)
    logits = torch.randn(B, C, H, W, generator=g) * k["sigma"]
    blocks = torch.randint(0, C, (B, (H + 3) // 4, (W + 3) // 4), generator=g)
    gts = blocks.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W].clone()
    gts[torch.rand(B, H, W, generator=g) < 0.05] = k["ignore"]
    r = 2 * b + 3
    for i in range(B):
        y0 = int(torch.randint(0, H - r + 1, (1,), generator=g))
        x0 = int(torch.randint(0, W - r + 1, (1,), generator=g))
        gts[i, y0:y0 + r, x0:x0 + r] = k["ignore"]
    gts[B - 1, :, int(torch.randint(0, W, (1,), generator=g))] = k["ignore"]
    if "all_ignore_image" in k:
        gts[k["all_ignore_image"]] = k["ignore"]
    return logits, gts.to(torch.uint8)


def checksum(logits):
    return logits.double().sum(), logits.double().abs().sum()


_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = torch.load(GOLDEN)
    return _GOLDEN


_REF = {}


def reference(n):
    """What the tests hold the kernels to, computed once per case: the golden data of the real reference for cases 1-7
    (multi-hot target, class weights, loss, gradient), tests/relaxloss_ref.py for case 8; class sets and counts from the
    restatement over that target.  dict(logits, labels, mh, sets, stats, w, loss, grad [B,C,H,W])."""
    if n in _REF:
        return _REF[n]
    import relaxloss_ref as R
    k = CASES[n]
    logits, labels = inputs(n)
    if n in GOLDEN_CASES:
        gd = golden()["case%d" % n]
        s, a = checksum(logits)
        assert torch.equal(gd["labels"], labels) and float(gd["logits_sum"]) == float(s) and \
            float(gd["logits_abs_sum"]) == float(a), "case %d: the seeded inputs are not the ones the fixture was made of" % n
        mh, w, loss, grad = gd["multihot"].numpy(), gd["weights"], gd["loss"].double(), gd["grad"]
    else:
        mh = R.multihot(labels.numpy(), k["C"], k["ignore"], k["border"], k["strict"])
        w = R.class_weights(mh, k["ub"], k["batch"])
        x = logits.double().requires_grad_(True)
        loss = R.loss(x, mh, k["ub"], k["batch"])
        (loss * k["up"]).backward()
        loss, grad = loss.detach(), x.grad.float()
    _REF[n] = dict(logits=logits, labels=labels, mh=torch.from_numpy(mh), sets=R.class_sets(mh), stats=R.stats(mh), w=w,
                   loss=loss, grad=grad)
    return _REF[n]
