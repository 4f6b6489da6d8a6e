"""The references, premises and regimes of tests/ocr_cases.py, checked without a GPU: each reference against
oracle.ops.object_attention / spatial_gather run in float64 with autograd, each case on the mirrors of the kernels'
index arithmetic in the regime it is listed for."""
import math

import pytest
import torch

import ocr_cases as OC
from oracle import ops as O
from resample_ref import _MANT
from util import ACT_DTYPE

D = OC.D


def test_acc_row_mirror():
    """acc_row is a bijection of (register, lane half) onto the 32 regions of an m-block, and region_home inverts it."""
    for mb in range(3):
        seen = {}
        for h in range(2):
            for r in range(16):
                region = OC.acc_row(mb, r, h)
                assert region not in seen
                seen[region] = (mb, h)
                assert OC.region_home(region) == (mb, h)
        assert sorted(seen) == list(range(mb * 32, mb * 32 + 32))


def test_tie_case_lists():
    """Every K and every P of the issue's lists appears; every group size 1 .. 32 appears; from 33 regions on a group
    spans both lane halves and two m-blocks; four cases run on wider rows, each operand with its own extra stride."""
    assert {k for k, _ in OC.TIE_KP} == {1, 19, 31, 32, 33, 64, 65, 95, 96}
    assert {p for _, p in OC.TIE_KP} == {1, 31, 33, 127, 128, 129, 300}
    assert OC.GROUPS[19] == [8, 4, 4, 2, 1]
    assert {s for k, _ in OC.TIE_KP for s in OC.GROUPS[k]} == {1, 2, 4, 8, 16, 32}
    for K, P in OC.TIE_KP + [(97, 300)]:
        group, sizes = OC.tie_groups(K, 9100)
        assert torch.equal(torch.bincount(group, minlength=len(sizes)), sizes)
        targeted = set((torch.arange(P) % len(sizes)).tolist())
        homes = [{OC.region_home(int(r)) for r in (group == g).nonzero().flatten()} for g in sorted(targeted)]
        if K >= 33 and P >= len(sizes):
            assert any(len({mb for mb, _ in hs}) >= 2 and len({h for _, h in hs}) == 2 for hs in homes), K
    assert len(OC.TIE_LD) >= 3 and set(OC.TIE_LD) <= set(OC.TIE_KP)
    for extra in OC.TIE_LD.values():
        assert len(set(extra)) == 4 and all(e > 0 and e % 8 == 0 for e in extra)
    assert OC.attn_tiles(OC.GRID_STRIDE_KP[1]) == (1026, 1024)
    assert all(OC.attn_tiles(P)[0] == OC.attn_tiles(P)[1] for _, P in OC.TIE_KP)      # no second tile anywhere else


def _oracle_attention(c):
    q, k, v, dout = (c[n].double() for n in ("q", "k", "v", "dout"))
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = O.object_attention(q[None], k.t()[None], v[None], D)[0]
    out.backward(dout)
    return out.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("K,P", [(1, 129), (19, 300), (33, 128), (65, 300), (96, 300), (97, 33)])
def test_tie_reference_against_oracle(K, P):
    """The tie reference equals softmax attention in float64 up to float64 rounding, wherever it is not rounded to 16 bit
    on the way: out and dv (exact probabilities) directly, dq and dk recomputed from the unrounded dsim."""
    c = OC.tie_case(K, P)
    out, dq, dk, dv = _oracle_attention(c)
    q, k, v, dout = (c[n].double() for n in ("q", "k", "v", "dout"))
    probs = c["probsG"][c["pixel_group"]]
    sim = q @ k.t() * OC.SCALE
    assert float((torch.softmax(sim, 1) - probs).abs().max()) <= math.exp(-OC.SEPARATION) * K
    tol = 2.0 ** -40

    def close(name, a, b):
        err = float((a - b).abs().max())
        assert err <= tol * max(1.0, float(b.abs().max())), "%s: %g" % (name, err)
    close("out", probs @ v, out)
    assert torch.equal(c["out"].double(), (probs @ v).float().to(ACT_DTYPE).double())
    close("dv", c["dv64"], dv)
    dp = dout @ v.t()
    dsim = OC.SCALE * probs * (dp - (probs * dp).sum(1, keepdim=True))
    close("dq (unrounded dsim)", dsim @ k, dq)
    close("dk (unrounded dsim)", dsim.t() @ q, dk)
    # the rounded dsim is within half a storage step of it, and dq / dk are its products
    d16 = c["dsim"].double()[:, :K]
    assert bool(((d16 - dsim).abs() <= OC.step16(dsim) / 2).all())
    assert torch.equal(c["dq"].double(), (d16 @ k).float().to(ACT_DTYPE).double())
    assert torch.equal(c["dk64"], d16.t() @ q + 0.0)
    if K > 1:
        assert c["dsim_rounded"] > 0.0 or _MANT > 7, "no dsim value of this case needs the rounding"


def test_one_region_and_bounded_references():
    c = OC.k1_real_case(129)
    out = O.object_attention(c["q"].double()[None], c["k"].double().t()[None], c["v"].double()[None], D)[0]
    assert torch.equal(out, c["v"].double().expand(129, D))
    for K in (19, 65, 96):
        b = OC.bounded_case(K, 300)
        ref = O.object_attention(b["q"].double()[None], b["k"].double().t()[None], b["v"].double()[None], D)[0]
        # rounding the probabilities moves out by at most sum |v| * half a step
        slack = (OC.step16(torch.softmax(b["q"].double() @ b["k"].double().t() / 16, 1)) / 2) @ b["v"].double().abs()
        assert bool(((ref - b["out"]).abs() <= slack + 1e-12).all())
        assert float(b["probs"][:, K:].abs().sum()) == 0.0 and float(b["probs_bound"][:, K:].abs().sum()) == 0.0
        assert float(b["out_bound"].max()) < 0.05       # far below the 1e-2 * max|ref| of the tolerance test it sits beside


def test_gather_case_lists():
    """Every top value, every size, every placement; a class spread over >= 3 workgroups; the re-balanced plan."""
    names, sizes = set(), set()
    spread = 0
    for name, K, H, W, C, pad in OC.GATHER:
        c = OC.gather_case(K, H * W, C)
        HW = H * W
        RP, ppb, blocks = c["plan"]
        names |= set(c["top_names"])
        sizes |= set(c["m"].tolist())
        if K >= 7:
            assert set(c["top_names"]) == {"-40", "-17", "-3.5", "-0.0", "0", "2.25", "30"}, name
        if K >= 4:
            tops = [set(t.tolist()) for t in c["tops"]]
            assert any(0 in t for t in tops) and any(HW - 1 in t for t in tops)
            assert any(min(t) >= (blocks - 1) * ppb for t in tops)              # a class wholly in the ragged last range
        spread += sum(len(OC.blocks_of(c, k)) >= 3 for k in range(K))
    assert names == {"-40", "-17", "-3.5", "-0.0", "0", "2.25", "30"} and sizes == {1, 2, 4, 8, 16, 32}
    assert spread > 0
    assert sum(1 for g in OC.GATHER if g[5] > 0) == 2
    assert OC.stats_plan(13 * 21, 65) == (3, 48, 6) and 13 * 21 % 48 != 0
    name, K, H, W, C, pad = OC.GATHER_REBALANCE
    RP, ppb, blocks = OC.stats_plan(H * W, K)
    assert (H * W + 15) // 16 > 1024 and ppb == 17 and blocks == 972 and blocks > 1
    for n, K, H, W, C, pad in OC.GATHER:
        assert (H * W + OC.stats_plan(H * W, K)[1] - 1) // OC.stats_plan(H * W, K)[1] <= 1024, n


def test_gather_rebalance_placement():
    name, K, H, W, C, pad = OC.GATHER_REBALANCE
    c = OC.gather_case(K, H * W, C)
    blocks = c["plan"][2]
    assert any({0, blocks - 1} <= set(OC.blocks_of(c, k)) and any(0 < b < blocks - 1 for b in OC.blocks_of(c, k))
               for k in range(K)), "no class has top pixels in the first, a middle and the last workgroup"


@pytest.mark.parametrize("case", OC.GATHER, ids=[g[0] for g in OC.GATHER])
def test_gather_reference_against_oracle(case):
    name, K, H, W, C, pad = case
    c = OC.gather_case(K, H * W, C)
    feats = c["feats"].double().t().reshape(1, C, H, W).clone().requires_grad_(True)
    logits = c["logits"].double().t().reshape(1, K, H, W).clone().requires_grad_(True)
    ctx = O.spatial_gather(feats, logits)                           # [1, C, K, 1]
    ctx.backward(c["dctx"].double().t().reshape(1, C, K, 1))
    tol = 2.0 ** -40

    def close(name, a, b):
        err = float((a - b).abs().max())
        assert err <= tol * max(1.0, float(b.abs().max())), "%s: %g" % (name, err)
    close("ctx", c["ctx"].double(), ctx[0, :, :, 0].t().detach())
    close("dlogits", c["dlogits"].double(), logits.grad.reshape(K, H * W).t())
    dfeats = feats.grad.reshape(C, H * W).t()
    assert torch.equal(c["dfeats"].double(), (c["probs64"] @ c["dctx"].double()).float().to(ACT_DTYPE).double())
    close("dfeats (unrounded)", c["probs64"] @ c["dctx"].double(), dfeats)
    assert float(c["probs"].double()[:, K:].abs().sum()) == 0.0
