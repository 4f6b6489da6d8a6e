"""Input builders and float64 references of the exact / bounded OCR head tests (tests/test_exact_ocr_gpu.py and
tests/test_ocr_cases_cpu.py share them; a plain module).  Every premise is asserted here, on the reference.

Object attention, "tie" cases (csrc/ocr_attn.hip and the three-launch form; D = 256, scale = 2^-4):
  The K regions are split into groups of power-of-two sizes m by a seeded permutation; group g has an integer key vector
  in [-4, 4]^256, k[r] = key[group(r)], and pixel p targets group g(p) = p mod G with q[p] = 8 key[g(p)].  sim = q k^T / 16
  is then an integer or half-integer, exactly tied inside the target group and (asserted) >= 128 below it elsewhere:
  exp(-128) = 2^-184.7 is below half the smallest fp32 denormal 2^-150, so those probabilities are 0 in ANY exp
  implementation and the probabilities are exactly 1/m on the group.  With integer v and dout every later value is a
  multiple of a power-of-two quantum (1/m for out, dv and the row dot; 2^-4 / m^2 for dsim, before AND after its
  rounding to 16 bit, since a rounding step is a coarser power of two), every sum of absolute terms stays below 2^24
  quanta (assert_premise), so every fp32 partial sum in any order is exact and float64 with ONE final rounding is the
  kernels' result bit for bit.  Zeros: the kernels add products into a +0.0 accumulator, so a sum of zero terms is +0.0
  (the references add 0.0 to every matmul); the element-wise dsim = (scale * probs) * (dprobs - dot) keeps the sign of
  its second factor where probs = +0.0, in fp32 as in float64.

HW softmax / spatial gather, exact cases (csrc/ocr.hip; logits fp32 [HW, K]):
  Class k has a top value from TOPS at m_k in {1 .. 32} pixels and every other pixel 128 to 177 below it, so
  probs = 1/m_k on the top pixels, exactly.  The +0.0 class has +0.0 at its first top pixel and -0.0 at the others (they
  tie numerically and order below +0.0 as bit patterns); the -0.0 class has only strictly negative lows.
"""
import torch

from exact_util import assert_integers, assert_premise, ints, not_representable, to_act, to_f32
from resample_ref import _MANT, half_ulp_act
from util import ACT_DTYPE, bf16_round

D = 256
SCALE = 2.0 ** -4                   # 256 ** -0.5
SEPARATION = 128.0                  # exp(-128) < 2^-150: derived, see above

# group sizes per region count (19 = Cityscapes, 65 = Mapillary, 96 = the fused kernel's limit, 97 = the fallback)
GROUPS = {1: [1], 19: [8, 4, 4, 2, 1], 31: [16, 8, 4, 2, 1], 32: [32], 33: [16, 8, 4, 2, 2, 1],
          64: [32, 16, 8, 4, 2, 1, 1], 65: [32, 16, 8, 4, 2, 2, 1], 95: [32, 32, 16, 8, 4, 2, 1],
          96: [32, 32, 16, 8, 4, 2, 1, 1], 97: [32, 32, 16, 8, 4, 2, 2, 1]}

# (K, P) of the tie cases run through the C ABI: every K and every P once at least, no full product
TIE_KP = [(1, 1), (1, 129), (19, 31), (19, 300), (31, 33), (32, 127), (33, 128), (64, 129), (65, 300), (95, 33),
          (96, 1), (96, 300)]
# extra row strides (ldq, ldo, lddo, lddq) - 256 of the cases run as channel slices of wider rows
TIE_LD = {(19, 300): (8, 24, 16, 40), (65, 300): (40, 8, 24, 16), (96, 300): (16, 40, 8, 24), (33, 128): (24, 16, 40, 8)}
GRID_STRIDE_KP = (19, 131072 + 133)


def roundup(n, m):
    return (n + m - 1) // m * m


# ---- mirrors of the kernels' index arithmetic
def acc_row(mb, r, h):
    """csrc/ocr_attn.hip acc_row: the region held by accumulator register r of a lane in half h, m-block mb."""
    return mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h


def region_home(region):
    """(m-block, lane half) that hold `region`: the inverse of acc_row (asserted in test_ocr_cases_cpu)."""
    return region >> 5, (region >> 2) & 1


def attn_tiles(P):
    """(tiles of 128 pixels, workgroups) of csrc/ocr_attn.hip launch()."""
    tiles = (P + 127) // 128
    return tiles, min(tiles, 1024)


def stats_plan(HW, K):
    """(RP, pix_per_block, blocks) of ssa_softmax_hw_stats."""
    RP = 256 // K
    ppb = RP * 16
    blocks = (HW + ppb - 1) // ppb
    if blocks > 1024:
        blocks = 1024
        ppb = (HW + blocks - 1) // blocks
        blocks = (HW + ppb - 1) // ppb
    return RP, ppb, blocks


def step16(v):
    """One unit in the last place of the 16-bit storage format at |v| (float64 tensor)."""
    return 2.0 * half_ulp_act(v)


# ---- attention: the tie cases
def tie_groups(K, seed):
    """(group of every region [K], size of every group [G]): the sizes of GROUPS[K], members by a seeded permutation."""
    sizes = GROUPS[K]
    assert sum(sizes) == K and all(s & (s - 1) == 0 and 1 <= s <= 32 for s in sizes)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(seed))
    group = torch.empty(K, dtype=torch.long)
    at = 0
    for g, s in enumerate(sizes):
        group[perm[at:at + s]] = g
        at += s
    return group, torch.tensor(sizes, dtype=torch.long)


def tie_case(K, P, seed=0, backward=True):
    """Operands (integer-valued fp32) and references of a tie case.  backward False: q, out and the per-group tables only
    (`pixel_group` indexes them), for the grid-stride case."""
    group, sizes = tie_groups(K, 9100 + seed)
    G = len(sizes)
    Kp = roundup(K, 32)
    key = ints((G, D), -4, 4, 9200 + seed)
    # v = a per-channel offset of either sign plus a small per-region part: group means reach 64 and beyond, where
    # multiples of 1/32 need 12 significant bits (more than either storage format holds), while dprobs - <probs, dprobs>,
    # which only sees the per-region part, stays small enough for the premise of the pixel reduction dk
    off = ints((1, D), 64, 96, 9300 + seed) * (ints((1, D), 0, 1, 9301 + seed) * 2 - 1)
    v = off + ints((K, D), -8, 8, 9302 + seed)
    k = key[group]
    assert_integers("tie operands", key * 8, k, v)
    assert float(v.abs().max()) >= 100
    pg = torch.arange(P) % G                                     # g(p)
    m = sizes.double()

    # premises of the softmax, per (target group, region): P pixels share G rows
    key64, k64, v64 = key.double(), k.double(), v.double()
    assert_premise("tie sim", (8 * key64).abs() @ k64.abs().t())
    simG = (8 * key64) @ k64.t() * SCALE                          # [G, K]
    member = group[None, :] == torch.arange(G)[:, None]           # [G, K]
    top = simG.max(1).values
    assert bool((simG[member] == top[:, None].expand(G, K)[member]).all()), "sim is not tied inside the target group"
    assert bool((simG[~member] <= (top[:, None].expand(G, K) - SEPARATION)[~member]).all()), \
        "a region outside the target group is less than %g below the maximum" % SEPARATION
    probsG = member.double() / m[:, None]                         # [G, K]: exactly 1/m on the group
    assert_premise("tie out", (probsG @ v64.abs()) * 32)
    outG64 = probsG @ v64 + 0.0                                   # [G, D]
    # 64 <= |out| < 128 in multiples of 1/m takes 7 + log2(m) significant bits: more than the format's from m = 4 (bf16) or
    # m = 32 (fp16) on; below that every output is representable and only dsim, dq and dk see a rounding
    if int(sizes[pg.unique()].max()) > 2 ** (_MANT - 6):
        assert not_representable(outG64[pg.unique()]) > 0, "no output of this case needs the rounding to 16 bit"
    case = dict(K=K, P=P, Kp=Kp, G=G, group=group, sizes=sizes, pixel_group=pg, key=key, k=k, v=v, simG=simG,
                probsG=probsG, outG=to_act(outG64))
    if not backward:
        return case
    q = 8 * key[pg]
    dout = ints((P, D), -2, 2, 9400 + seed)
    assert_integers("tie operands", q, dout)
    q64, dout64 = q.double(), dout.double()
    probs = torch.zeros(P, Kp, dtype=torch.float64)
    probs[:, :K] = probsG[pg]
    mp = m[pg]                                                    # group size per pixel
    dp = torch.zeros(P, Kp, dtype=torch.float64)
    dp[:, :K] = dout64 @ v64.t() + 0.0                            # padding regions: v staged as zeros -> +0.0
    adp = dout64.abs() @ v64.abs().t()
    assert_premise("tie dprobs", adp)
    assert_premise("tie <probs, dprobs> and dprobs - dot, in units of 1/32", 2 * 32 * adp)
    dot = (probs * dp).sum(1, keepdim=True) + 0.0
    dsim64 = (SCALE * probs) * (dp - dot)                         # the kernels' factors, in their order
    dsim = to_act(dsim64)                                         # [P, Kp] 16 bit
    quantum = SCALE / (mp * mp)                                   # per pixel: dsim, rounded or not, is a multiple of it
    units = dsim.double() / quantum[:, None]
    assert torch.equal(units, units.round()), "dsim is not a multiple of 2^-4 / m^2"
    ds = dsim.double()[:, :K]
    assert_premise("tie dq", (ds.abs() @ k64.abs()) / quantum[:, None])
    dq64 = ds @ k64 + 0.0
    assert_premise("tie dv", (probs[:, :K].t() @ dout64.abs()) * 32)
    dv64 = probs[:, :K].t() @ dout64 + 0.0
    mr = m[group]                                                 # group size per region: only its group's pixels count
    assert_premise("tie dk", (ds.abs().t() @ q64.abs()) * (mr * mr / SCALE)[:, None])
    dk64 = ds.t() @ q64 + 0.0
    nz = dsim64 != 0
    case.update(q=q, dout=dout, probs=to_act(probs), dprobs=to_f32(dp[:, :K]), dsim=dsim, out=to_act(probs[:, :K] @ v64 + 0.0),
                dq=to_act(dq64), dv64=dv64, dk64=dk64, sim=to_f32(q64 @ k64.t() + 0.0),
                dsim_rounded=float((dsim.double() != dsim64)[nz].double().mean()) if bool(nz.any()) else 0.0)
    return case


def k1_real_case(P, seed=0):
    """One region and a real-valued q of large magnitude: probs = 1 whatever sim is (its values spread over about
    +-500, so the row maximum is negative for half the pixels), out = v[0] bit for bit, dsim = dq = +0.0."""
    g = torch.Generator().manual_seed(9500 + seed)
    q = bf16_round(torch.randn(P, D, generator=g) * 64)
    k = ints((1, D), -4, 4, 9501 + seed)
    v = bf16_round(torch.randn(1, D, generator=g) * 50)
    dout = ints((P, D), -2, 2, 9502 + seed)
    sim = (q.double() @ k.double().t()) * SCALE
    assert float(sim.min()) < -150 and float(sim.max()) > 150
    return dict(K=1, P=P, Kp=32, q=q, k=k, v=v, dout=dout, out=v.to(ACT_DTYPE).expand(P, D).contiguous(),
                dq=torch.zeros(P, D, dtype=ACT_DTYPE))


def bounded_case(K, P, seed=0):
    """Gaussian operands as in test_ocr_attention; the float64 reference rounds probs to 16 bit where the kernel does.
    Bounds (derived): a stored probability is computed in fp32 to a relative error orders of magnitude below half a
    16-bit step, so it is round16(p_ref) or its neighbour: one step at the larger of the two.  out sums K products of v
    with such probabilities in fp32 and is rounded once."""
    g = torch.Generator().manual_seed(9600 + seed)
    q, k, v, dout = (bf16_round(torch.randn(n, D, generator=g)) for n in (P, K, K, P))
    Kp = roundup(K, 32)
    q64, k64, v64 = q.double(), k.double(), v.double()
    p_ref = torch.softmax(q64 @ k64.t() * (D ** -0.5), dim=1)
    p16 = p_ref.float().to(ACT_DTYPE).double()
    probs = torch.zeros(P, Kp, dtype=torch.float64)
    probs[:, :K] = p16
    pbound = torch.zeros(P, Kp, dtype=torch.float64)              # padding columns: exactly 0
    pbound[:, :K] = torch.maximum(step16(p_ref), step16(p16))
    out = p16 @ v64
    a = step16(p_ref) @ v64.abs()
    b = 2.0 ** -20 * (p_ref @ v64.abs())
    obound = a + b + half_ulp_act(out.abs() + a + b)
    return dict(K=K, P=P, Kp=Kp, q=q, k=k, v=v, dout=dout, probs=probs, probs_bound=pbound, out=out, out_bound=obound)


# ---- HW softmax / spatial gather: the exact cases
TOPS = [-40.0, -17.0, -3.5, -0.0, 0.0, 2.25, 30.0]
SIZES = [1, 2, 4, 8, 16, 32]
# (id, K, H, W, C, ld - K of the logits)
GATHER = [("k1", 1, 4, 4, 64, 0), ("k19-3x5", 19, 3, 5, 64, 0), ("k19-13x21", 19, 13, 21, 64, 5), ("k65", 65, 13, 21, 64, 0),
          ("k150", 150, 7, 9, 64, 3), ("k256", 256, 5, 8, 64, 0), ("k19-c512", 19, 8, 9, 512, 0)]
GATHER_REBALANCE = ("k256-rebalance", 256, 1, 16515, 32, 0)


def _is_neg_zero(x):
    return x == 0.0 and str(float(x)).startswith("-")


def gather_logits(K, HW, seed=0):
    """logits [HW, K] fp32, the top pixels of every class and their count m [K]."""
    g = torch.Generator().manual_seed(9700 + seed)
    RP, ppb, blocks = stats_plan(HW, K)
    cap = max(s for s in SIZES if s <= max(1, HW // 2))
    logits = torch.empty(HW, K, dtype=torch.float64)
    tops, m, mode, names = [], torch.empty(K, dtype=torch.long), [], []
    for c in range(K):
        tv = TOPS[(c + 3 + seed) % len(TOPS)]
        mc = min(SIZES[c % len(SIZES)], cap)
        if tv == 0.0 and not _is_neg_zero(tv):
            mc = max(mc, 2)                                       # room for +0.0 and -0.0
        md = c % 4
        if md == 3 and mc >= 3:                                   # spread over the whole pixel range
            first = [int(round(i * (HW - 1) / (mc - 1))) for i in range(mc)]
        else:
            first = [[0], [HW - 1], [(blocks - 1) * ppb], [HW // 2]][md]
        first = torch.tensor(first, dtype=torch.long)
        perm = torch.randperm(HW, generator=g)
        rest = perm[~torch.isin(perm, first)]
        pix = torch.cat([first, rest[:mc - len(first)]]).sort().values
        assert len(pix) == mc
        base = 0.0 if tv == 0.0 else tv
        logits[:, c] = base - torch.randint(128, 178, (HW,), generator=g).double()
        logits[pix, c] = tv
        if tv == 0.0 and not _is_neg_zero(tv):
            logits[pix[1:], c] = -0.0
        tops.append(pix)
        m[c] = mc
        mode.append(md)
        names.append("-0.0" if _is_neg_zero(tv) else "%g" % tv)
    return logits.float(), tops, m, mode, names


def gather_case(K, HW, C, seed=0):
    logits, tops, m, mode, names = gather_logits(K, HW, seed)
    feats = ints((HW, C), -8, 8, 9800 + seed)
    dctx = ints((K, C), -4, 4, 9801 + seed)
    assert_integers("gather operands", feats, dctx)
    Kp = roundup(K, 32)
    l64 = logits.double()
    mx = l64.max(0).values
    is_top = l64 == mx[None, :]
    assert torch.equal(is_top.sum(0), m)
    for c in range(K):
        assert torch.equal(is_top[:, c].nonzero().flatten(), tops[c])
    low = mx[None, :] - l64
    assert bool(((low >= SEPARATION) & (low <= 177))[~is_top].all()), "a low pixel is not 128 to 177 below the top"
    sign = torch.signbit(l64)
    for c in range(K):
        if float(mx[c]) == 0.0 and bool(sign[tops[c], c].all()):                      # the -0.0 class
            assert bool((l64[~is_top[:, c], c] < 0).all())
        if float(mx[c]) == 0.0 and not bool(sign[tops[c], c].all()):                  # the +0.0 class
            assert bool(sign[tops[c], c].any()), "the +0.0 class has no -0.0 pixel"
    probs = is_top.double() / m.double()[None, :]                 # [HW, K]
    f64, d64 = feats.double(), dctx.double()
    assert_premise("gather ctx", (probs.t() @ f64.abs()) * 32)
    ctx64 = probs.t() @ f64 + 0.0                                 # [K, C]
    assert_premise("gather dfeats", (probs @ d64.abs()) * 32)
    dfeats64 = probs @ d64 + 0.0
    adp = f64.abs() @ d64.abs().t()
    assert_premise("gather dprobs", adp)
    dprobs64 = f64 @ d64.t() + 0.0                                # [HW, K]
    adot = (ctx64.abs() * d64.abs()).sum(1)
    assert_premise("gather row dot and dprobs - dot, in units of 1/32", (adp + adot[None, :]) * 32)
    dot64 = (ctx64 * d64).sum(1) + 0.0
    dlogits64 = probs * (dprobs64 - dot64[None, :])               # the kernel's factors: probs = +0.0 keeps the sign
    probs16 = torch.zeros(HW, Kp, dtype=torch.float64)
    probs16[:, :K] = probs
    rowstat = torch.stack([mx, m.double()], 1)
    return dict(K=K, HW=HW, C=C, Kp=Kp, logits=logits, feats=feats, dctx=dctx, tops=tops, m=m, mode=mode, top_names=names, probs64=probs,
                rowstat=to_f32(rowstat), probs=to_act(probs16), ctx=to_f32(ctx64), dfeats=to_act(dfeats64),
                dprobs=to_f32(dprobs64), dot=to_f32(dot64), dlogits=to_f32(dlogits64), plan=stats_plan(HW, K))


def blocks_of(case, c):
    """The workgroups of the stats plan that hold top pixels of class c."""
    ppb = case["plan"][1]
    return sorted(set(int(p) // ppb for p in case["tops"][c]))
