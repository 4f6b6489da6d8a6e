"""What hoisting the coefficient loads of the BatchNorm passes (csrc/bn.hip: ssa_bn_apply_train, ssa_bn_bwd_apply) in front
of the data loads can newly break -- the single-launch exact tests of test_kernels_gpu.py pin the arithmetic on every
grid regime; here:
  * a grouped launch equals its problems launched one by one, BIT FOR BIT, over mixed C / P / nrep / flags: a hoisted
    load that takes another problem's pointer, C or nrep shows;
  * the statistics and per-channel operands sit in guard-banded buffers of exactly nrep * 2 * C / C elements (the guard is
    NaN: a stray read poisons the result, which must stay finite) at C = 264, where only 8 threads have a second
    channel, and at C = 8, P = 3, where most threads have no row but still reach the barrier;
  * the once-per-launch side effects: two passes over one layer in a step advance num_batches_tracked by exactly 2 and
    leave the chained running statistics of the reference."""
import pytest
import torch

from exact_util import assert_bits_equal, assert_guard_intact, guarded, guarded_copy, split_replicas_real
from util import bf16_round, check_close, nhwc, ACT_DTYPE

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (C, P) of the issue: one workgroup with P < RP; 252 of 256 threads active; C > 256 with 8 threads on a second channel;
# C > 256 with half a second trip; three trips with idle threads (180 active)
PROBLEMS = [(8, 3), (48, 198), (264, 37), (384, 70), (720, 301)]


def _hb():
    from semseg_amd import hip_backend
    return hip_backend


def _check():
    from semseg_amd._lib import check
    return check


def _rand(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + shift


def _pp(g):
    return _hb()._p(g.view) if g is not None else None


def _reps():
    return (1, _hb().stat_replicas(), 11)


# ---- ssa_bn_apply_train
def _train_problem(i, C, P, nrep, res, relu, post, mask, track):
    """Host-side operands of one training apply: real-valued data, its own fp64 statistics split over nrep replicas."""
    d = dict(C=C, P=P, nrep=nrep, res=res, relu=relu, post=post, mask=mask, track=track)
    d["x"] = bf16_round(_rand((P, C), 900 + i, 1.7, 0.3)).to(ACT_DTYPE)
    d["r"] = _rand((P, C), 910 + i).to(ACT_DTYPE)
    xd = d["x"].double()
    d["sums"], _ = split_replicas_real(torch.stack([xd.sum(0), (xd * xd).sum(0)]), nrep, 920 + i)
    d["gamma"] = _rand((C,), 930 + i, 0.3, 1.0)
    d["beta"] = _rand((C,), 940 + i, 0.3)
    d["rm"], d["rv"] = _rand((C,), 950 + i, 0.2), _rand((C,), 960 + i).abs() + 0.5
    d["pm"] = (torch.rand(1, C, generator=torch.Generator().manual_seed(970 + i)) > 0.3).float() * 2.0
    return d


def _train_buffers(d):
    C, P = d["C"], d["P"]
    return dict(x=guarded_copy(d["x"], DEV), r=guarded_copy(d["r"], DEV) if d["res"] else None,
                z=guarded((P, C), ACT_DTYPE, DEV), sums=guarded_copy(d["sums"], DEV),
                gamma=guarded_copy(d["gamma"], DEV), beta=guarded_copy(d["beta"], DEV),
                pm=guarded_copy(d["pm"], DEV) if d["post"] else None, coef=guarded((4, C), torch.float32, DEV),
                mask=guarded((P, C // 8), torch.uint8, DEV) if d["mask"] else None,
                rm=guarded_copy(d["rm"], DEV) if d["track"] else None, rv=guarded_copy(d["rv"], DEV) if d["track"] else None,
                ps=guarded((2 * C + 1,), torch.float32, DEV) if d["track"] else None,
                nbt=guarded_copy(torch.tensor([7], dtype=torch.int64), DEV) if d["track"] else None)


def _train_launch(d, b):
    hb = _hb()
    C, P = d["C"], d["P"]
    _check()(hb.lib().ssa_bn_apply_train(hb._p(b["x"].view), C, _pp(b["r"]), C if d["res"] else 0, hb._p(b["z"].view), C, P, C,
                                         hb._p(b["sums"].view), d["nrep"], float(P), hb._p(b["gamma"].view),
                                         hb._p(b["beta"].view), _pp(b["rm"]), _pp(b["rv"]), _pp(b["nbt"]), 0.1, 1e-5,
                                         hb._p(b["coef"].view), _pp(b["ps"]), int(d["relu"]), _pp(b["pm"]), P, _pp(b["mask"]),
                                         hb._s()), "ssa_bn_apply_train")


_TRAIN_OUT = ("z", "mask", "coef", "rm", "rv", "ps", "nbt")


def _train_mix():
    reps = _reps()
    probs = []
    for i, (C, P) in enumerate(PROBLEMS):
        # residual and sign mask on every second problem, ReLU off on one, post on two, the side effects off on one
        probs.append(_train_problem(i, C, P, reps[i % 3], res=i % 2 == 0, relu=i != 3, post=i in (1, 4),
                                    mask=i % 2 == 0 and i != 3, track=i != 1))
    return probs


def test_bn_apply_train_grouped_equals_single():
    hb = _hb()
    probs = _train_mix()
    single = []
    for d in probs:
        b = _train_buffers(d)
        _train_launch(d, b)
        single.append(b)
    torch.cuda.synchronize()
    grouped = [_train_buffers(d) for d in probs]
    with hb.group():
        for d, b in zip(probs, grouped):
            _train_launch(d, b)
    torch.cuda.synchronize()
    for d, s, g in zip(probs, single, grouped):
        tag = "bn_apply_train grouped C=%d P=%d nrep=%d res=%d relu=%d post=%d" % (d["C"], d["P"], d["nrep"], d["res"], d["relu"], d["post"])
        assert bool(torch.isfinite(s["z"].view.float()).all()) and bool(torch.isfinite(s["coef"].view).all()), tag
        for k in _TRAIN_OUT:
            if s[k] is not None:
                assert_bits_equal("%s: %s" % (tag, k), g[k].view.cpu(), s[k].view.cpu())
        if d["track"]:
            assert int(s["nbt"].view) == 8 and int(g["nbt"].view) == 8, tag
        assert_guard_intact(tag, *[v for v in list(s.values()) + list(g.values()) if v is not None])


# ---- ssa_bn_bwd_apply
_MODES = ("bits", "x", "z", "norelu")


def _bwd_problem(i, C, P, nrep, mode, dres, gamma, pg):
    d = dict(C=C, P=P, nrep=nrep, mode=mode, dres=dres, has_gamma=gamma, pg=pg)
    d["x"] = bf16_round(_rand((P, C), 1000 + i, 1.5)).to(ACT_DTYPE)
    d["dz"] = bf16_round(_rand((P, C), 1010 + i)).to(ACT_DTYPE)
    d["z"] = bf16_round(_rand((P, C), 1020 + i)).to(ACT_DTYPE)
    d["bits"] = torch.randint(0, 256, (P, C // 8), generator=torch.Generator().manual_seed(1030 + i)).to(torch.uint8)
    d["mean"], d["invstd"] = _rand((C,), 1040 + i, 0.3), _rand((C,), 1050 + i).abs() + 0.5
    d["gamma"] = _rand((C,), 1060 + i, 0.3, 1.0)
    d["msc"], d["msh"] = _rand((C,), 1070 + i), _rand((C,), 1080 + i, 0.5)
    g = torch.Generator().manual_seed(1090 + i)
    d["sums"] = (torch.rand(nrep, 2, C, generator=g, dtype=torch.float64) - 0.5) * 40.0
    d["pre"] = _rand((2, C), 1100 + i, 3.0)
    return d


def _bwd_buffers(d):
    C, P, mode = d["C"], d["P"], d["mode"]
    b = dict(x=guarded_copy(d["x"], DEV), dz=guarded_copy(d["dz"], DEV), z=guarded_copy(d["z"], DEV) if mode == "z" else None,
             bits=guarded_copy(d["bits"], DEV) if mode == "bits" else None,
             mean=guarded_copy(d["mean"], DEV), invstd=guarded_copy(d["invstd"], DEV),
             gamma=guarded_copy(d["gamma"], DEV) if d["has_gamma"] else None,
             msc=guarded_copy(d["msc"], DEV) if mode == "x" else None, msh=guarded_copy(d["msh"], DEV) if mode == "x" else None,
             sums=guarded_copy(d["sums"], DEV), dx=guarded((P, C), ACT_DTYPE, DEV),
             dres=guarded((P, C), ACT_DTYPE, DEV) if d["dres"] else None,
             pg=guarded((2, C), torch.float32, DEV) if d["pg"] != "null" else None)
    if d["pg"] == "acc":
        b["pg"].view.copy_(d["pre"])
    return b


def _bwd_launch(d, b):
    hb = _hb()
    C, P, mode = d["C"], d["P"], d["mode"]
    pg = b["pg"]
    _check()(hb.lib().ssa_bn_bwd_apply(hb._p(b["x"].view), C, hb._p(b["dz"].view), C, _pp(b["z"]), C if b["z"] else 0,
                                       hb._p(b["dx"].view), C, _pp(b["dres"]), C if b["dres"] else 0, P, C, _pp(b["gamma"]),
                                       hb._p(b["mean"].view), hb._p(b["invstd"].view), hb._p(b["sums"].view), d["nrep"],
                                       float(P), int(mode != "norelu"), None, P, hb._p(pg.view[0]) if pg else None,
                                       hb._p(pg.view[1]) if pg else None, 0.5, _pp(b["msc"]), _pp(b["msh"]),
                                       int(d["pg"] == "acc"), _pp(b["bits"]), hb._s()), "ssa_bn_bwd_apply")


@pytest.mark.parametrize("mode", _MODES)
def test_bn_bwd_apply_grouped_equals_single(mode):
    hb = _hb()
    reps = _reps()
    # the store and the accumulate form of the parameter gradients in ONE bracket, and one problem without them
    probs = [_bwd_problem(10 * _MODES.index(mode) + i, C, P, reps[(i + 1) % 3], mode, dres=i % 2 == 0, gamma=i != 2,
                          pg=("write", "acc", "acc", "write", "null")[i]) for i, (C, P) in enumerate(PROBLEMS)]
    single = []
    for d in probs:
        b = _bwd_buffers(d)
        _bwd_launch(d, b)
        single.append(b)
    torch.cuda.synchronize()
    grouped = [_bwd_buffers(d) for d in probs]
    with hb.group():
        for d, b in zip(probs, grouped):
            _bwd_launch(d, b)
    torch.cuda.synchronize()
    for d, s, g in zip(probs, single, grouped):
        tag = "bn_bwd_apply grouped mode=%s C=%d P=%d nrep=%d pg=%s" % (mode, d["C"], d["P"], d["nrep"], d["pg"])
        assert bool(torch.isfinite(s["dx"].view.float()).all()), tag
        for k in ("dx", "dres", "pg"):
            if s[k] is not None:
                assert_bits_equal("%s: %s" % (tag, k), g[k].view.cpu(), s[k].view.cpu())
        if d["pg"] != "null":       # one add (or one store) per launch: s * param_grad_scale on the pre-fill, [0] dgamma, [1] dbeta
            want = torch.stack([d["sums"][:, 1].sum(0), d["sums"][:, 0].sum(0)]) * 0.5 + (d["pre"].double() if d["pg"] == "acc" else 0.0)
            check_close(tag + " parameter gradients", s["pg"].view.cpu(), want.float(), 1e-5, 1e-5)
        assert_guard_intact(tag, *[v for v in list(s.values()) + list(g.values()) if v is not None])


# ---- no read outside the operands
@pytest.mark.parametrize("C,P", [(264, 37), (8, 3)])
@pytest.mark.parametrize("nrep_i", [0, 1, 2])
def test_bn_prologue_reads_stay_inside(C, P, nrep_i):
    """sums [nrep][2][C] and gamma / beta / mean / invstd / mask scale / shift [C] in buffers of exactly that size between
    NaN guards (exact_util.guarded): the eight unconditional replica loads, the stand-in loads of a null operand and the
    loads of the threads past C stay inside; every output is finite and every guard intact."""
    nrep = _reps()[nrep_i]
    for res in (False, True):
        d = _train_problem(50 + nrep_i, C, P, nrep, res=res, relu=True, post=False, mask=res, track=True)
        b = _train_buffers(d)
        assert b["sums"].view.numel() == nrep * 2 * C and b["gamma"].view.numel() == C and b["beta"].view.numel() == C
        _train_launch(d, b)
        torch.cuda.synchronize()
        tag = "bn_apply_train guards C=%d P=%d nrep=%d res=%d" % (C, P, nrep, res)
        for k in ("z", "coef", "rm", "rv", "ps"):
            assert bool(torch.isfinite(b[k].view.float()).all()), "%s: %s is not finite" % (tag, k)
        assert int(b["nbt"].view) == 8, tag
        assert_guard_intact(tag, *[v for v in b.values() if v is not None])
    for i, mode in enumerate(_MODES):
        d = _bwd_problem(60 + 4 * nrep_i + i, C, P, nrep, mode, dres=True, gamma=i % 2 == 0, pg="write")
        b = _bwd_buffers(d)
        assert b["sums"].view.numel() == nrep * 2 * C and b["mean"].view.numel() == C and b["invstd"].view.numel() == C
        _bwd_launch(d, b)
        torch.cuda.synchronize()
        tag = "bn_bwd_apply guards mode=%s C=%d P=%d nrep=%d" % (mode, C, P, nrep)
        for k in ("dx", "dres", "pg"):
            assert bool(torch.isfinite(b[k].view.float()).all()), "%s: %s is not finite" % (tag, k)
        assert_guard_intact(tag, *[v for v in b.values() if v is not None])


# ---- once-per-launch side effects
@pytest.mark.parametrize("C", [48, 264])
def test_bn_two_passes_side_effects_once_per_launch(C):
    """Two training passes over one layer in one step (problems of one grouped launch), as in
    test_bn_deferred_running_stats_two_passes: num_batches_tracked advances by exactly 2 and the running statistics are the
    reference's two sequential in-place updates, in issue order.  C = 264: channels 256.. belong to the second trip.
    This goes through batch_norm_act, i.e. the DEFERRED update: what it pins of the apply kernel is block 0's pass_stats
    (mean, biased variance, count: written once per launch, for every channel of every trip) and of
    bn_update_running_kernel the chaining -- not the kernel's own read-modify-write of running_mean / running_var and
    num_batches_tracked, which test_exact_bn_apply_train checks against float64 and the grouped-equals-single test and the
    guard test above (num_batches_tracked 7 -> 8 exactly) run with the pointers given."""
    from oracle import ops as O
    from semseg_amd import ops, nn as snn
    hb = _hb()
    bn = snn.BatchNorm2d(C, momentum=0.1)
    rm, rv = _rand((C,), 1200, 0.1), _rand((C,), 1201).abs() + 0.5
    with torch.no_grad():
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
        bn.num_batches_tracked.fill_(3)
    xa, xb = bf16_round(_rand((1, C, 6, 10), 1202)), bf16_round(_rand((2, C, 12, 20), 1203, 2.0, 0.5))
    one, zero = torch.ones(C), torch.zeros(C)
    O.batch_norm(xa, one, zero, rm, rv, True, 0.1, 1e-5)
    O.batch_norm(xb, one, zero, rm, rv, True, 0.1, 1e-5)
    bn = bn.to(DEV).train()
    be = ops.HipBackend()
    hb.begin_step(torch.device(DEV))
    be.batch_norm_act([nhwc(xa).to(DEV).to(ACT_DTYPE), nhwc(xb).to(DEV).to(ACT_DTYPE)], bn)
    be.end_forward()
    torch.cuda.synchronize()
    assert int(bn.num_batches_tracked) == 5
    check_close("running_mean after two passes", bn.running_mean, rm, 1e-4, 1e-4)
    check_close("running_var after two passes", bn.running_var, rv, 1e-4, 1e-4)
