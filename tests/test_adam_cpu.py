"""`--optimizer adam | adam --amsgrad | radam` of the product's get_optimizer without a GPU: the classes it returns,
the LR sequences of the reference (tests/golden/adam_golden.json), state_dict round trips with the optimizers the
fused classes replace (torch.optim.Adam; the reference's RAdam, whose state layout and types are recorded in the
golden), what is refused, and no fallback for CPU parameters."""
import argparse
import copy

import pytest
import torch

from adam_util import SHAPES, case_id, golden


def _args(c, **over):
    c = dict(c, **over)
    return argparse.Namespace(momentum=0.9, **c)


def _net():
    return torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))


@pytest.mark.parametrize("case", golden(), ids=case_id)
def test_get_optimizer_classes_and_lr_sequences(case):
    from semseg_amd.loss.optimizer import FusedAdam, FusedRAdam, get_optimizer
    c = case["case"]
    opt, sch = get_optimizer(_args(c), _net())
    if c["optimizer"] == "radam":
        assert type(opt) is FusedRAdam and case["optimizer_class"] == "RAdam"
    else:
        assert type(opt) is FusedAdam and case["optimizer_class"] == "Adam"
        assert opt.param_groups[0]["amsgrad"] is c["amsgrad"]
    g = opt.param_groups[0]
    assert g["weight_decay"] == c["weight_decay"] and list(g["betas"]) == case["betas"] and g["eps"] == case["eps"]
    for epoch, lr in enumerate(case["lrs"]):
        assert abs(opt.param_groups[-1]["lr"] - lr) <= 1e-15 + 1e-12 * abs(lr), epoch
        opt._step_count = 1          # silence LambdaLR's "step order" warning: no GPU step here
        sch.step()


def test_get_optimizer_still_refuses_what_the_reference_refuses():
    from semseg_amd.loss.optimizer import FusedSGD, get_optimizer
    c = golden()[0]["case"]
    with pytest.raises(ValueError):
        get_optimizer(_args(c, optimizer="lamb"), _net())
    assert type(get_optimizer(_args(c, optimizer="sgd"), _net())[0]) is FusedSGD


@pytest.mark.parametrize("amsgrad", [False, True])
def test_state_dict_round_trip_with_torch_adam(amsgrad):
    """torch.optim.Adam -> FusedAdam -> torch.optim.Adam: the restored optimizer goes on exactly as the original."""
    from semseg_amd.loss.optimizer import FusedAdam
    torch.manual_seed(0)
    net = _net()
    ref = torch.optim.Adam(net.parameters(), lr=0.01, weight_decay=1e-4, amsgrad=amsgrad)
    for _ in range(3):
        for p in net.parameters():
            p.grad = torch.randn_like(p)
        ref.step()
    mine = FusedAdam(net.parameters(), lr=0.5, amsgrad=amsgrad)
    mine.load_state_dict(copy.deepcopy(ref.state_dict()))     # (load_state_dict adopts fp32 tensors as they are)
    assert mine.param_groups[0]["lr"] == 0.01 and mine.param_groups[0]["weight_decay"] == 1e-4
    assert mine.step_counts() == [3, 3, 3, 3]
    names = ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if amsgrad else ())
    for p in net.parameters():
        assert set(mine.state[p]) == set(names)              # the step count lives in the device record
        assert all(torch.equal(mine.state[p][k], ref.state[p][k]) for k in names)
    sd = mine.state_dict()
    want = ref.state_dict()
    assert sorted(sd["state"]) == sorted(want["state"])
    for i, st in sd["state"].items():
        assert list(st) == list(want["state"][i])            # torch's keys, in torch's order
        assert torch.is_tensor(st["step"]) and st["step"].dtype == want["state"][i]["step"].dtype
        assert st["step"].shape == want["state"][i]["step"].shape and float(st["step"]) == 3.0
    twin = _net()
    twin.load_state_dict(net.state_dict())
    back = torch.optim.Adam(twin.parameters(), lr=0.7)
    back.load_state_dict(copy.deepcopy(sd))
    assert back.param_groups[0]["lr"] == 0.01 and back.param_groups[0]["amsgrad"] is amsgrad
    for p, q in zip(net.parameters(), twin.parameters()):
        p.grad = torch.randn_like(p)
        q.grad = p.grad.clone()
    ref.step()
    back.step()
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), twin.parameters()))


@pytest.mark.parametrize("case", [c for c in golden() if c["case"]["optimizer"] == "radam"], ids=case_id)
def test_state_dict_round_trip_with_the_references_radam(case):
    """The reference's RAdam state as recorded after 12 steps (int 'step', 'exp_avg', 'exp_avg_sq'; groups of lr,
    betas, eps, weight_decay) -> FusedRAdam -> back: same key set, same types, same values."""
    from semseg_amd.loss.optimizer import FusedRAdam
    assert case["state_keys"] == ["step", "exp_avg", "exp_avg_sq"] and case["state"][0]["step_type"] == "int"
    c = case["case"]
    group = dict(lr=case["lrs"][-1], betas=tuple(case["betas"]), eps=case["eps"], weight_decay=c["weight_decay"],
                 initial_lr=c["lr"], params=[0, 1, 2, 3])
    assert sorted(k for k in group if k != "params") == case["group_keys"]
    state = {i: {"step": int(st["step"]),
                 "exp_avg": torch.tensor(st["exp_avg"], dtype=torch.float32).reshape(SHAPES[i]),
                 "exp_avg_sq": torch.tensor(st["exp_avg_sq"], dtype=torch.float32).reshape(SHAPES[i])}
             for i, st in enumerate(case["state"])}
    mine = FusedRAdam(_net().parameters(), lr=0.3)
    mine.load_state_dict({"state": state, "param_groups": [group]})
    assert mine.step_counts() == [12] * 4 and mine.param_groups[0]["lr"] == case["lrs"][-1]
    sd = mine.state_dict()
    assert sorted(k for k in sd["param_groups"][0] if k != "params") == case["group_keys"]
    assert not hasattr(mine, "buffer")                       # the reference's memo is no state
    for i, st in sd["state"].items():
        assert list(st) == case["state_keys"]
        assert type(st["step"]) is int and st["step"] == 12
        assert torch.equal(st["exp_avg"], state[i]["exp_avg"]) and torch.equal(st["exp_avg_sq"], state[i]["exp_avg_sq"])
    again = FusedRAdam(_net().parameters())
    again.load_state_dict(sd)
    assert again.step_counts() == [12] * 4


def test_a_parameter_without_state_stays_without():
    from semseg_amd.loss.optimizer import FusedAdam
    net = _net()
    ref = torch.optim.Adam(net.parameters(), lr=0.01)
    for p in list(net.parameters())[:2]:
        p.grad = torch.ones_like(p)
    ref.step()
    mine = FusedAdam(net.parameters())
    mine.load_state_dict(ref.state_dict())
    assert mine.step_counts() == [1, 1, 0, 0]
    assert sorted(mine.state_dict()["state"]) == [0, 1]


@pytest.mark.parametrize("bad", [dict(maximize=True), dict(decoupled_weight_decay=True), dict(capturable=True),
                                 dict(foreach=True), dict(fused=True), dict(differentiable=True),
                                 dict(lr=torch.tensor(1e-3)), dict(lr=-1.0), dict(betas=(0.9, 1.0)), dict(eps=-1.0),
                                 dict(weight_decay=-1.0)], ids=lambda d: next(iter(d)))
def test_refused_arguments(bad):
    from semseg_amd.loss.optimizer import FusedAdam, FusedRAdam
    for cls in (FusedAdam, FusedRAdam):
        with pytest.raises(ValueError):
            cls(_net().parameters(), **bad)
    with pytest.raises(TypeError):
        FusedRAdam(_net().parameters(), amsgrad=True)
    if "lr" not in bad and "betas" not in bad and "eps" not in bad and "weight_decay" not in bad:
        ref = torch.optim.Adam(_net().parameters(), lr=0.01)
        sd = ref.state_dict()
        sd["param_groups"][0].update(bad)
        with pytest.raises(ValueError):                      # ... also when it comes in through a checkpoint
            FusedAdam(_net().parameters()).load_state_dict(sd)


def test_cpu_parameters_raise_instead_of_falling_back():
    from semseg_amd.loss.optimizer import FusedAdam, FusedRAdam
    for cls in (FusedAdam, FusedRAdam):
        net = _net()
        opt = cls(net.parameters())
        for p in net.parameters():
            p.grad = torch.ones_like(p)
        before = [p.detach().clone() for p in net.parameters()]
        with pytest.raises(RuntimeError):
            opt.step()
        assert all(torch.equal(p, q) for p, q in zip(net.parameters(), before))
