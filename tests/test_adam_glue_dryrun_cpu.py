"""Dry run of FusedAdam / FusedRAdam's host glue on CPU tensors (the pattern of tests/test_hip_glue_dryrun_cpu.py):
libsemseg_hip.so is loaded for real, ssa_adam_advance / ssa_adam_step / the loss-scaling entry points are replaced
by stand-ins that check every call against the ctypes signature declared in semseg_amd/_lib.py and return 0.  All
three modes, with and without a loss scaler: the order of the launches, the tables, the version counters."""
import collections
import contextlib
import ctypes

import pytest
import torch

LAUNCHING = ("ssa_adam_advance", "ssa_adam_step", "ssa_amp_check_grads", "ssa_amp_update_counted",
             "ssa_sgd_momentum_step")


class DryLib:
    def __init__(self, real):
        self._real = real
        self.calls = collections.Counter()
        self.order = []
        self.args = {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in LAUNCHING:
            return fn
        argtypes = fn.argtypes

        def launch(*args):
            assert len(args) == len(argtypes), "%s: %d arguments for %d parameters" % (name, len(args), len(argtypes))
            for i, (t, a) in enumerate(zip(argtypes, args)):
                try:
                    t.from_param(a)
                except (ctypes.ArgumentError, TypeError) as e:
                    raise AssertionError("%s: argument %d (%r) does not convert to %s: %s" % (name, i, a, t, e))
            self.calls[name] += 1
            self.order.append(name)
            self.args[name] = args
            return 0
        return launch


@pytest.fixture()
def dry(monkeypatch):
    from semseg_amd import _lib, hip_backend
    from semseg_amd.loss import optimizer as sopt
    d = DryLib(_lib.lib())
    monkeypatch.setattr(_lib, "_LIB", d)
    monkeypatch.setattr(sopt, "_on_gpu", lambda p: True)
    monkeypatch.setattr(sopt, "_launch_scope", lambda device: contextlib.nullcontext((None, False)))
    yield d
    hip_backend.enable_fp16_training(False)


def _make(kind, params):
    from semseg_amd.loss.optimizer import FusedAdam, FusedRAdam
    if kind == "radam":
        return FusedRAdam(params, lr=1e-3, weight_decay=1e-4), 2
    return FusedAdam(params, lr=1e-3, weight_decay=1e-4, amsgrad=kind == "amsgrad"), 1 if kind == "amsgrad" else 0


@pytest.mark.parametrize("scaler", [False, True], ids=["plain", "scaler"])
@pytest.mark.parametrize("kind", ["adam", "amsgrad", "radam"])
def test_adam_family_step_glue(dry, monkeypatch, kind, scaler):
    from semseg_amd import amp as samp
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))
    idle = list(net[2].parameters())                           # never get a gradient
    opt, mode = _make(kind, net.parameters())
    if scaler:
        monkeypatch.setattr(samp, "ACT", "fp16")                # (what SSA_ACT_DTYPE=fp16 makes of the process)
        assert samp.initialize(net, opt)[1] is opt and samp.scaler_of(opt) is None      # CPU module: no device to put it on
        sc = samp.attach_scaler(opt, torch.device("cpu"), init_scale=1024.0)
        assert samp.scaler_of(opt) is sc
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        x = torch.randn(4, 7)
        loss = net[1](net[0](x)).square().mean()
        with samp.scale_loss(loss, opt) as scaled:
            assert float(scaled.detach()) == float(loss.detach()) * (1024.0 if scaler else 1.0)
            scaled.backward()
        live = [p for p in net.parameters() if p.grad is not None]
        assert len(live) == 4
        versions = [p._version for p in live]
        dry.order.clear()
        opt.step()
        want = ["ssa_adam_advance", "ssa_adam_step"]
        if scaler:
            want = ["ssa_amp_check_grads"] + want + ["ssa_amp_update_counted"]
        assert dry.order == want
        assert all(p._version > v for p, v in zip(live, versions))
        adv, stp = dry.args["ssa_adam_advance"], dry.args["ssa_adam_step"]
        assert adv[1] == 4 and adv[2] == mode and (adv[3], adv[4]) == (0.9, 0.999)
        assert stp[7] == 4 and stp[8] == mode and (stp[4] is not None) == (kind == "amsgrad")
        assert (adv[5] is not None) == scaler and (stp[15] is not None) == scaler
        rec = opt._rec[torch.device("cpu")]
        assert list(stp[5]) == [rec.data_ptr() + 16 * i for i in range(4)] and list(adv[0]) == list(stp[5])
        assert list(stp[6]) == [p.numel() for p in live]
        assert list(stp[0]) == [p.data_ptr() for p in live] and list(stp[1]) == [p.grad.data_ptr() for p in live]
        assert list(stp[2]) == [opt.state[p]["exp_avg"].data_ptr() for p in live]
        assert list(stp[3]) == [opt.state[p]["exp_avg_sq"].data_ptr() for p in live]
    assert dry.calls["ssa_adam_step"] == 3 and dry.calls["ssa_sgd_momentum_step"] == 0
    names = {"exp_avg", "exp_avg_sq"} | ({"max_exp_avg_sq"} if kind == "amsgrad" else set())
    assert all(set(opt.state[p]) == names for p in live) and all(not opt.state.get(p) for p in idle)
    assert rec.shape == (6, 4) and rec.dtype == torch.int32 and rec.data_ptr() % 16 == 0
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2, 3] and ("loss_scaler" in sd) == scaler
    if scaler:
        sd["loss_scaler"] = {"loss_scale": 64.0, "unskipped": 3}
        opt.load_state_dict(sd)
        assert sc.state.tolist()[:3] == [64.0, 0.0, 3.0]


def test_snapshot_and_restore_put_the_state_back(dry):
    """What a graph capture relies on: warm-up steps leave no trace in the moment estimates or the step records; state
    that did not exist at the snapshot goes back to zeros and t = 0.  (The stand-ins launch nothing, so the test
    writes what a step would.)"""
    net = torch.nn.Linear(4, 3)
    opt, _ = _make("amsgrad", net.parameters())
    snap = opt.snapshot_state()
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    rec = opt._rec[torch.device("cpu")]
    rec[:, 0] = 2
    for p in net.parameters():
        opt.state[p]["exp_avg"].fill_(1.0)
    ptrs = [opt.state[p]["exp_avg"].data_ptr() for p in net.parameters()]
    opt.restore_state(snap)
    assert opt.step_counts() == [0, 0] and all(float(opt.state[p]["exp_avg"].abs().max()) == 0.0 for p in net.parameters())
    assert ptrs == [opt.state[p]["exp_avg"].data_ptr() for p in net.parameters()] and opt._rec[torch.device("cpu")] is rec
    rec[:, 0] = 5
    for p in net.parameters():
        opt.state[p]["exp_avg_sq"].fill_(3.0)
    snap = opt.snapshot_state()
    rec[:, 0] = 7
    for p in net.parameters():
        opt.state[p]["exp_avg_sq"].fill_(4.0)
    opt.restore_state(snap)
    assert opt.step_counts() == [5, 5] and all(float(opt.state[p]["exp_avg_sq"].min()) == 3.0 for p in net.parameters())
