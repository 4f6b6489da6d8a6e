"""The hipGraph proxies of semseg_amd.graphed are transparent to the module tree (round-3 advisor finding): a state_dict
taken through an outer data-parallel wrapper loads back through it -- what the reference's restore_net ->
forgiving_state_restore(net, ...) does with --snapshot / --resume (train.py:396) -- and the guards of the stepper
(graph cap, invalidation on optimizer reload) behave.  No GPU: the stepper is never asked to capture."""
import torch
from torch import nn

from semseg_amd import graphed
from semseg_amd.loss.optimizer import forgiving_state_restore
from semseg_amd.parallel import DistributedDataParallel


def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.Sequential(nn.Conv2d(4, 2, 1)))


def test_state_dict_round_trip_through_an_outer_wrapper():
    net = _net()
    optim = torch.optim.SGD(net.parameters(), lr=0.1, momentum=0.9)
    gnet, goptim = graphed.graph_training(net, optim)
    assert list(gnet.state_dict().keys()) == list(net.state_dict().keys())
    assert [n for n, _ in gnet.named_parameters()] == [n for n, _ in net.named_parameters()]
    wrapped = DistributedDataParallel(gnet)
    sd = wrapped.state_dict()
    assert all(k.startswith("module.") and not k.startswith("module.wrapped.") for k in sd), list(sd)[:3]
    assert [k[len("module."):] for k in sd] == list(net.state_dict().keys())
    # perturb, then restore the way the reference does
    saved = {k: v.clone() for k, v in sd.items()}
    with torch.no_grad():
        for p in net.parameters():
            p.add_(1.0)
    forgiving_state_restore(wrapped, saved)
    for k, v in wrapped.state_dict().items():
        assert torch.equal(v, saved[k]), k
    wrapped.load_state_dict(saved)                      # strict loading too
    # train / eval reach the wrapped net
    wrapped.eval()
    assert not net.training and not net[1].training
    wrapped.train()
    assert net.training and net[1].training
    # evaluation goes straight to the module
    x = torch.randn(1, 3, 8, 8)
    wrapped.eval()
    with torch.no_grad():
        assert torch.equal(wrapped(x), net(x))


def test_optimizer_reload_invalidates_the_graphs_and_the_cap_holds():
    net = _net()
    optim = torch.optim.SGD(net.parameters(), lr=0.1, momentum=0.9)
    gnet, goptim = graphed.graph_training(net, optim, max_graphs=2)
    st = gnet._stepper
    st._graphs = {"a": object(), "b": object()}
    # a third signature would exceed the cap: the stepper runs the step eagerly instead of capturing
    called = []
    st._run_eager = lambda inputs: called.append(1) or torch.zeros(())
    st._capture = lambda inputs: (_ for _ in ()).throw(AssertionError("must not capture"))
    st({"images": torch.zeros(1, 3, 8, 8)})
    assert called == [1]
    goptim.load_state_dict(optim.state_dict())
    assert st._graphs == {}
    # the optimizer proxy forwards everything else
    assert goptim.param_groups is optim.param_groups
    goptim.zero_grad()
    goptim.step()


def test_evaluation_proxy_routes_and_evicts_least_recently_used(monkeypatch):
    """graph_eval / the evaluation half of graph_training without a GPU: CPU inputs and grad-enabled calls go straight to
    the module; the signature cache is LRU (capture stubbed: the bookkeeping around it is what runs here); a capture
    that raises switches evaluation to eager launches for good; SSA_GRAPHED_EVAL=0 installs no evaluation stepper."""
    net = _net().eval()
    g = graphed.graph_eval(net, max_graphs=2, capture_after=1)
    ev = g._eval_stepper
    assert isinstance(ev, graphed.GraphedEval) and g._stepper is None
    x = torch.randn(1, 3, 8, 8)
    with torch.no_grad():
        assert torch.equal(g(x), net(x))                      # not a dict of device tensors: the module itself
    assert ev.captures == 0
    # the stepper's cache, with the capture and the replay stubbed
    class _G:
        def __init__(self):
            self.n = 0

        def replay(self):
            self.n += 1
    made = []

    def fake_capture(inputs):
        gr = _G()
        made.append(gr)
        return gr, {k: v.clone() for k, v in inputs.items()}, {"pred": torch.zeros(1)}
    ev._capture = fake_capture
    from semseg_amd import hip_backend
    monkeypatch.setattr(hip_backend, "refresh_packed_filters", lambda: None)
    a, b, c = ({"images": torch.zeros(1, 3, s, s)} for s in (8, 9, 10))
    for inp in (a, b, a, c, b):
        out = ev(inp)
        assert set(out) == {"pred"}
    # a, b captured; a replayed (now most recent); c evicts b; b comes back and evicts a
    assert (ev.captures, ev.evictions, ev.replays) == (4, 2, 5)
    assert [k[0][1] for k in ev._graphs] == [(1, 3, 10, 10), (1, 3, 9, 9)]
    # the default policy: a signature is captured when it comes the second time -- sizes that never repeat stay eager
    ev3 = graphed.GraphedEval(net, max_graphs=2)
    ev3._capture = fake_capture
    calls = []
    ev3._forward = lambda inputs: calls.append(tuple(inputs["images"].shape)) or {"pred": torch.ones(1)}
    for s_ in (8, 9, 10, 11, 9, 9):
        ev3({"images": torch.zeros(1, 3, s_, s_)})
    assert (ev3.captures, ev3.eager_calls, ev3.replays) == (1, 4, 2) and len(calls) == 4
    # a capture that raises: eager from then on
    ev2 = graphed.GraphedEval(net, max_graphs=1, capture_after=1)
    ev2._capture = lambda inputs: (_ for _ in ()).throw(RuntimeError("no device"))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    net_calls = []
    ev2._forward = lambda inputs: net_calls.append(1) or {"pred": torch.ones(1)}
    ev2({"images": torch.zeros(1, 3, 8, 8)})
    ev2({"images": torch.zeros(1, 3, 8, 8)})
    assert ev2.eager_only and net_calls == [1, 1] and ev2.captures == 0
    # the switch
    monkeypatch.setenv("SSA_GRAPHED_EVAL", "0")
    assert graphed.graph_eval(net)._eval_stepper is None
    optim = torch.optim.SGD(net.parameters(), lr=0.1)
    assert graphed.graph_training(net, optim)[0]._eval_stepper is None
