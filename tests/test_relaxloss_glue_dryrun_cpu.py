"""Dry run of the label relaxation's host glue (tests/test_hip_glue_dryrun_cpu.py's machinery: the real library, every
launching entry point replaced by a stand-in that checks the call against the ctypes signature of semseg_amd/_lib.py):
RelaxNllFn's launch budget -- forward four entry points (five launches: the first clears its counters by a launch of
its own, no memset), backward 1 --, no torch operator on a full-size tensor, no host read-back, and one training step of DeepV3PlusW38 with
the criterion."""
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from test_hip_glue_dryrun_cpu import DryLib, dry, _batch  # noqa: F401  (dry: the fixture)

RELAX = ("ssa_relax_mask_labels", "ssa_relax_mask_multihot", "ssa_relax_multihot", "ssa_relax_weights",
         "ssa_relax_nll_fwd", "ssa_relax_nll_finalize", "ssa_relax_nll_bwd")
# operators that compute nothing: allocation and views
FREE = {"empty", "empty_like", "empty_strided", "view", "_unsafe_view", "detach", "alias", "as_strided", "permute",
        "slice", "select", "unsqueeze", "squeeze", "expand", "t", "transpose", "reshape", "_reshape_alias"}


class Spy(TorchDispatchMode):
    def __init__(self, full):
        super().__init__()
        self.full, self.big, self.names = full, [], []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = func.__name__.split(".")[0]
        self.names.append(name)
        tensors = [a for a in list(args) + [out] if isinstance(a, torch.Tensor)]
        if name not in FREE and any(t.numel() >= self.full for t in tensors):
            self.big.append(name)
        return out


def _relax_calls(d):
    return {k: v for k, v in d.calls.items() if k in RELAX}


@pytest.mark.parametrize("target", ["int64", "uint8", "multihot"])
def test_launch_budget_and_no_full_size_torch_op(dry, target):
    from semseg_amd import hip_backend as hb
    B, H, W, C = 2, 24, 40, 19
    x = torch.randn(B, H, W, C).requires_grad_(True)
    up = torch.tensor(1.7)
    if target == "multihot":
        t = torch.zeros(B, C + 1, H, W, dtype=torch.uint8)
    else:
        t = torch.zeros(B, H, W, dtype=torch.int64 if target == "int64" else torch.uint8)
    first = "ssa_relax_mask_multihot" if target == "multihot" else "ssa_relax_mask_labels"
    with Spy(H * W) as spy:
        loss, sets, stats, w = hb.RelaxNllFn.apply(x, t, C, 255, 1, [3, 7], 1.0, False)
        assert _relax_calls(dry) == {first: 1, "ssa_relax_weights": 1, "ssa_relax_nll_fwd": 1, "ssa_relax_nll_finalize": 1}
        assert sum(dry.calls.values()) <= 5
        assert loss.dim() == 0 and loss.requires_grad and not sets.requires_grad
        assert tuple(sets.shape) == (B, H, W, 2) and tuple(stats.shape) == (B, C + 2) and tuple(w.shape) == (B, C)
        dry.calls.clear()
        loss.backward(up)
        assert dict(dry.calls) == {"ssa_relax_nll_bwd": 1}
    assert not spy.big, spy.big
    assert not {"item", "_local_scalar_dense", "_to_copy", "copy_"} & set(spy.names), spy.names
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == torch.float32


def test_strict_classes_as_bits():
    from semseg_amd.hip_backend import strict_bits
    assert strict_bits(None, 19) == (0, 0) and strict_bits([3, 7], 19) == ((1 << 3) | (1 << 7), 0)
    assert strict_bits([0, 64, 70, 200], 65) == (1, 1)          # the ignore channel and classes that do not exist drop out


def test_wrn38_training_step_with_the_criterion(dry):
    from semseg_amd.loss import ImgWtLossSoftNLL
    from semseg_amd.network import get_model
    net = get_model("deepv3.DeepV3PlusW38", 19, ImgWtLossSoftNLL(19, ignore_index=255)).train()
    inputs = _batch()                                       # 2 x 64 x 96, int64 label maps
    loss = net(inputs)
    assert loss.dim() == 0 and loss.requires_grad
    assert _relax_calls(dry) == {"ssa_relax_mask_labels": 1, "ssa_relax_weights": 1, "ssa_relax_nll_fwd": 1,
                                 "ssa_relax_nll_finalize": 1}
    assert dry.calls["ssa_ce_fwd"] == 0
    loss.backward()
    assert dry.calls["ssa_relax_nll_bwd"] == 1
    missing = [n for n, p in net.named_parameters() if p.grad is None]
    assert not missing, missing[:5]
