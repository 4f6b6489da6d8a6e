"""Golden Adam / AMSGrad / RAdam trajectories from the REAL reference's
loss/optimizer.py:get_optimizer (`--optimizer adam [--amsgrad] | radam` + LambdaLR).  Run in the build container:
    python tests/golden/make_golden_adam.py
Writes adam_golden.json: per case the learning rates, the initial parameters, the seeded gradients (their scale
jumps by 100x every three steps, up and down, so AMSGrad's running maximum matters), the parameters after every
step and the optimizer's final state (step counts as the reference holds them, moment estimates, key sets)."""
import argparse
import json
import os
import sys
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_bootstrap import bootstrap  # noqa: E402

STEPS = 12
SCHEDULE = dict(lr_schedule="poly", lr=0.01, max_epoch=14, poly_exp=2.0, poly_step=110, rescale=1.0, repoly=1.5)
CASES = (
    dict(optimizer="adam", amsgrad=False, weight_decay=1e-4),
    dict(optimizer="adam", amsgrad=True, weight_decay=1e-4),
    dict(optimizer="radam", amsgrad=False, weight_decay=1e-4),
    dict(optimizer="adam", amsgrad=True, weight_decay=0.0),
    dict(optimizer="radam", amsgrad=False, weight_decay=0.0),
)


def grad_scale(step):
    return 0.01 * (100.0 if (step // 3) % 2 else 1.0)


def _net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))


def main():
    cfg = bootstrap(19)
    cfg.REDUCE_BORDER_EPOCH = -1
    from loss.optimizer import get_optimizer
    warnings.filterwarnings("ignore", category=UserWarning)      # loss/radam.py uses the deprecated add_ / addcmul_ overloads
    out = []
    for c in CASES:
        args = argparse.Namespace(momentum=0.9, **c, **SCHEDULE)
        net = _net()
        opt, sch = get_optimizer(args, net)
        params = list(net.parameters())
        init = [p.detach().flatten().tolist() for p in params]
        lrs, grads, traj = [], [], []
        g = torch.Generator().manual_seed(9)
        for epoch in range(SCHEDULE["max_epoch"]):
            lrs.append(opt.param_groups[-1]["lr"])
            if epoch < STEPS:            # one step per epoch: the learning rate changes every step
                for p in params:
                    p.grad = torch.randn(p.shape, generator=g) * grad_scale(epoch)
                grads.append([p.grad.flatten().tolist() for p in params])
                opt.step()
                traj.append([p.detach().flatten().tolist() for p in params])
            sch.step()
        state = []
        for p in params:
            st = opt.state[p]
            state.append({k: (v.flatten().tolist() if torch.is_tensor(v) and v.dim() else float(v))
                          for k, v in st.items()})
            state[-1]["step_type"] = "tensor.%s" % str(st["step"].dtype).split(".")[-1] if torch.is_tensor(st["step"]) \
                else type(st["step"]).__name__
        out.append({"case": dict(c, **SCHEDULE), "optimizer_class": type(opt).__name__, "lrs": lrs, "init": init,
                    "grads": grads, "traj": traj, "state": state,
                    "state_keys": [k for k in opt.state[params[0]]],
                    "group_keys": sorted(k for k in opt.param_groups[0] if k != "params"),
                    "betas": list(opt.param_groups[0]["betas"]), "eps": opt.param_groups[0]["eps"]})
    with open(os.path.join(HERE, "adam_golden.json"), "w") as f:
        json.dump(out, f)
    print(len(out), "cases;", [(o["optimizer_class"], len(o["traj"])) for o in out])


if __name__ == "__main__":
    main()
