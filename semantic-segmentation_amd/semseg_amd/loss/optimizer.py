"""Optimizer and LR schedule of the training step (loss/optimizer.py:43-98 of the
reference): `get_optimizer(args, net) -> (optimizer,
scheduler)` with the reference's arguments (`--optimizer sgd|adam|radam`, `--amsgrad`,
`--lr`, `--weight_decay`, `--momentum`, `--lr_schedule poly|poly2|scl-poly`, `--poly_exp`,
`--poly_step`, `--max_epoch`, `--rescale`, `--repoly`).

Every optimizer is ONE streaming pass over all parameter tensors in a handful of
launches: `FusedSGD` (ssa_sgd_momentum_step), `FusedAdam` / `FusedRAdam`
(ssa_adam_advance + ssa_adam_step).  Their state_dicts have the layout of the
optimizers they replace (torch.optim.SGD's 'momentum_buffer'; torch.optim.Adam's and
loss/radam.py's 'step', 'exp_avg', 'exp_avg_sq'[, 'max_exp_avg_sq']), so the
reference's checkpoints restore into them (`restore_opt`) and vice versa.  What they
share -- the learning rate as a device scalar, the loss scaler of fp16 training, the
checks on the tensors, the snapshot a graph capture takes -- is `_FusedOptimizer`."""
import contextlib
import ctypes
import math

import torch
from torch import optim

from .._lib import lib, check
from ..config import cfg


def _on_gpu(p):
    return p.is_cuda


@contextlib.contextmanager
def _launch_scope(device):
    """Make `device` current and yield (stream handle, is that stream being captured)."""
    with torch.cuda.device(device):
        yield torch.cuda.current_stream().cuda_stream, torch.cuda.is_current_stream_capturing()


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def snapshot_state(optimizer):
    """Clones of every state tensor of `optimizer`, by parameter and name (what a graph capture's warm-up
    steps change and `restore_state` puts back)."""
    return {p: {k: v.clone() for k, v in st.items() if torch.is_tensor(v)} for p, st in optimizer.state.items()}


def restore_state(optimizer, snap):
    """Every state tensor back to its value in `snap`; one that did not exist then goes to zeros (the
    optimizers' first-step state).  In place: a captured graph keeps the tensors' addresses."""
    with torch.no_grad():
        for p, st in optimizer.state.items():
            old = snap.get(p, {})
            for k, v in st.items():
                if torch.is_tensor(v):
                    if k in old:
                        v.copy_(old[k])
                    else:
                        v.zero_()


class _FusedOptimizer(optim.Optimizer):
    """What the fused optimizers share.

    The learning rate is read by the kernels from a device scalar, so a captured
    hipGraph of the training step follows the LR schedule: after the scheduler
    changed `param_groups[..]['lr']` call `sync_lr()` (step() does it itself when
    it is not being captured)."""

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._lr_dev = {}          # group index -> (device scalar, value it holds)
        self.loss_scaler = None    # semseg_amd.amp.LossScaler (fp16 training): un-scale, overflow test, skipped steps
        self._pending_scaler_state = None   # a checkpoint's scaler state loaded before a scaler was attached

    def _lr_scalar(self, gi, group, device, capturing):
        ent = self._lr_dev.get(gi)
        lr = float(group["lr"])
        if ent is None or ent[0].device != device:
            ent = self._lr_dev[gi] = [torch.full((1,), lr, dtype=torch.float32, device=device), lr]
        elif ent[1] != lr and not capturing:
            ent[0].fill_(lr)
            ent[1] = lr
        return ent[0]

    def sync_lr(self):
        """Push the groups' current learning rates to the device scalars the kernels read."""
        for gi, group in enumerate(self.param_groups):
            ent = self._lr_dev.get(gi)
            if ent is not None and ent[1] != float(group["lr"]):
                ent[0].fill_(float(group["lr"]))
                ent[1] = float(group["lr"])

    def _dense_grad(self, p):
        """p's gradient, contiguous, after the checks every fused update makes (no fallback: they raise)."""
        name = type(self).__name__
        g = p.grad
        if not (_on_gpu(p) and p.dtype == torch.float32 and g.dtype == torch.float32 and not g.is_sparse):
            raise RuntimeError("%s updates dense fp32 parameters on the GPU" % name)
        if not p.is_contiguous():
            raise RuntimeError("%s needs contiguous parameters" % name)
        return g if g.is_contiguous() else g.contiguous()

    def _new_state(self, p, what):
        if p.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("%s: run one eager step before capturing the step in a graph (the %s are created on "
                               "the first step)" % (type(self).__name__, what))
        return torch.zeros_like(p, memory_format=torch.contiguous_format)

    def _scaler_check(self):
        """With a loss scaler: the overflow test over EVERY gradient before any parameter moves (apex skips the
        whole step).  Returns the address of the scaler's device record, or None."""
        amp = self.loss_scaler
        if amp is None:
            return None
        grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                 for group in self.param_groups for p in group["params"] if p.grad is not None]
        if any(g.device != amp.state.device for g in grads):
            raise RuntimeError("%s with a loss scaler drives ONE device per process: the overflow record lives "
                               "on %s, a gradient on another device" % (type(self).__name__, amp.state.device))
        if grads:
            with _launch_scope(amp.state.device) as (stream, _):
                amp.check(grads, stream)
        return amp.state.data_ptr()

    def _scaler_update(self):
        amp = self.loss_scaler
        if amp is not None:
            with _launch_scope(amp.state.device) as (stream, _):
                amp.update(stream)

    def snapshot_state(self):
        """What a graph capture's warm-up steps change in the optimizer (semseg_amd/graphed.py puts it back)."""
        return snapshot_state(self)

    def restore_state(self, snap):
        restore_state(self, snap)

    def state_dict(self):
        sd = super().state_dict()
        if self.loss_scaler is not None:
            sd["loss_scaler"] = self.loss_scaler.state_dict()       # (apex keeps amp.state_dict() beside the optimizer's)
        return sd

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        ls = state_dict.pop("loss_scaler", None)
        super().load_state_dict(state_dict)
        if ls is not None:
            if self.loss_scaler is not None:
                self.loss_scaler.load_state_dict(ls)
            else:                       # restored before amp.initialize: semseg_amd.amp.attach_scaler applies it
                self._pending_scaler_state = dict(ls)


class FusedSGD(_FusedOptimizer):
    """torch.optim.SGD(lr, momentum, weight_decay, nesterov) semantics, dampening 0."""

    def __init__(self, params, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError("invalid SGD hyper-parameters")
        if dampening != 0.0:
            raise ValueError("dampening is not supported (the reference trains with 0)")
        if nesterov and momentum <= 0.0:
            raise ValueError("Nesterov momentum requires a momentum")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        amp_ptr = self._scaler_check()
        for gi, group in enumerate(self.param_groups):
            momentum = float(group["momentum"])
            by_device = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = self._dense_grad(p)
                buf = None
                if momentum != 0.0:
                    st = self.state[p]
                    buf = st.get("momentum_buffer")
                    if buf is None:          # zeros: m*0 + d == d, torch's first step
                        buf = st["momentum_buffer"] = self._new_state(p, "momentum buffers")
                by_device.setdefault(p.device, []).append((p, g, buf))
            for device, items in by_device.items():
                n = len(items)
                with _launch_scope(device) as (stream, capturing):
                    lr_dev = self._lr_scalar(gi, group, device, capturing)
                    P = (ctypes.c_void_p * n)(*[p.data_ptr() for p, _, _ in items])
                    G = (ctypes.c_void_p * n)(*[g.data_ptr() for _, g, _ in items])
                    Bf = (ctypes.c_void_p * n)(*[b.data_ptr() for _, _, b in items]) if momentum != 0.0 else None
                    N = (ctypes.c_int64 * n)(*[p.numel() for p, _, _ in items])
                    check(lib().ssa_sgd_momentum_step(P, G, Bf, N, n, float(group["lr"]), lr_dev.data_ptr(),
                                                      momentum, float(group["weight_decay"]),
                                                      int(bool(group["nesterov"])), amp_ptr, stream),
                          "ssa_sgd_momentum_step")
                # the kernel wrote through raw pointers: tell autograd (saved-tensor checks) and the
                # packed-filter cache (hip_backend.refresh_packed_filters keys on ._version) that
                # the parameters and buffers changed
                _mark_updated([p for p, _, _ in items] + [b for _, _, b in items if b is not None])
        self._scaler_update()
        return loss


_ADAM, _AMSGRAD, _RADAM = 0, 1, 2       # `mode` of ssa_adam_advance / ssa_adam_step
# what torch.optim.Adam's newer signature offers and the fused kernels do not: refused unless switched off
_ADAM_REFUSED = ("maximize", "decoupled_weight_decay", "capturable", "differentiable", "foreach", "fused")


class _FusedAdamFamily(_FusedOptimizer):
    """Adam, AMSGrad and RAdam on ssa_adam_advance + ssa_adam_step.

    The step counts live on the DEVICE, one 16-byte record {t, rectified, c1, c2} per parameter (a row of
    `_rec[device]`): the advance kernel counts and derives the bias corrections from t, so a captured step
    counts its own replays, a step the loss scaler skips does not count, and a parameter without a gradient
    keeps its own t.  `state_dict()` reads the counts back in one copy and writes them as 'step' in the layout
    of the optimizer this class replaces; `load_state_dict()` writes them to the device."""

    _STATE = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, defaults):
        lr, (beta1, beta2) = defaults["lr"], defaults["betas"]
        if torch.is_tensor(lr):
            raise ValueError("a tensor lr is not supported (the kernels read the device scalar of sync_lr())")
        if lr < 0.0 or defaults["eps"] < 0.0 or defaults["weight_decay"] < 0.0 or \
                not 0.0 <= beta1 < 1.0 or not 0.0 <= beta2 < 1.0:
            raise ValueError("invalid %s hyper-parameters" % type(self).__name__)
        super().__init__(params, defaults)
        self._rec = {}             # device -> int32 [parameters of this optimizer, 4]: the step records
        self._rows = {}            # parameter -> its row
        self._tables = {}          # (group, device) -> the launch tables that only change with the parameter set

    def _mode(self, group):
        raise NotImplementedError

    def _step_value(self, t):
        """A step count as the replaced optimizer's state_dict holds it."""
        raise NotImplementedError

    def _row_of(self, p):
        if p not in self._rows:
            self._rows = {q: i for i, q in enumerate(q for g in self.param_groups for q in g["params"])}
        return self._rows[p]

    def _records(self, device):
        """The step records on `device` (zeros = no step taken), one row per parameter of the optimizer."""
        n = sum(len(g["params"]) for g in self.param_groups)
        rec = self._rec.get(device)
        if rec is None or rec.shape[0] < n:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("%s: run one eager step before capturing the step in a graph (the step records "
                                   "are created on the first step)" % type(self).__name__)
            new = torch.zeros((n, 4), dtype=torch.int32, device=device)
            if rec is not None:
                new[:rec.shape[0]] = rec
            rec = self._rec[device] = new
            self._tables = {}
        return rec

    def step_counts(self):
        """The device step count of every parameter, in the order of `param_groups` (one copy per device)."""
        params = [p for g in self.param_groups for p in g["params"]]
        host = {d: r[:, 0].cpu().tolist() for d, r in self._rec.items()}
        return [host[p.device][self._row_of(p)] if p.device in host and self._row_of(p) < len(host[p.device]) else 0
                for p in params]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        amp_ptr = self._scaler_check()
        for gi, group in enumerate(self.param_groups):
            mode = self._mode(group)
            names = self._STATE + (("max_exp_avg_sq",) if mode == _AMSGRAD else ())
            beta1, beta2 = (float(b) for b in group["betas"])
            by_device = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = self._dense_grad(p)
                st = self.state[p]
                for k in names:
                    if k not in st:          # zeros and t = 0: the optimizers' first-step state
                        st[k] = self._new_state(p, "moment estimates")
                by_device.setdefault(p.device, ([], []))
                by_device[p.device][0].append(p)
                by_device[p.device][1].append(g)
            for device, (ps, gs) in by_device.items():
                n = len(ps)
                rec = self._records(device)
                tab = self._tables.get((gi, device))
                sts = [self.state[p] for p in ps]
                key = (mode, rec.data_ptr(), tuple(id(st[k]) for st in sts for k in names))
                if tab is None or tab[0] != key:
                    base = rec.data_ptr()
                    tab = self._tables[(gi, device)] = (
                        key, [_ptr_array([st[k] for st in sts]) for k in names],
                        (ctypes.c_void_p * n)(*[base + 16 * self._row_of(p) for p in ps]),
                        (ctypes.c_int64 * n)(*[p.numel() for p in ps]),
                        [st[k] for st in sts for k in names])
                _, S, R, N, state_tensors = tab
                with _launch_scope(device) as (stream, capturing):
                    lr_dev = self._lr_scalar(gi, group, device, capturing)
                    check(lib().ssa_adam_advance(R, n, mode, beta1, beta2, amp_ptr, stream), "ssa_adam_advance")
                    check(lib().ssa_adam_step(_ptr_array(ps), _ptr_array(gs), S[0], S[1],
                                              S[2] if mode == _AMSGRAD else None, R, N, n, mode, float(group["lr"]),
                                              lr_dev.data_ptr(), beta1, beta2, float(group["eps"]),
                                              float(group["weight_decay"]), amp_ptr, stream), "ssa_adam_step")
                # (raw-pointer writes: see FusedSGD.step)
                _mark_updated(ps + state_tensors)
        self._scaler_update()
        return loss

    def snapshot_state(self):
        return snapshot_state(self), {d: r.clone() for d, r in self._rec.items()}

    def restore_state(self, snap):
        tensors, recs = snap
        restore_state(self, tensors)
        with torch.no_grad():
            for d, r in self._rec.items():
                r.zero_()                    # (a record that did not exist then: t = 0)
                if d in recs:
                    r[:recs[d].shape[0]] = recs[d]

    def state_dict(self):
        sd = super().state_dict()
        counts = self.step_counts()
        # torch packs the parameters in the order of param_groups: packed index i is row i
        sd["state"] = {i: dict([("step", self._step_value(counts[i]))] + list(st.items()))
                       for i, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        for group in state_dict["param_groups"]:
            self._refuse(group)
        super().load_state_dict(state_dict)
        self._tables = {}
        params = [p for g in self.param_groups for p in g["params"]]
        self._rows = {p: i for i, p in enumerate(params)}
        counts = {}
        for i, p in enumerate(params):
            st = self.state.get(p)
            if not st:
                continue
            counts.setdefault(p.device, [0] * len(params))[i] = int(st.pop("step", 0))
            for k in list(st):               # dense fp32 beside the parameter, whatever the checkpoint held
                if torch.is_tensor(st[k]):
                    st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()
        self._rec = {}
        for d, ts in counts.items():         # one copy per device (c1, c2 are derived from t by the next advance)
            host = torch.zeros((len(params), 4), dtype=torch.int32)
            host[:, 0] = torch.tensor(ts, dtype=torch.int32)
            self._rec[d] = host.to(d)

    @staticmethod
    def _refuse(options):
        for k in _ADAM_REFUSED:
            if options.get(k):
                raise ValueError("%s=%r is not supported by the fused Adam / RAdam step" % (k, options[k]))


class FusedAdam(_FusedAdamFamily):
    """torch.optim.Adam(lr, betas, eps, weight_decay, amsgrad) semantics: L2 weight decay, single-tensor arithmetic."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **unsupported):
        unknown = sorted(set(unsupported) - set(_ADAM_REFUSED))
        if unknown:
            raise TypeError("FusedAdam got unexpected keyword arguments %s" % unknown)
        self._refuse(unsupported)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad)))

    def _mode(self, group):
        return _AMSGRAD if group["amsgrad"] else _ADAM

    def _step_value(self, t):
        return torch.tensor(float(t), dtype=torch.float32)


class FusedRAdam(_FusedAdamFamily):
    """The reference's RAdam (loss/radam.py) as written: rectified from N_sma >= 5 on, the weight decay scales the
    parameter (`p += -wd lr p`) and stays out of the gradient."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, **unsupported):
        unknown = sorted(set(unsupported) - set(_ADAM_REFUSED))
        if unknown:
            raise TypeError("FusedRAdam got unexpected keyword arguments %s" % unknown)
        self._refuse(unsupported)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _mode(self, group):
        return _RADAM

    def _step_value(self, t):
        return int(t)


def _mark_updated(tensors):
    torch.autograd.graph.increment_version(tensors)


def poly_schedules(args):
    """The LR multipliers of loss/optimizer.py:67-92, by name."""
    def poly_schd(epoch):
        return math.pow(1 - epoch / args.max_epoch, args.poly_exp)

    def poly2_schd(epoch):
        poly_exp = args.poly_exp if epoch < args.poly_step else 2 * args.poly_exp
        return math.pow(1 - epoch / args.max_epoch, poly_exp)

    def scl_poly_schd(epoch):
        thresh = cfg.get("REDUCE_BORDER_EPOCH", -1)
        if epoch < thresh:
            return math.pow(1 - epoch / args.max_epoch, args.poly_exp)
        return args.rescale * math.pow(1 - (epoch - thresh) / (args.max_epoch - thresh), args.repoly)

    return {"poly": poly_schd, "poly2": poly2_schd, "scl-poly": scl_poly_schd}


def get_optimizer(args, net):
    """loss/optimizer.py:43-98: `--optimizer sgd | adam (+ --amsgrad) | radam`, each on its fused HIP step."""
    if args.optimizer == "sgd":
        optimizer = FusedSGD(net.parameters(), lr=args.lr, weight_decay=args.weight_decay, momentum=args.momentum,
                             nesterov=False)
    elif args.optimizer == "adam":
        optimizer = FusedAdam(net.parameters(), lr=args.lr, weight_decay=args.weight_decay, amsgrad=args.amsgrad)
    elif args.optimizer == "radam":
        optimizer = FusedRAdam(net.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    else:
        raise ValueError("Not a valid optimizer: {}".format(args.optimizer))
    schedules = poly_schedules(args)
    if args.lr_schedule not in schedules:
        raise ValueError("unknown lr schedule {}".format(args.lr_schedule))
    if args.lr_schedule == "scl-poly" and cfg.get("REDUCE_BORDER_EPOCH", -1) == -1:
        raise ValueError("ERROR Cannot Do Scale Poly")
    scheduler = optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=schedules[args.lr_schedule])
    return optimizer, scheduler


def forgiving_state_restore(net, loaded_dict):
    """loss/optimizer.py:134-154: load the entries whose name and size match, keep the rest."""
    net_state_dict = net.state_dict()
    matched = {k: loaded_dict[k] for k in net_state_dict
               if k in loaded_dict and net_state_dict[k].size() == loaded_dict[k].size()}
    net_state_dict.update(matched)
    net.load_state_dict(net_state_dict)
    return net


def restore_opt(optimizer, checkpoint):
    """loss/optimizer.py:124-126"""
    assert "optimizer" in checkpoint, "cant find optimizer in checkpoint"
    optimizer.load_state_dict(checkpoint["optimizer"])


def restore_net(net, checkpoint):
    """loss/optimizer.py:129-131"""
    assert "state_dict" in checkpoint, "cant find state_dict in checkpoint"
    forgiving_state_restore(net, checkpoint["state_dict"])


def restore_snapshot(net, optimizer, snapshot, restore_optimizer_bool):
    """loss/optimizer.py:106-121"""
    checkpoint = torch.load(snapshot, map_location=torch.device("cpu"))
    if optimizer is not None and "optimizer" in checkpoint and restore_optimizer_bool:
        optimizer.load_state_dict(checkpoint["optimizer"])
    net = forgiving_state_restore(net, checkpoint["state_dict"] if "state_dict" in checkpoint else checkpoint)
    return net, optimizer


load_weights = restore_snapshot      # loss/optimizer.py:97-103 (the reference's wrapper only adds a log line)
