"""--align_corners (cfg.MODEL.ALIGN_CORNERS = True) end to end on the GPU: tests/test_e2e_gpu.py's op-by-op evaluation rule
and its training-step rule -- the very functions, imported -- at 2 x 256 x 256 with the flag on.  The teacher (the fp32
oracle operators) and the storage emulation are subclasses of OracleBackend / Bf16EmuBackend whose `_bilinear` and
`image_to_nhwc` resize with align_corners=True; the tolerances are that file's own, relative to the emulation's measured
floor.  A last case captures a training step with the flag on and replays it: the flag is a launch argument, baked into
the graph, and the replay gives the eager step's loss."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import test_e2e_gpu as E

pytestmark = pytest.mark.gpu


def _ac_backends():
    import bf16_emu_backend as BE
    import oracle_backend as OB

    def resize(x_nhwc, size):
        return OB._to_nhwc(F.interpolate(OB._to_nchw(x_nhwc), size=tuple(size), mode="bilinear", align_corners=True))

    def image_to_nhwc(self, images, out_hw=None):
        x = images if images.dtype == torch.float64 else images.float()
        if out_hw is not None and tuple(out_hw) != tuple(x.shape[2:]):
            x = F.interpolate(x, size=tuple(out_hw), mode="bilinear", align_corners=True)
        x = OB._to_nhwc(x)
        return F.pad(x, (0, 16 - x.shape[3]))

    def bilinear(self, x, size, out_f32=False):
        return x if tuple(x.shape[1:3]) == tuple(size) else resize(x, size)

    def emu_bilinear(self, x, size, out_f32=False):
        if tuple(x.shape[1:3]) == tuple(size):
            return x
        y = resize(x, size)
        return y if (out_f32 or x.shape[3] in BE.F32_CHANNELS) else BE.R(y)      # Bf16EmuBackend._bilinear's storage rule

    # (the teacher keeps the class NAME: test_e2e_gpu._run tells the oracle from the storage paths by it)
    oracle = type("OracleBackend", (OB.OracleBackend,), {"_bilinear": bilinear, "image_to_nhwc": image_to_nhwc})
    emu = type("Bf16EmuBackendAC", (BE.Bf16EmuBackend,), {
        "_bilinear": emu_bilinear, "image_to_nhwc": lambda self, images, out_hw=None: BE.R(image_to_nhwc(self, images, out_hw))})
    return oracle, emu


@contextlib.contextmanager
def _flag_on():
    """cfg.MODEL.ALIGN_CORNERS = True; the oracle's operators and the two backends test_e2e_gpu's rules instantiate under
    the same rule; everything restored."""
    import bf16_emu_backend as BE
    import oracle_backend as OB
    from oracle import ops as O
    from semseg_amd.config import cfg
    oracle, emu = _ac_backends()
    saved = (cfg.MODEL.ALIGN_CORNERS, O.bilinear, O.resize_x, OB.OracleBackend, BE.Bf16EmuBackend)
    cfg.MODEL.ALIGN_CORNERS = True
    O.bilinear = lambda x, size: F.interpolate(x, size=size, mode="bilinear", align_corners=True)
    O.resize_x = lambda x, scale_factor: F.interpolate(x, scale_factor=scale_factor, mode="bilinear", align_corners=True,
                                                       recompute_scale_factor=True)
    OB.OracleBackend, BE.Bf16EmuBackend = oracle, emu
    try:
        yield cfg
    finally:
        cfg.MODEL.ALIGN_CORNERS, O.bilinear, O.resize_x, OB.OracleBackend, BE.Bf16EmuBackend = saved


@pytest.fixture(scope="module")
def setup():
    """test_e2e_gpu's fixture (seeded weights, 2 x 256 x 256 batch, BN statistics calibrated by the oracle) with the
    calibration pass under align_corners=True."""
    from semseg_amd.config import cfg
    from semseg_amd.loss import RMILoss
    from semseg_amd.network import ocrnet
    from oracle.model import Net
    cfg.LOSS.SUPERVISED_MSCALE_WT = 0.05
    cfg.MODEL.N_SCALES = None
    cfg.MODEL.BNFUNC = None
    net = ocrnet.HRNet_Mscale(19, RMILoss(num_classes=19, ignore_index=255))
    shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    sd = E.parity_state_dict(shapes, seed=0)
    images, gts = E._synth(2, 256, 256, seed=77)
    with _flag_on(), torch.no_grad():
        Net(sd, 19, training=True, bn_momentum=1.0, criterion="ce").two_scale_forward(images, gts)
    return sd, images, gts


def test_backends_follow_the_rule():
    """The two subclasses really resize under the other rule (and only the resize differs)."""
    import oracle_backend as OB
    x = torch.randn(1, 5, 7, 19)
    with _flag_on():
        import bf16_emu_backend as BE
        y = OB.OracleBackend()._bilinear(x, (9, 13))
        e = BE.Bf16EmuBackend()._bilinear(x, (9, 13))
        assert type(OB.OracleBackend()).__name__ == "OracleBackend"
    y0 = OB.OracleBackend()._bilinear(x, (9, 13))
    assert torch.equal(y[:, ::2, ::2], x) and not torch.equal(y, y0) and torch.equal(e, y)      # corners aligned; 19 channels stay fp32


def test_eval_op_by_op_with_the_flag_on(setup):
    with _flag_on():
        E.test_eval_op_by_op(setup)


def test_train_step_with_the_flag_on(setup):
    with _flag_on():
        E._check_train_step(*setup)


def test_captured_step_with_the_flag_on_replays_the_eager_loss():
    """tests/test_graphed_step_gpu.py's network and loop at 1 x 256 x 256, flag on, with the learning rate at zero: the
    weights stay put, so every step on the batch -- the eager one, the captured step's warm-up passes and its replays --
    computes ONE loss, up to the order of the atomics inside the BatchNorm sums (that file's reason for a tolerance, and
    its tolerance).  With weight updates the steps of this random network drift apart by more than that within two
    iterations, flag or no flag, and a replay could not be held to the eager loss.  The flag is baked in at capture: switched
    off afterwards, the replay still gives the flag-on loss, and an eager step gives another."""
    import semseg_amd
    import __graft_entry__ as ge
    from semseg_amd.config import cfg
    from test_graphed_step_gpu import _build, _reference_loop
    images, gts = ge._synth(1, 256, 256, 40, "cuda")
    batch = {"images": images, "gts": gts}

    def frozen():
        net, optim = _build()
        for g in optim.param_groups:
            g["lr"] = 0.0
        return net, optim
    with _flag_on():
        net, optim = frozen()
        init = {k: v.clone() for k, v in net.state_dict().items()}
        eager = _reference_loop(net, optim, [batch] * 2)
        net2, optim2 = frozen()
        net2.load_state_dict(init)
        gnet, goptim = semseg_amd.graph_training(net2, optim2)
        graphed = _reference_loop(gnet, goptim, [batch] * 5)
        replays = gnet._stepper.replays
        assert cfg.MODEL.ALIGN_CORNERS
    # flag off again: the graph keeps the rule of its capture, an eager step does not
    assert not cfg.MODEL.ALIGN_CORNERS
    late = _reference_loop(gnet, goptim, [batch])
    net3, optim3 = frozen()
    net3.load_state_dict(init)
    off = _reference_loop(net3, optim3, [batch])
    print("eager", eager, "graphed", graphed, "replay after the flag went off", late, "eager with the flag off", off, "replays", replays)
    assert replays >= 2 and gnet._stepper.replays == replays + 1
    for b in graphed + late:
        assert abs(b - eager[0]) <= 2e-3 * abs(eager[0]), (eager, graphed, late)
    assert abs(off[0] - eager[0]) > 2e-3 * abs(eager[0]), (off, eager)          # outside the tolerance above
