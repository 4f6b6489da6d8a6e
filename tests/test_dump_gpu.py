"""The dump-tail kernels on the device (csrc/dump_tail.hip), through the C ABI: the cases of tests/dump_cases.py (the
same functions tests/test_dump_emu_cpu.py runs on the CPU emulation) against tests/dump_ref.py byte for byte -- here the
device's own arithmetic is under test: the IEEE fp32 division, the sums and products that must not contract into FMAs,
the saturating cast.  Then ImageDumper.dump of the reference's golden case with device assets, and one graph capture of
ssa_dump_tail replayed on two inputs."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dump_cases as K
import dump_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    from semseg_amd import _lib
    return _lib.lib()


def test_all_outputs_at_every_shape(L):
    assert K.check_shapes_all_outputs(L, DEV) == 21


def test_subsets_of_outputs(L):
    assert K.check_subsets_of_outputs(L, DEV) == 10


def test_unaligned_pointers_take_the_pixel_path(L):
    assert K.check_unaligned_pointers(L, DEV) == 14


def test_all_pairs_blend_equals_live_pillow(L):
    assert K.check_all_pairs_blend(L, DEV) == 3


def test_all_bytes_denormalise_equals_torch(L):
    assert K.check_all_bytes_denormalise(L, DEV) == 1


def test_mask_u8(L):
    assert K.check_mask_u8(L, DEV) == 10


def test_full_size_image_passes_the_cap_of_the_grid(L):
    assert K.check_full_size(L, DEV) == 7


def test_image_dumper_writes_the_reference_files_from_device_assets(tmp_path):
    """ImageDumper.dump with the assets as eval_minibatch(assets_on_device=True) leaves them, in the three modes, against
    the files the reference itself wrote for the same batch (tests/golden/dump_golden.npz)."""
    from semseg_amd.config import cfg
    from semseg_amd.utils import dumper
    z, meta = R.load_golden()
    saved = {k: cfg.get(k) for k in ("RESULT_DIR", "DATASET_INST", "GLOBAL_RANK")}
    saved_ms = (cfg.DATASET.MEAN, cfg.DATASET.STD)
    try:
        cfg.DATASET_INST, cfg.GLOBAL_RANK = R.golden_dataset(meta), 0
        cfg.DATASET.MEAN, cfg.DATASET.STD = meta["mean"], meta["std"]
        for mode, kw in (("visual", dict(dump_assets=True)), ("submission", dict(dump_for_submission=True)),
                         ("auto_labelling", dict(dump_for_auto_labelling=True))):
            cfg.RESULT_DIR = str(tmp_path / mode)
            d = dumper.ImageDumper(val_len=meta["val_len"], tensorboard=False, **kw)
            dd = K.device_form(R.golden_dump_dict(z, meta), DEV)
            d.dump(dd, 0)
            assert "predictions" not in dd["assets"]
            want = R.golden_files(z, meta, mode)
            assert sorted(f for f in os.listdir(d.save_dir) if f.endswith(".png")) == sorted(want)
            for fn, entry in want.items():
                assert R.same(R.decode(os.path.join(d.save_dir, fn)), entry), (mode, fn)
    finally:
        cfg.update(saved)
        cfg.DATASET.MEAN, cfg.DATASET.STD = saved_ms


def test_graph_capture_replayed_on_two_inputs(L):
    """One torch.cuda.graph over ssa_dump_tail with every output; replayed on two different inputs copied into the
    captured buffers: nothing in the launch depends on the host or allocates."""
    H, W = 37, 53
    pal, ids = K.tables()
    inputs = [K.random_inputs(H, W, seed) for seed in (31, 32)]
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    bufs = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in inputs[0]]
    pal_d, ids_d = torch.from_numpy(pal).to(DEV), torch.from_numpy(ids).to(DEV)
    outs = {k: torch.zeros((H, W, 3) if k.endswith("_rgb") else (H, W), dtype=torch.uint8, device=DEV) for k in K.OUTS}
    inv_mean, inv_std = R.inv_norm(K.MEAN, K.STD)
    im, isd = (ctypes.c_float * 3)(*inv_mean.tolist()), (ctypes.c_float * 3)(*inv_std.tolist())

    def launch():
        x, gts, pred, prob, err = bufs
        rc = L.ssa_dump_tail(P(x), H * W, im, isd, P(gts), P(pred), P(pal_d), P(ids_d), P(prob), P(err), R.ALPHA, H, W,
                             *[P(outs[k]) for k in K.OUTS], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    n = 0
    for inp in (inputs[1], inputs[0]):
        for b, a in zip(bufs, inp):
            b.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        g.replay()
        torch.cuda.synchronize()
        n += K.compare({k: t.cpu().numpy() for k, t in outs.items()}, K.expected(*inp, pal, ids))
    assert n == 14
