"""The boundary F-score without a GPU:
  * tests/fboundary_ref.py reproduces the golden data of the real reference (tests/golden/fboundary_golden.npz: Fpc, Fc
    and every per-(image, class) F and precision) with == in float64, and live scikit-image where that is installed;
  * the radius rule against NumPy, argument rejection before anything touches a device, the branches of f_scores,
    BoundaryMeter's arithmetic on hand-made counts, the `utils.f_boundary` registration of dropin.install();
  * the cases of tests/fboundary_cases.py discriminate what they are there for.
tests/test_fboundary_emu_cpu.py runs the kernels themselves on the CPU emulation."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fboundary_cases as K
import fboundary_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fb():
    from semseg_amd.utils import f_boundary
    return f_boundary


@pytest.mark.parametrize("name", K.ALL)
def test_restatement_reproduces_the_reference_fixture(name):
    g, k, ref = K.golden(), K.CASES[name], K.reference(name)
    pred, gt = K.inputs(name)
    assert np.array_equal(g[k["inp"] + "/pred"], pred) and np.array_equal(g[k["inp"] + "/gt"], gt), \
        "the seeded inputs are not the ones the fixture was made of"
    for key in ("F", "P", "Fpc", "Fc"):
        want = g[name + "/" + key]
        assert want.dtype == np.float64 and want.shape == ref[key].shape
        assert (ref[key] == want).all(), (name, key)


def test_fixture_records_its_shims():
    meta = json.loads(str(K.golden()["meta"]))
    assert any("np.bool" in s for s in meta["shims"]) and any("disk" in s for s in meta["shims"])
    assert any("binary_dilation" in s for s in meta["shims"])


@pytest.mark.parametrize("name", ("seam_r3", "disk_out", "disk_in", "edge_5x7_r8", "checker"))
def test_restatement_equals_live_scikit_image(name):
    morph = pytest.importorskip("skimage.morphology")
    k, ref = K.CASES[name], K.reference(name)
    pred, gt = K.inputs(name)
    for i in range(pred.shape[0]):
        ign = gt[i] == k["ignore"]
        for c in range(k["C"]):
            fg_b, gt_b = R.seg2bmap((pred[i] == c) & ~ign), R.seg2bmap((gt[i] == c) & ~ign)
            fg_d = morph.binary_dilation(fg_b, morph.disk(ref["r"]))
            gt_d = morph.binary_dilation(gt_b, morph.disk(ref["r"]))
            assert (fg_b.sum(), gt_b.sum(), (fg_b & gt_d).sum(), (gt_b & fg_d).sum()) == tuple(ref["counts"][i, c])


def test_radius_rule():
    fb = _fb()
    for shape in ((1024, 2048), (2177, 2177), (70, 131), (1, 1), (713, 713), (1536, 2177)):
        for th in (0.008, 0.02, 0.0, 0.003, 1, 3, 32, 5.0):
            want = th if th >= 1 else np.ceil(th * np.linalg.norm(shape))
            if want <= 32:
                r = fb.boundary_radius(shape, th)
                assert isinstance(r, int) and r == want, (shape, th)
    assert fb.boundary_radius((1024, 2048), 0.008) == 19 and fb.boundary_radius((2177, 2177), 0.008) == 25
    assert fb.boundary_radius((70, 131), np.float64(0.02)) == 3
    for shape, th in (((70, 131), 1.5), ((70, 131), 33), ((70, 131), 2.0001), ((4000, 4000), 0.008), ((70, 131), -0.1),
                      ((70, 131), float("nan")), ((0, 5), 0.008)):
        with pytest.raises(ValueError):
            fb.boundary_radius(shape, th)


def test_python_surface_rejects_bad_arguments_without_a_device():
    fb = _fb()
    pred = torch.zeros((1, 4, 5), dtype=torch.uint8)
    gts = torch.zeros((1, 4, 5), dtype=torch.int64)
    bad = [
        (pred.long(), gts, 19, 255, 0.008),             # pred must be uint8
        (pred[0], gts[0], 19, 255, 0.008),              # [B, H, W]
        (pred, gts.int(), 19, 255, 0.008),              # gts uint8 or int64
        (pred, gts[:, :3], 19, 255, 0.008),             # one shape
        (pred, gts, 0, 255, 0.008), (pred, gts, 255, 255, 0.008),
        (pred, gts, 19, 255, 33), (pred, gts, 19, 255, 2.5),
        (pred.numpy(), gts.numpy(), 19, 255, 0.008),
    ]
    for a in bad:
        with pytest.raises(ValueError):
            fb.boundary_counts(*a)
    with pytest.raises(ValueError):
        fb.f_scores(np.zeros((2, 3)))


def test_boundary_counts_is_refused_inside_a_graph_capture(monkeypatch):
    """Graph capture is not offered: under a capturing stream boundary_counts raises before anything is launched."""
    fb = _fb()

    class OnDevice:
        is_cuda = True
    fb._refuse_capture(torch.zeros(1))                       # a host tensor (the emulation's device memory): no query
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    fb._refuse_capture(OnDevice())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="graph capture"):
        fb._refuse_capture(OnDevice())
    import inspect
    src = inspect.getsource(fb.boundary_counts)
    assert src.index("_refuse_capture(pred)") < src.index("torch.empty")     # before the first allocation


def test_c_abi_rejects_bad_arguments_without_a_device():
    """ssa_fboundary_counts returns SSA_EINVAL / SSA_EUNSUPPORTED before it touches the device."""
    from semseg_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)         # a non-null address; never dereferenced
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(pred=p, gts=p, B=1, H=4, W=4, C=19, r=2, counts=p, work=p, nbytes=128):
        return L.ssa_fboundary_counts(pred, gts, 0, B, H, W, C, 255, r, counts, work, nbytes, None)
    bad = (-1, -2)
    assert call(pred=None) in bad and call(gts=None) in bad and call(counts=None) in bad and call(work=None) in bad
    assert call(C=0) in bad and call(C=255) in bad and call(C=-1) in bad
    assert call(r=33) == -2 and call(r=-1) == -2
    assert call(B=0) in bad and call(B=65536) in bad and call(H=0) in bad and call(W=0) in bad
    assert call(nbytes=127) == -1                    # workspace below 8 * B * H * W bytes
    n = ctypes.c_size_t(0)
    assert L.ssa_fboundary_workspace_bytes(2, 70, 131, ctypes.byref(n)) == 0 and n.value == 8 * 2 * 70 * 131
    assert L.ssa_fboundary_workspace_bytes(0, 70, 131, ctypes.byref(n)) == -1
    assert L.ssa_fboundary_workspace_bytes(2, 70, 131, None) == -1


def test_f_scores_branches():
    fb = _fb()
    #                  n_fg n_gt fg_m gt_m
    cnt = np.array([[[0, 7, 0, 0],          # only the ground truth: P = 1, R = 0 -> F = 0
                     [5, 0, 0, 0],          # only the prediction: P = 0, R = 1 -> F = 0
                     [0, 0, 0, 0],          # neither: P = R = 1 -> F = 1
                     [4, 6, 0, 0],          # both, no match: P + R == 0 -> F = 0
                     [3, 7, 1, 5],          # both
                     [9, 9, 9, 9]]], dtype=np.int64)
    F, P = fb.f_scores(cnt)
    assert F.dtype == np.float64 and P.dtype == np.float64 and F.shape == (1, 6)
    p, r = 1 / float(3), 5 / float(7)
    assert F[0].tolist() == [0.0, 0.0, 1.0, 0.0, 2 * p * r / (p + r), 1.0]
    assert P[0].tolist() == [1.0, 0.0, 1.0, 0.0, p, 1.0]
    F2, P2 = fb.f_scores(torch.from_numpy(cnt))
    assert (F2 == F).all() and (P2 == P).all()
    Fr, Pr = R.scores(cnt)
    assert (Fr == F).all() and (Pr == P).all()


@pytest.mark.parametrize("name", K.ALL)
def test_f_scores_equal_the_fixture_on_the_restatement_counts(name):
    g, ref = K.golden(), K.reference(name)
    F, P = _fb().f_scores(ref["counts"])
    assert (F == g[name + "/F"]).all() and (P == g[name + "/P"]).all()


def test_boundary_meter_arithmetic():
    fb = _fb()
    a = np.array([[[3, 7, 1, 5], [0, 0, 0, 0], [0, 4, 0, 0]],
                  [[8, 8, 4, 2], [2, 0, 0, 0], [5, 5, 5, 5]]], dtype=np.int64)
    b = np.array([[[6, 6, 3, 6], [0, 0, 0, 0], [1, 1, 0, 0]]], dtype=np.int64)
    m = fb.BoundaryMeter(3, 255)
    with pytest.raises(ValueError):
        m.avg
    m.add_counts(torch.from_numpy(a))
    m.add_counts(b)
    F = np.concatenate([R.scores(a)[0], R.scores(b)[0]])
    Fpc, Fc = R.fpc_fc(F)
    assert (m.Fpc == Fpc).all() and (m.Fc == Fc).all() and m.Fc.tolist() == [3.0, 3.0, 3.0]
    assert m.avg == float(np.mean(Fpc / Fc))
    m.reset()
    m.add_counts(b)
    assert m.Fc.tolist() == [1.0, 1.0, 1.0] and (m.Fpc == R.scores(b)[0][0]).all()


def test_install_registers_f_boundary_only_on_request():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "semantic-segmentation_amd"), ROOT]))
    code = """
import inspect
import sys
import semseg_amd.dropin as dropin
dropin.install()
assert "utils.f_boundary" not in sys.modules
dropin.install(device_eval_tail=True, device_dumper=False)
assert "utils.f_boundary" not in sys.modules
dropin.install(device_f_boundary=True)
import semseg_amd.utils as U
m = sys.modules["utils.f_boundary"]
assert m.eval_mask_boundary is U.eval_mask_boundary and m.BoundaryMeter is U.BoundaryMeter
assert list(inspect.signature(m.eval_mask_boundary).parameters)[:5] == ["seg_mask", "gt_mask", "num_classes", "num_proc", "bound_th"]
sig = inspect.signature(m.eval_mask_boundary).parameters
assert sig["num_proc"].default == 10 and sig["bound_th"].default == 0.008
assert inspect.signature(U.eval_minibatch).parameters["boundary"].default is None
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


# ---------------------------------------------------------------------------- what the cases are there for
def test_every_branch_occurs_and_the_radius_matters():
    cnt = K.reference("branches")["counts"][0]
    assert [R.branch(cnt[c]) for c in range(8)] == ["both", "gt", "both", "pred", "both", "none", "none", "none"]
    assert cnt[2, 2] == 0 and cnt[2, 3] == 0 and cnt[2, 0] > 0 and cnt[2, 1] > 0          # both present, no match
    assert 0 < cnt[0, 2] < cnt[0, 0] and 0 < cnt[0, 3] < cnt[0, 1]                           # 0 < match < n, both ways
    seen = {R.branch(K.reference(n)["counts"][i, c]) for n in K.ALL for i in range(K.reference(n)["counts"].shape[0])
            for c in range(K.CASES[n]["C"])}
    assert seen == {"gt", "pred", "none", "both"}


def test_disk_cases_tell_the_disk_from_its_neighbours():
    """radius 5 against 4 (the ring just inside the disk loses matches), against 6 and against the 11 x 11 square (the
    ring just outside gains some): the counts differ under each of them."""
    import scipy.ndimage as ndi
    for name, r in (("disk_in", 4), ("disk_out", 6)):
        k = K.CASES[name]
        pred, gt = K.inputs(name)
        assert K.reference(name)["r"] == 5
        assert not np.array_equal(R.counts(pred, gt, k["C"], k["ignore"], r), K.reference(name)["counts"]), (name, r)
    pred, gt = K.inputs("disk_out")
    fg_b, gt_b = R.seg2bmap(pred[0] == 0), R.seg2bmap(gt[0] == 0)
    square = (fg_b & ndi.binary_dilation(gt_b, structure=np.ones((11, 11), bool))).sum()
    assert square != K.reference("disk_out")["counts"][0, 0, 2]
    # inside the ring everything matches, outside not everything does
    assert K.reference("disk_in")["counts"][0, 0, 2] == K.reference("disk_in")["counts"][0, 0, 0]
    assert K.reference("disk_out")["counts"][0, 0, 2] < K.reference("disk_out")["counts"][0, 0, 0]


def test_case_shapes_cover_the_kernel_tiles_and_label_rules():
    pred, gt = K.inputs("seam_r20")
    B, H, W = pred.shape
    assert B == 2 and -(-H // K.TILE_H) >= 3 and -(-W // K.TILE_W) >= 3 and H % K.TILE_H and W % K.TILE_W
    assert [K.reference(n)["r"] for n in ("seam_r2", "seam_r3", "seam_r20")] == [2, 3, 20] and 20 > K.TILE_H
    assert (gt == 255).mean() > 0.02
    pred, gt = K.inputs("labels65")
    assert (gt == 65).any() and (gt == 70).any() and (gt == 255).any() and (gt == -1).any() and (pred >= 65).any()
    assert not K.fits_u8("labels65") and K.fits_u8("seam_r2")
    assert K.reference("edge_5x7_r8")["r"] == 8 and K.reference("c254_r0")["r"] == 0 and K.reference("r32")["r"] == 32
    pred, gt = K.inputs("checker")
    cnt = K.reference("checker")["counts"][0]
    assert cnt[0, 0] + cnt[1, 0] >= 2 * (pred.shape[1] * pred.shape[2] - pred.shape[1] - pred.shape[2] - 30)
    # a ground-truth label that is no class is not ignored: the prediction under it still has its boundaries
    k = K.CASES["labels65"]
    pred, gt = K.inputs("labels65")
    as_ignored = np.where((gt < 0) | (gt > 65), 65, gt)
    assert not np.array_equal(R.counts(pred, as_ignored, k["C"], k["ignore"], 2), K.reference("labels65")["counts"])
