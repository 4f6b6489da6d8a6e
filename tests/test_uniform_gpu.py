"""The class-uniform sampling kernels on the device: ssa_class_centroids_u8 (csrc/centroids.hip) and ssa_pad_u8
(csrc/pad_u8.hip) through the C ABI and through semseg_amd.datasets, bit for bit against tests/uniform_ref.py (which
tests/test_uniform_cpu.py pins to the real reference and to SciPy) on the cases of tests/uniform_cases.py; the files of
the reference's cache from PNGs on disk; RandomSizeAndCrop.apply + crop_flip_normalize against the bytes the reference
returned; a graph capture of the centroid call.

tests/test_uniform_emu_cpu.py runs this file on the CPU emulation of the kernel sources (the graph capture skips there:
the GPU runs it)."""
import collections
import json
import os
import random

import numpy as np
import pytest
import torch

import uniform_cases as K
import uniform_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
_EMU = bool(os.environ.get("SSA_EMU"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "uniform_golden.json")) as f:
        return json.load(f)


class _OnDevice(torch.Tensor):
    """A CPU tensor that answers is_cuda as a device tensor does: how the emulation, whose device memory is host memory,
    runs the public entry points that assert it."""
    is_cuda = property(lambda self: True)


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.as_subclass(_OnDevice) if DEV == "cpu" else t.to(DEV)


@pytest.fixture(autouse=True)
def _emu_stream(monkeypatch):
    if _EMU:
        monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: collections.namedtuple("S", "cuda_stream")(0))


_WANT = {}


def want(name):
    """(sums uint64 [N, tiles, C, 3], centroids int32 [N, tiles, C, 2]) of a case by the restatement; computed once."""
    if name not in _WANT:
        N, H, W, tile, C, id2trainid, _, _ = K.CASES[name]
        per = [R.centroid_table(m, tile, C, id2trainid) for m in K.label_maps(name)]
        _WANT[name] = (np.stack([p[0] for p in per]), np.stack([p[1] for p in per]))
    return _WANT[name]


def _labels(name):
    """The case's maps on the device, inside a wider buffer of other bytes where the case has a row stride."""
    N, H, W, _, _, _, extra, _ = K.CASES[name]
    maps = torch.from_numpy(K.label_maps(name).copy())
    if not extra:
        return maps.to(DEV)
    wide = torch.full((N, H, W + extra), 7, dtype=torch.uint8)
    wide[:, :, :W] = maps
    return wide.to(DEV)[:, :, :W]


@pytest.mark.parametrize("name", list(K.CASES))
def test_centroids_c_abi(name):
    from semseg_amd import _lib, hip_backend as hb
    N, H, W, tile, C, id2trainid, extra, _ = K.CASES[name]
    lab = _labels(name)
    assert lab.stride(1) == W + extra
    lut = torch.from_numpy(R.lut_of(id2trainid)).to(DEV) if id2trainid else None
    tiles = (H // tile) * (W // tile)
    # (one spare element behind each output: an image without tiles still hands over valid pointers, and nothing is written)
    sums_buf = torch.full((N * tiles * C * 3 + 1,), -1, dtype=torch.int64, device=DEV)       # the call clears them itself
    cent_buf = torch.full((N * tiles * C * 2 + 1,), -7, dtype=torch.int32, device=DEV)
    sums, cent = sums_buf[:-1].view(N, tiles, C, 3), cent_buf[:-1].view(N, tiles, C, 2)
    rc = _lib.lib().ssa_class_centroids_u8(hb._p(lab), N, H, W, W + extra, tile, C, hb._p(lut), hb._p(sums_buf), hb._p(cent_buf),
                                           hb._s())
    assert rc == 0
    torch.cuda.synchronize()
    assert int(sums_buf[-1]) == -1 and int(cent_buf[-1]) == -7
    w_sums, w_cent = want(name)
    assert w_sums.shape == tuple(sums.shape) and w_cent.shape == tuple(cent.shape)
    assert np.array_equal(sums.cpu().numpy().view(np.uint64), w_sums), name
    assert np.array_equal(cent.cpu().numpy(), w_cent), name
    if name.startswith("full"):         # beyond a signed, then beyond any 32-bit sum
        assert int(w_sums[0, 0, 5, 1]) == tile * (tile * (tile - 1) // 2) > (1 << 31 if tile == 2048 else 1 << 32)
    if name == "no_tiles":
        assert tiles == 0


@pytest.mark.parametrize("name", ["t16_lut_n3", "t16_ld", "t64_c65", "no_tiles", "c256_lut"])
def test_class_centroids(name):
    from semseg_amd.datasets import class_centroids
    N, H, W, tile, C, id2trainid, extra, _ = K.CASES[name]
    lab = _labels(name)
    got = class_centroids(lab, tile, C, id2trainid)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want(name)[1])
    one = class_centroids(lab[N - 1], tile, C, id2trainid)                       # [H, W], strided where the case is
    assert one.dim() == 3 and np.array_equal(one.cpu().numpy(), want(name)[1][N - 1])
    strided = torch.stack([lab, lab], -1)[..., 0]                                # pixel stride 2: copied
    assert strided.stride(2) == 2
    assert np.array_equal(class_centroids(strided, tile, C, id2trainid).cpu().numpy(), want(name)[1])


def test_cache_file_from_pngs(golden, tmp_path, monkeypatch):
    """build_centroids over PNGs on disk writes the reference's file, byte for byte; per-image dicts in tile order."""
    from PIL import Image
    from semseg_amd.config import cfg
    from semseg_amd.datasets import build_centroids, class_centroids_image, uniform as U
    monkeypatch.chdir(tmp_path)
    if _EMU:
        monkeypatch.setattr(U, "DEVICE", "cpu")
    items = [K.file_names(n, i) for n in K.JSON_SET for i in range(K.CASES[n][0])]
    maps = [K.label_maps(n)[i] for n in K.JSON_SET for i in range(K.CASES[n][0])]
    items.append((K.JSON_BIG[0] + "_leftImg8bit.png", K.JSON_BIG[0] + "_labelIds.png"))
    maps.append(K.json_big_map())
    for (_, label_fn), m in zip(items, maps):
        Image.fromarray(np.asarray(m)).save(label_fn)
    saved = dict(cfg.DATASET)
    cfg.DATASET.update(CENTROID_ROOT="centroid_cache", NAME="toy", CLASS_UNIFORM_TILE=512, CLASS_UNIFORM_PCT=0.5)
    copies = []
    real = U.class_centroids
    monkeypatch.setattr(U, "class_centroids", lambda labels, *a, **k: (copies.append(tuple(labels.shape)), real(labels, *a, **k))[1])
    try:
        got = build_centroids(items, K.JSON_CLASSES, True, cv=0, id2trainid=K.TWO_ONTO_ONE)
        assert open(os.path.join("centroid_cache", golden["json_name"])).read() == golden["json_text"]
        assert json.dumps(got, indent=4) == golden["json_text"]
        again = build_centroids(items, K.JSON_CLASSES, True, cv=0)              # now from the file
        assert again == {int(k): v for k, v in json.loads(golden["json_text"]).items()}
    finally:
        cfg.DATASET.clear()
        cfg.DATASET.update(saved)
    # the six maps have three sizes: three calls, one copy back each
    assert sorted(copies) == sorted([(4, 37, 53), (1, 19, 29), (1,) + K.json_big_map().shape]), copies
    name = "t16_lut_n3"
    N, H, W, tile, C, id2trainid, _, _ = K.CASES[name]
    d = class_centroids_image(K.file_names(name, 1), tile, C, id2trainid)
    assert dict(d) == dict(R.as_dict(K.file_names(name, 1), want(name)[1][1])) and list(d) == list(
        R.as_dict(K.file_names(name, 1), want(name)[1][1]))
    d2 = class_centroids_image(K.file_names(name, 1), tile, C, id2trainid, labels=_labels(name)[1])
    assert dict(d2) == dict(d)


@pytest.mark.parametrize("shape,lrtb,fill", [((13, 21), (3, 0, 7, 5), 255), ((13, 21, 3), (3, 0, 7, 5), (9, 0, 200)),
                                             ((5, 17), (0, 0, 0, 0), 4), ((5, 17, 3), (0, 0, 0, 0), (1, 2, 3)),
                                             ((40, 37, 3), (14, 9, 14, 9), (0, 0, 0)), ((1, 1), (0, 2, 1, 0), 19),
                                             ((300, 517, 3), (1, 0, 0, 2), (0, 0, 0))])
def test_pad(shape, lrtb, fill):
    from semseg_amd.datasets import pad_u8
    src = np.random.RandomState(sum(shape)).randint(0, 256, shape).astype(np.uint8)
    got = pad_u8(_dev(src), lrtb, fill)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), R.pad(src, lrtb, fill))


def _plan_dict(p):
    return {"scale_amt": p.scale_amt, "size": list(p.size), "border": list(p.border), "margins": list(p.margins),
            "window": list(p.window), "state": K.py_state_digest()}


@pytest.mark.parametrize("n", range(len(K.PAIRS)))
def test_apply_and_tail_against_the_reference_bytes(golden, n):
    """The pair RandomSizeAndCrop returned in the reference, from the device: resize, pad (cases 0, 2, 3), crop."""
    from oracle.data import crop_flip_normalize as oracle
    from semseg_amd.config import cfg
    from semseg_amd.datasets import RandomSizeAndCrop, crop_flip_normalize
    from semseg_amd.datasets.transforms import MEAN_STD
    from util import ACT_DTYPE
    seed, crop_size, (smin, smax), taf, size, centroid = K.PAIRS[n]
    e = golden["pairs"][n]
    img, lab = K.pair(seed, size)
    saved = cfg.DATASET.TRANSLATE_AUG_FIX
    cfg.DATASET.TRANSLATE_AUG_FIX = taf
    try:
        t = RandomSizeAndCrop(crop_size, False, scale_min=smin, scale_max=smax)
        random.seed(seed)
        plan = t.get_params(size, centroid)
    finally:
        cfg.DATASET.TRANSLATE_AUG_FIX = saved
    assert _plan_dict(plan) == {k: v for k, v in e.items() if k not in ("img", "lab")}
    assert any(plan.pad) == (n != 1)
    d_img, d_lab, window = t.apply(plan, _dev(img), _dev(lab))
    x0, y0, cw, ch = window
    want_img = np.frombuffer(bytes.fromhex(e["img"]), dtype=np.uint8).reshape(ch, cw, 3)
    want_lab = np.frombuffer(bytes.fromhex(e["lab"]), dtype=np.uint8).reshape(ch, cw)
    assert np.array_equal(d_img.cpu().numpy()[y0:y0 + ch, x0:x0 + cw], want_img)
    assert np.array_equal(d_lab.cpu().numpy()[y0:y0 + ch, x0:x0 + cw], want_lab)
    if DEV == "cpu":
        d_img, d_lab = d_img.as_subclass(_OnDevice), d_lab.as_subclass(_OnDevice)
    for flip in (False, True):
        out, gts = crop_flip_normalize(d_img, d_lab, window, flip)
        w_im, w_lab = oracle(want_img, want_lab, (0, 0, cw, ch), flip, *MEAN_STD)
        w_im = torch.from_numpy(w_im).permute(1, 2, 0).to(ACT_DTYPE).contiguous()
        assert torch.equal(out[0].cpu()[..., :3].contiguous().view(torch.int16), w_im.view(torch.int16))
        assert torch.equal(gts[0].cpu(), torch.from_numpy(w_lab))


def test_centroids_under_graph_capture():
    """One capture, replayed over two label maps written into the same buffer: no allocation, no synchronisation."""
    if _EMU:
        pytest.skip("graph capture needs the device")
    from semseg_amd import _lib, hip_backend as hb
    name = "t16_lut_n3"
    N, H, W, tile, C, id2trainid, _, _ = K.CASES[name]
    maps = K.label_maps(name)
    lab = torch.zeros((1, H, W), dtype=torch.uint8, device=DEV)
    lut = torch.from_numpy(R.lut_of(id2trainid)).to(DEV)
    tiles = (H // tile) * (W // tile)
    sums = torch.zeros((1, tiles, C, 3), dtype=torch.int64, device=DEV)
    cent = torch.zeros((1, tiles, C, 2), dtype=torch.int32, device=DEV)
    L = _lib.lib()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert L.ssa_class_centroids_u8(hb._p(lab), 1, H, W, W, tile, C, hb._p(lut), hb._p(sums), hb._p(cent), hb._s()) == 0
    torch.cuda.current_stream().wait_stream(side)
    for i in (0, 2):
        lab.copy_(torch.from_numpy(maps[i:i + 1].copy()))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(cent.cpu().numpy()[0], want(name)[1][i])
        assert np.array_equal(sums.cpu().numpy().view(np.uint64)[0], want(name)[0][i])
