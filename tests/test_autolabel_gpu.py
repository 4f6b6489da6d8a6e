"""The auto-labelled coarse data path on the device: ssa_autolabel_u8 (csrc/autolabel.hip) through the C ABI, through
prepare_labels and read_labels (PNGs on disk) and through the centroid pass of semseg_amd.datasets.uniform, bit for bit
against tests/autolabel_ref.py (which tests/test_autolabel_cpu.py pins to the real reference) on the cases of
tests/autolabel_cases.py; one graph capture replayed on two inputs whose presence bits differ.

tests/test_autolabel_emu_cpu.py runs this file on the CPU emulation of the kernel sources (the graph capture and the
full-size item skip there: the GPU runs them)."""
import collections
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import autolabel_cases as K
import autolabel_ref as R
import uniform_ref as UR

pytestmark = pytest.mark.gpu

DEV = "cuda"
_EMU = bool(os.environ.get("SSA_EMU"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "autolabel_golden.json")) as f:
        return json.load(f)


@pytest.fixture(autouse=True)
def _emu_stream(monkeypatch):
    if _EMU:
        from semseg_amd.datasets import autolabel as A, uniform as U
        monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: collections.namedtuple("S", "cuda_stream")(0))
        monkeypatch.setattr(A, "DEVICE", "cpu")
        monkeypatch.setattr(U, "DEVICE", "cpu")


@pytest.fixture()
def coarse_cfg():
    from semseg_amd.config import cfg
    saved, saved_boost = dict(cfg.DATASET), cfg.DROPOUT_COARSE_BOOST_CLASSES
    cfg.DATASET.update(CITYSCAPES_CUSTOMCOARSE=K.CUSTOMCOARSE, CITYSCAPES_DIR=K.CITYSCAPES_DIR)
    yield cfg
    cfg.DATASET.clear()
    cfg.DATASET.update(saved)
    cfg.DROPOUT_COARSE_BOOST_CLASSES = saved_boost


_WANT = {}


def want(name):
    """uint8 [N, H, W] of a kernel case by the restatement; computed once."""
    if name not in _WANT:
        c = K.KERNEL[name]
        o, g, p = K.inputs(name)
        _WANT[name] = R.merge_batch(o, g if c["coarse"] else None, p if c["cut"] else None, c["steps"], c["mode"], c["window"],
                                    c["cut"], c["ignore"])
        _WANT[name].setflags(write=False)
    return _WANT[name]


def _wide(a, extra, fill):
    """The maps on the device, inside a wider buffer of other bytes where the case has a row stride."""
    t = torch.from_numpy(np.array(a))
    if not extra:
        return t.to(DEV)
    N, H, W = t.shape
    wide = torch.full((N, H, W + extra), fill, dtype=torch.uint8)
    wide[:, :, :W] = t
    return wide.to(DEV)[:, :, :W]


def _steps_bytes(steps):
    return bytes(b for s in steps for b in s)


@pytest.mark.parametrize("name", list(K.KERNEL))
def test_autolabel_c_abi(name):
    from semseg_amd import _lib, hip_backend as hb
    c = K.KERNEL[name]
    N, H, W = c["N"], c["H"], c["W"]
    el, ec, ep, eo = c["extra"]
    o, g, p = K.inputs(name)
    lab = _wide(o, el, 27)                           # what lies between the rows would merge and be merged if it were read
    coarse = _wide(g, ec, 28) if c["coarse"] else None
    prob = _wide(p, ep, 0) if c["cut"] else None
    assert lab.stride(1) == W + el
    out_buf = torch.full((N * H * (W + eo) + 16,), 99, dtype=torch.uint8, device=DEV)
    out = out_buf[:N * H * (W + eo)].view(N, H, W + eo)
    pairs = torch.full((N * 2048 + 1,), -1, dtype=torch.int32, device=DEV)          # the call clears them itself
    table = torch.full((N * 65536 + 16,), 77, dtype=torch.uint8, device=DEV)
    x0, y0, x1, y1 = c["window"] or (0, 0, 0, 0)
    rc = _lib.lib().ssa_autolabel_u8(hb._p(lab), hb._p(coarse), hb._p(prob), N, H, W, W + el, W + ec, W + ep,
                                     _steps_bytes(c["steps"]), len(c["steps"]), 1 if c["mode"] == "current" else 0, x0, y0, x1, y1,
                                     c["cut"], c["ignore"], hb._p(pairs), hb._p(table), hb._p(out_buf), W + eo, hb._s())
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :, :W], want(name)), name
    assert (got[:, :, W:] == 99).all() and (out_buf[-16:] == 99).all()              # nothing outside the rows
    assert int(pairs[-1]) == -1 and (table[-16:] == 77).all()
    # the workspaces: exactly the pairs that occur, and their values; the entry of a pair that does not occur is not written
    keep = np.zeros((H, W), dtype=bool)
    keep[y0:y1, x0:x1] = True
    o_eff = np.where(keep[None], o, 0) if c["window"] else o
    g_eff = g if c["coarse"] else np.zeros_like(g)
    bits = np.unpackbits(pairs[:-1].cpu().numpy().view(np.uint8).reshape(N, 8192), axis=1, bitorder="little").astype(bool)
    tab = table[:-16].view(N, 65536).cpu().numpy()
    for i in range(N):
        occur = np.zeros(65536, dtype=bool)
        occur[o_eff[i].astype(np.int64) * 256 + g_eff[i]] = True
        assert np.array_equal(bits[i], occur), name
        assert (tab[i][~occur] == 77).all(), name
        mapped = want(name)[i] if not c["cut"] else R.merge(o[i], g_eff[i], None, c["steps"], c["mode"], c["window"])
        assert np.array_equal(tab[i][o_eff[i].astype(np.int64) * 256 + g_eff[i]], mapped), name


@pytest.mark.parametrize("name", ["3x37_ld_all", "64x80_ld_l", "h1_ld", "n3_one_image_current", "city_original", "no_steps_current",
                                  "all256_current"])
def test_prepare_labels(name):
    from semseg_amd.datasets import prepare_labels
    c = K.KERNEL[name]
    N, H, W = c["N"], c["H"], c["W"]
    el, ec, ep, _ = c["extra"]
    o, g, p = K.inputs(name)
    lab, coarse, prob = _wide(o, el, 27), _wide(g, ec, 28) if c["coarse"] else None, _wide(p, ep, 0) if c["cut"] else None
    steps = _steps_bytes(c["steps"])
    kw = dict(window=c["window"], prob_cut=c["cut"], ignore_label=c["ignore"])
    got = prepare_labels(lab, coarse, prob, steps, c["mode"], **kw)
    assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(got.cpu().numpy(), want(name))
    pick = lambda t: None if t is None else t[N - 1]                              # noqa: E731  [H, W], strided where the case is
    one = prepare_labels(pick(lab), pick(coarse), pick(prob), steps, c["mode"], **kw)
    assert one.dim() == 2 and np.array_equal(one.cpu().numpy(), want(name)[N - 1])
    strided = torch.stack([lab, lab], -1)[..., 0]                                  # pixel stride 2: copied
    assert strided.stride(2) == 2
    assert np.array_equal(prepare_labels(strided, coarse, prob, steps, c["mode"], **kw).cpu().numpy(), want(name))


@pytest.mark.parametrize("name", [n for n in K.ITEMS])
def test_read_labels_from_pngs(golden, coarse_cfg, tmp_path, monkeypatch, name):
    """The loader's label of every item, from the files: equal to the restatement, and for the full-size item -- the
    reference's own drop mask on the reference's own size -- to the SHA-256 of what the real reference returned."""
    if _EMU and name == "full":
        pytest.skip("the full-size item runs on the device")
    from semseg_amd.datasets import read_labels
    cfg = coarse_cfg
    path, (H, W), ids, st = K.ITEMS[name]
    monkeypatch.chdir(tmp_path)
    K.write_tree([name])
    cfg.DROPOUT_COARSE_BOOST_CLASSES = st["boost"]
    cfg.DATASET.update(MASK_OUT_CITYSCAPES=st["mask_out"], CUSTOM_COARSE_PROB=st["prob"])
    got = read_labels(path, K.ID_MAPS[ids])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (H, W) and got.is_contiguous()
    o, g, p = K.item_maps(name)
    expect = R.loader_labels(path, o, g, p, K.ID_MAPS[ids], K.CUSTOMCOARSE, st["boost"], st["mask_out"], st["prob"])
    assert np.array_equal(got.cpu().numpy(), expect)
    if name == "full":
        assert hashlib.sha256(got.cpu().numpy().tobytes()).hexdigest() == golden["labels"]["full"]["sha256"]


def test_centroids_of_a_mixed_list(golden, coarse_cfg, tmp_path, monkeypatch):
    """pooled_class_centroids_all over auto-labelled and plain items of two sizes: the reference's centroids, one merge
    call per group of auto-labelled maps of one size, one centroid call per group."""
    from semseg_amd.datasets import class_centroids_image, pooled_class_centroids_all, uniform as U
    cfg = coarse_cfg
    monkeypatch.chdir(tmp_path)
    files = K.write_tree(K.CENTROID_LIST + K.CENTROID_CHAIN)
    calls = []
    real_prepare, real_cent = U.prepare_labels, U.class_centroids
    monkeypatch.setattr(U, "prepare_labels", lambda labels, coarse, prob, steps, mode, **k: (
        calls.append(("merge", tuple(labels.shape), coarse is not None, prob, mode)), real_prepare(labels, coarse, prob, steps, mode, **k))[1])
    monkeypatch.setattr(U, "class_centroids", lambda labels, tile, C, id2trainid=None: (
        calls.append(("centroids", tuple(labels.shape), id2trainid is not None)), real_cent(labels, tile, C, id2trainid))[1])
    for key, names, ids, boost in (("list", K.CENTROID_LIST, "CITY", K.CITY_BOOST), ("chain", K.CENTROID_CHAIN, "CHAIN", K.CHAIN_BOOST)):
        cfg.DROPOUT_COARSE_BOOST_CLASSES = boost
        items = [files[n] for n in names]
        del calls[:]
        got = pooled_class_centroids_all(items, K.CENTROID_CLASSES, K.ID_MAPS[ids], K.CENTROID_TILE)
        index = {it[1]: i for i, it in enumerate(items)}
        assert [[int(c), [[index[e[1]], int(e[2][0]), int(e[2][1])] for e in got[c]]] for c in got] == golden["centroids"][key]
        assert all(e[0] == items[index[e[1]]][0] and e[3] == c for c in got for e in got[c])
        if key == "list":
            assert calls == [("merge", (3, 37, 53), True, None, "original"), ("centroids", (3, 37, 53), False),
                             ("centroids", (1, 37, 53), True),
                             ("merge", (1, 19, 29), True, None, "original"), ("centroids", (1, 19, 29), False),
                             ("centroids", (2, 19, 29), True)], calls
    # one image, as the reference's class_centroids_image: from the files, and from maps the caller holds
    cfg.DROPOUT_COARSE_BOOST_CLASSES = K.CITY_BOOST
    item = files["refine"]
    d = class_centroids_image(item, K.CENTROID_TILE, K.CENTROID_CLASSES, K.CITY)
    o, g, _ = K.item_maps("refine")
    d2 = class_centroids_image(item, K.CENTROID_TILE, K.CENTROID_CLASSES, K.CITY, labels=torch.from_numpy(np.array(o)).to(DEV),
                               coarse=torch.from_numpy(np.array(g)).to(DEV))
    assert dict(d) == dict(d2) and list(d) == list(d2)
    m = R.centroid_labels(item[1], o, g, K.CITY, K.CUSTOMCOARSE, K.CITY_BOOST)
    want_d = UR.as_dict(item, UR.centroid_table(m, K.CENTROID_TILE, K.CENTROID_CLASSES)[1])
    assert dict(d) == dict(want_d) and list(d) == list(want_d)


def test_autolabel_under_graph_capture():
    """One capture, replayed over two inputs written into the same buffers whose presence bits differ: image 0 of the
    one-image batch lacks the boosted id and image 1 has it, so the pair set and the table must follow the data, not
    the capture."""
    if _EMU:
        pytest.skip("graph capture needs the device")
    from semseg_amd import _lib, hip_backend as hb
    name = "n3_one_image_current"
    c = K.KERNEL[name]
    H, W = c["H"], c["W"]
    o, g, p = K.inputs(name)
    lab = torch.zeros((1, H, W), dtype=torch.uint8, device=DEV)
    coarse = torch.zeros((1, H, W), dtype=torch.uint8, device=DEV)
    out = torch.zeros((1, H, W), dtype=torch.uint8, device=DEV)
    pairs = torch.zeros((1, 2048), dtype=torch.int32, device=DEV)
    table = torch.zeros((1, 65536), dtype=torch.uint8, device=DEV)
    steps = _steps_bytes(c["steps"])
    L = _lib.lib()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert L.ssa_autolabel_u8(hb._p(lab), hb._p(coarse), None, 1, H, W, W, W, 0, steps, len(c["steps"]), 1, 0, 0, 0, 0, 0,
                                      255, hb._p(pairs), hb._p(table), hb._p(out), W, hb._s()) == 0
    torch.cuda.current_stream().wait_stream(side)
    tables = []
    for i in (0, 1, 0):
        lab.copy_(torch.from_numpy(o[i:i + 1].copy()))
        coarse.copy_(torch.from_numpy(g[i:i + 1].copy()))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy()[0], want(name)[i])
        tables.append(table.cpu().numpy().copy())
    # the pair (26, 28) -- o has road-side 26 where g has the boosted 28 -- is in all three images: merged only in image 1
    # (entries of pairs that do not occur keep what an earlier replay left there: only the pairs of the image are compared)
    assert [t[0, 26 * 256 + 28] for t in tables] == [13, 15, 13]
    occur = np.unique(o[0].astype(np.int64) * 256 + g[0])
    assert np.array_equal(tables[0][0, occur], tables[2][0, occur])
