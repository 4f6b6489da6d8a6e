"""The device RandomGaussianBlur (csrc/gblur.hip through semseg_amd.datasets) against the CPU restatement of the reference's
blur (tests/gblur_ref.py, pinned to SciPy and to the reference by tests/test_gblur_cpu.py) and against the fixture
tests/golden/gblur_golden.npz.  Every comparison is exact; neither SciPy nor the reference is needed here.  These are the
tests that can see a contracted multiply-add: the device has v_fma_f64 and hipcc forms it by default, the CPU emulation
build has no FMA target (with contraction forced into the emulation build, 392 of the 65536 pixels of the levels image
differ at sigma 0.3)."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import colorjit_ref as CR
import gblur_cases as K
import gblur_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_sigma_and_shape():
    K.check_sigmas_and_shapes(DEV)


def test_windows_smaller_than_the_radius():
    K.check_small_windows_at_radius_5(DEV)


def test_window_over_several_tiles():
    K.check_window_over_several_tiles(DEV)


def test_levels_image_at_every_radius():
    """Constant neighbourhoods at all 256 grey levels: where one ulp of the fp64 sum decides the byte."""
    K.check_levels(DEV, K.ONE_PER_RADIUS)


def test_reference_fixture():
    K.check_fixture_entries(DEV)


def test_random_gaussian_blur_call_with_the_recorded_seeds():
    from semseg_amd.datasets import RandomGaussianBlur
    inputs, outputs, meta = R.load_golden()
    for e, img, want in zip(meta["entries"], inputs, outputs):
        random.seed(e["seed"])
        got = RandomGaussianBlur()(torch.from_numpy(img).to(DEV))
        assert random.random() == e["random_after"]
        assert got.dtype == torch.uint8 and got.is_cuda and np.array_equal(got.cpu().numpy(), want), e["seed"]


def test_fused_normalise_equals_two_steps():
    K.check_fused_equals_two_steps(DEV)


def test_fused_normalise_on_the_other_storage_build():
    """The same test in a child process on the other build of the library (fp16 storage when this one is bf16)."""
    from semseg_amd import _lib
    other = "fp16" if _lib.ACT == "bf16" else "bf16"
    env = dict(os.environ, SSA_ACT_DTYPE=other)
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gblur_gpu.py"), "-k", "test_fused_normalise_equals_two_steps"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    tail = r.stdout[-3000:]
    assert r.returncode == 0, "fused blur tail under SSA_ACT_DTYPE=%s:\n%s\n%s" % (other, tail, r.stderr[-2000:])
    assert "1 passed" in tail, tail


def test_jitter_then_blur():
    K.check_jitter_then_blur(DEV)


def test_crop_flip_normalize_with_jitter_and_blur():
    """crop_flip_normalize(jitter=p, blur=b) == restatement(jitter) -> restatement(blur) -> the CPU normalise, cast to the
    loaded build's element type; the labels are those of the call without either."""
    from oracle.data import crop_flip_normalize as oracle
    from semseg_amd import _lib
    from semseg_amd.datasets import BlurParams, crop_flip_normalize
    from semseg_amd.datasets.transforms import MEAN_STD
    from util import ACT_DTYPE
    window = (7, 5, 2 * K.TILE_W + 5, K.TILE_H + 3)
    src = K.hostile_source(window, K.TILE_H + 3 + 11, 2 * K.TILE_W + 5 + 16)
    lab = np.random.RandomState(8).randint(0, 256, src.shape[:2]).astype(np.uint8)
    t, tl = torch.from_numpy(src).to(DEV), torch.from_numpy(lab).to(DEV)
    p = K.params(K.JITTER_DRAWS)
    for sigma in (0.3, 0.75, 1.2999):
        for flip in (False, True):
            for jitter in (None, p):
                _lib.lib().ssa_launch_count(1)
                out, gts = crop_flip_normalize(t, tl, window, flip, jitter=jitter, blur=BlurParams(sigma))
                assert _lib.lib().ssa_launch_count(0) == (2 if jitter is None else 4)   # (clear + luma sum,) blur tail, labels
                pre = src if jitter is None else CR.jitter(src, CR.program_of(K.JITTER_DRAWS), window, flip)
                u8 = R.blur(src, sigma, window, flip) if jitter is None else R.blur(pre, sigma)
                want_im, _ = oracle(u8, lab[:window[3], :window[2]], (0, 0, window[2], window[3]), False, *MEAN_STD)
                want = torch.from_numpy(want_im).permute(1, 2, 0).to(ACT_DTYPE).contiguous()
                got = out[0].cpu()
                assert out.dtype == ACT_DTYPE and tuple(out.shape) == (1, window[3], window[2], 16)
                assert torch.equal(got[..., :3].contiguous().view(torch.int16), want.view(torch.int16)), (sigma, flip)
                assert not got[..., 3:].view(torch.int16).any()
                assert torch.equal(gts, crop_flip_normalize(t, tl, window, flip)[1])


def test_captured_luma_sum_and_fused_tail_replay():
    """Luma sum + the fused jitter / blur / normalise launch captured in one linear graph, replayed after another image was
    copied into the same buffer: both times the bytes of the eager call on that image."""
    from semseg_amd.datasets import BlurParams, crop_flip_normalize
    window, flip = (7, 5, K.TILE_W + 5, K.TILE_H + 3), True
    a = K.hostile_source(window, K.TILE_H + 3 + 11, K.TILE_W + 5 + 16)
    b = (a // 3 + 150).astype(np.uint8)
    p, blur = K.params(K.JITTER_DRAWS), BlurParams(0.75)
    want_a = crop_flip_normalize(torch.from_numpy(a).to(DEV), None, window, flip, jitter=p, blur=blur)[0].clone()
    want_b = crop_flip_normalize(torch.from_numpy(b).to(DEV), None, window, flip, jitter=p, blur=blur)[0].clone()
    assert not torch.equal(want_a.view(torch.int16), want_b.view(torch.int16))
    buf = torch.from_numpy(a).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        crop_flip_normalize(buf, None, window, flip, jitter=p, blur=blur)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = crop_flip_normalize(buf, None, window, flip, jitter=p, blur=blur)[0]
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), want_a.view(torch.int16))
    buf.copy_(torch.from_numpy(b).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), want_b.view(torch.int16))
