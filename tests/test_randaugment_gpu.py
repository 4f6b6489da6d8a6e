"""RandAugment on the device: the cases of tests/randaug_cases.py (the same functions tests/test_randaugment_cpu.py runs
on the CPU emulation) against the restatement of tests/randaug_ref.py, byte for byte -- here the device's own arithmetic
is under test: fp64 and fp32 sums that must not contract into FMAs, the fp64 division of AutoContrast, the LDS and global
atomics of the histogram.  Then the whole tail against its steps in sequence, and one graph capture replayed on two
images."""
import numpy as np
import pytest
import torch

import randaug_cases as K
import randaug_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


def test_every_op_on_the_fixture_images():
    assert K.check_every_op_on_the_fixture_images(DEV) == 95


def test_tables_and_point_ops_on_special_images():
    assert K.check_table_ops_on_special_images(DEV) == 20


def test_sharpness_images():
    assert K.check_sharpness_images(DEV) == 6


def test_label_translations():
    assert K.check_label_translations(DEV) == 106


def test_reference_fixture_chains():
    assert K.check_fixture_chains(DEV) == 32


def test_window_inside_a_larger_source():
    assert K.check_window_inside_a_larger_source(DEV) == 18


def test_window_over_several_tiles():
    assert K.check_window_over_several_tiles(DEV) == 12


def test_tiny_windows():
    assert K.check_tiny_windows(DEV) == 36


def test_labels_absent():
    assert K.check_labels_absent(DEV) == 9


def test_fused_tail_equals_the_steps_in_sequence():
    assert K.check_tail_equals_steps_in_sequence(DEV) == 4


def test_graph_capture_of_histogram_chain_and_tail_replayed_on_two_images():
    """One torch.cuda.graph over the clearing of the histogram, the chain (a warp of both buffers, Equalize with its
    histogram and table, the stencil), the jitter with its luma sum and the normalising tail; replayed on two different
    source images copied into the captured buffers: the right result each time, so the histogram and the counter are
    cleared inside the graph and nothing in it depends on the host."""
    import colorjit_ref as CR
    import gblur_cases as GK
    from semseg_amd.datasets import crop_flip_normalize
    window = (7, 5, K.TILE_W + 5, K.TILE_H + 3)
    H, W = K.TILE_H + 3 + 11, K.TILE_W + 5 + 16
    program = [("Rotate", 11.0), ("Equalize", 0.0), ("Sharpness", 0.1)]
    p, jitter = K.params(program, window[2], window[3]), GK.params(GK.JITTER_DRAWS)
    sources = [K.hostile_source(window, H, W, seed) for seed in (3, 4)]
    img = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
    lab = torch.zeros((H, W), dtype=torch.uint8, device=DEV)
    img.copy_(torch.from_numpy(sources[0][0]))
    lab.copy_(torch.from_numpy(sources[0][1]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # one eager run first: allocations and tables settle outside
        crop_flip_normalize(img, lab, window, True, jitter=jitter, augment=p)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, gts = crop_flip_normalize(img, lab, window, True, jitter=jitter, augment=p)
    n = 0
    for src, lb in (sources[1], sources[0]):
        img.copy_(torch.from_numpy(src))
        lab.copy_(torch.from_numpy(lb))
        g.replay()
        torch.cuda.synchronize()
        wi, wl = R.augment(src, lb, program, window, True)
        want_u8 = CR.jitter(wi, CR.program_of(GK.JITTER_DRAWS))
        eager, _ = crop_flip_normalize(torch.from_numpy(want_u8).to(DEV), None, (0, 0, window[2], window[3]), False)
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16)), n
        assert np.array_equal(gts.cpu().numpy()[0], wl.astype(np.int64)), n
        n += 1
    assert n == 2
