"""The class-uniform sampling tests (tests/test_uniform_gpu.py: ssa_class_centroids_u8 and ssa_pad_u8 through the C ABI
and through semseg_amd.datasets) on the CPU EMULATION build of the kernel sources, for both storage builds -- as
tests/test_relaxloss_emu_cpu.py runs the label relaxation tests -- so that the default CPU suite checks the chunk walk
with its partial chunks, the run merging, the wave tables and their flush, the tile order, the 64-bit sums and the
padding bit for bit against the restatement.  Only the graph capture skips under emulation (the GPU runs it)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 17 cases through the C ABI, 5 through class_centroids, the cache file, 7 paddings, 4 pairs through apply and the tail
MIN_PASSED = 34


@pytest.mark.parametrize("act", ["bf16", "fp16"])
def test_uniform_on_the_emulated_kernels(act):
    env = dict(os.environ, SSA_EMU="1", SSA_ACT_DTYPE=act)
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_uniform_gpu.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, "under SSA_EMU=1 SSA_ACT_DTYPE=%s:\n%s\n%s" % (act, tail, r.stderr[-2000:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) >= MIN_PASSED and "failed" not in tail, tail
