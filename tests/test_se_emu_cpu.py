"""The exact tests of the squeeze-and-excitation gate and of the ceil-mode pool (tests/test_exact_se_gpu.py: ssa_se_*,
ssa_maxpool3x3s2c_*) on the CPU EMULATION build of the kernel sources, for both storage types -- as
tests/test_dwconv_emu_cpu.py runs the depthwise family -- so that the default CPU suite checks the split plan, the block
reductions, the gate's index arithmetic, the window clipping and the argument checks of the kernels.  The 2 M-element SE
case and the pool shape past the grid cap skip under emulation (the GPU runs them)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 6 of the 7 SE cases in three tests, the regime mirror, 16 of the 17 pool shapes, the two argument checks
MIN_PASSED = 37


@pytest.mark.parametrize("act", ["bf16", "fp16"])
def test_exact_se_on_the_emulated_kernels(act):
    env = dict(os.environ, SSA_EMU="1", SSA_ACT_DTYPE=act)
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_exact_se_gpu.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, "under SSA_EMU=1 SSA_ACT_DTYPE=%s:\n%s\n%s" % (act, tail, r.stderr[-2000:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) >= MIN_PASSED and "failed" not in tail, tail
