"""The exact tests of the grouped 3x3 conv family (tests/test_exact_gconv_gpu.py: ssa_gconv3x3, ssa_gconv3x3_bwd) on the
CPU EMULATION build of the kernel sources, for both storage types -- as tests/test_dwconv_emu_cpu.py runs the depthwise
family -- so that the default CPU suite checks the MFMA fragment maps, the bounds of every tap, the block-diagonal filter,
the partial-tile reduce and the argument checks of the kernels.  The case of 2.1 M elements skips under emulation (the GPU
runs it)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 7 of the 8 cases forward and backward, the regime mirror, the 4 checks of the host reference, the argument checks
MIN_PASSED = 20


@pytest.mark.parametrize("act", ["bf16", "fp16"])
def test_exact_gconv_on_the_emulated_kernels(act):
    env = dict(os.environ, SSA_EMU="1", SSA_ACT_DTYPE=act)
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_exact_gconv_gpu.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, "under SSA_EMU=1 SSA_ACT_DTYPE=%s:\n%s\n%s" % (act, tail, r.stderr[-2000:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) >= MIN_PASSED and "failed" not in tail, tail
