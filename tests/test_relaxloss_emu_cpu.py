"""The label relaxation tests (tests/test_relaxloss_gpu.py: the kernels of csrc/relax_loss.hip through the C ABI, through
RelaxNllFn, the criterion and the public transform) on the CPU EMULATION build of the kernel sources, for both storage
builds -- as tests/test_dwconv_emu_cpu.py runs the depthwise conv tests -- so that the default CPU suite checks the
stencil's halo and tile seams, the class-set words, every integer count, the class weights, the loss and its gradient
against the golden data of the real reference, and the argument checks.  The graph capture and the 1024 x 1024 run skip
under emulation (the GPU runs them)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 8 cases through the C ABI, 8 through RelaxNllFn, 2 sliced, 2 on the multi-hot target, criterion, launch budget,
# transform, arguments
MIN_PASSED = 24


@pytest.mark.parametrize("act", ["bf16", "fp16"])
def test_relaxloss_on_the_emulated_kernels(act):
    env = dict(os.environ, SSA_EMU="1", SSA_ACT_DTYPE=act)
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_relaxloss_gpu.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, "under SSA_EMU=1 SSA_ACT_DTYPE=%s:\n%s\n%s" % (act, tail, r.stderr[-2000:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) >= MIN_PASSED and "failed" not in tail, tail
