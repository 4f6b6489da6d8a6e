"""The auto-labelled coarse data path tests (tests/test_autolabel_gpu.py: ssa_autolabel_u8 through the C ABI, through
prepare_labels, read_labels and the centroid pass) on the CPU EMULATION build of the kernel sources, for both storage
builds -- as tests/test_uniform_emu_cpu.py runs the class-uniform tests -- so that the default CPU suite checks the chunk
walk with its partial chunks and load widths, the pair bit sets and their flush, the step walk with its gates and the
apply pass bit for bit against the restatement.  Only the graph capture and the full-size item skip under emulation
(the GPU runs them)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 39 cases through the C ABI, 7 through prepare_labels, 12 items through read_labels and the mixed list
MIN_PASSED = 59


@pytest.mark.parametrize("act", ["bf16", "fp16"])
def test_autolabel_on_the_emulated_kernels(act):
    env = dict(os.environ, SSA_EMU="1", SSA_ACT_DTYPE=act)
    env.pop("PYTEST_CURRENT_TEST", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_autolabel_gpu.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, "under SSA_EMU=1 SSA_ACT_DTYPE=%s:\n%s\n%s" % (act, tail, r.stderr[-2000:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) >= MIN_PASSED and "failed" not in tail, tail
