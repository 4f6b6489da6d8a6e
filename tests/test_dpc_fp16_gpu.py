"""The rectangular-dilation conv family and the Dense Prediction Cell on the fp16-storage build (lib/libsemseg_hip_f16.so,
SSA_ACT_DTYPE=fp16), in the way tests/test_fp16_storage_gpu.py runs the other kernels on it: the same test files in a
child process, whose tests/util.py rounds inputs and references to the product's format.  The exact tests of
csrc/conv_dil.hip bit for bit, the cell op by op against the fp16 storage floor, and the new route against the existing
one at a square dilation.  (Training a network on this build needs the loss scaler: tests/test_amp_fp16_gpu.py.)"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dilconv_and_cell_on_the_fp16_build():
    env = dict(os.environ, SSA_ACT_DTYPE="fp16")
    env.pop("PYTEST_CURRENT_TEST", None)
    args = ["tests/test_exact_dilconv_gpu.py", "tests/test_dpc_gpu.py", "-k", "dilconv or cell or square"]
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-s"] + args,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout)                     # (the child's figures, with -s)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, "%s under SSA_ACT_DTYPE=fp16:\n%s\n%s" % (args, tail, r.stderr[-2000:])
    assert "23 passed" in tail and " failed" not in tail and " skipped" not in tail, tail
