"""Run a tool / bench.py against an experiment build of the library (tools/expbuild.sh):
python tools/libvariant.py <name> <script.py> [args...]   -> lib/libsemseg_hip_<name>.so
(fp16 storage, SSA_ACT_DTYPE=fp16 in the environment: lib/libsemseg_hip_f16_<name>.so; bench.py's own default of fp16 is
set after this module has chosen the library, so name the storage format explicitly)"""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-segmentation_amd")):
    sys.path.insert(0, p)
from semseg_amd import _lib  # noqa: E402

name, script = sys.argv[1], sys.argv[2]
_lib.LIB_PATH = _lib.LIB_PATH[:-len(".so")] + "_%s.so" % name
sys.argv = [script] + sys.argv[3:]
runpy.run_path(script, run_name="__main__")
