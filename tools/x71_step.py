#!/usr/bin/env python
"""One training step of deepv3.DeepV3PlusX71 (network/deepv3.py:117: the Xception-71 trunk; 800 x 800 crop, cross entropy,
SGD) on the device: tools/wrn38_step.py with this architecture as the default of --arch; same options, same JSON record.
    python tools/x71_step.py [--crop 800] [--batch 1] [--steps 10] [--warmup 3] [--eager] [--json FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/x71_step.py --steps 3 --warmup 1 --eager"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wrn38_step  # noqa: E402

if __name__ == "__main__":
    wrn38_step.main("deepv3.DeepV3PlusX71")
