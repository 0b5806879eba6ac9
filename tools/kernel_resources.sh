#!/bin/bash
# Per-kernel register / spill / LDS / occupancy report of the engine source (compile-only, no GPU), with the
# build's own flags (build.py, -disable-machine-licm included). Only defines are accepted as arguments:
#   bash tools/kernel_resources.sh [-DNAME[=VALUE] ...]
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R && python -m crowdnav_dsrnn_amd.build --resources cn_engine.hip "$@"
