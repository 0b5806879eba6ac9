#!/bin/bash
# Per-kernel register / spill / LDS / occupancy report of the engine source (compile-only, no GPU), with the
# build's own flags (build.py, -disable-machine-licm included). Arguments are defines and, optionally, the sources
# to report instead of the engine's (names ending in .hip):
#   bash tools/kernel_resources.sh [SOURCE.hip ...] [-DNAME[=VALUE] ...]
R=$(cd "$(dirname "$0")/.." && pwd)
SRC=()
REST=()
for a in "$@"; do
    case "$a" in
        *.hip) SRC+=("$a") ;;
        *) REST+=("$a") ;;
    esac
done
[ ${#SRC[@]} -eq 0 ] && SRC=(cn_engine.hip)
cd $R && python -m crowdnav_dsrnn_amd.build --resources "${SRC[@]}" "${REST[@]}"
