# diagnostic library with in-kernel s_memtime stamps (tools/probe_stamps.py), same flags as build.py; add -DCN_LABEL_ROT=3
# as an argument for the rotated env ranges of "probe_stamps.py xcd 3"
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R && python -m crowdnav_dsrnn_amd.build --out $R/crowdnav_dsrnn_amd/lib/libcrowdnav_hip_stamps.so -DCN_STAMPS "$@"
