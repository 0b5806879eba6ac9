# diagnostic: libraries with compile-time variants of the unit cn_gru.hip (its sections: csrc/policy/*.h) (tools/probe_gru_seq.py via CN_LIB_PATH)
#   bash tools/build_gru_variants.sh name "-DGF_WPC=3 ..." [name "-D..."] ...
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
while [ $# -ge 2 ]; do
  n=$1; d=$(for x in $2; do echo "-Dcn_gru.hip:${x#-D}"; done); shift 2
  python -m crowdnav_dsrnn_amd.build --resources cn_gru.hip $d | grep fused_kernel | sed "s/\$/ <- $n/"
  python -m crowdnav_dsrnn_amd.build --out $R/crowdnav_dsrnn_amd/lib/variants/libcrowdnav_hip_$n.so $d
done
