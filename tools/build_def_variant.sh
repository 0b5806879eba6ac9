# diagnostic: the engine library of the working tree with extra defines, for A/B runs through CN_LIB_PATH
#   bash tools/build_def_variant.sh <name> "<-Dflags...>"   -> crowdnav_dsrnn_amd/lib/variants/libcn_<name>.so
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R && python -m crowdnav_dsrnn_amd.build --out $R/crowdnav_dsrnn_amd/lib/variants/libcn_$1.so --tag def-$1 $2
