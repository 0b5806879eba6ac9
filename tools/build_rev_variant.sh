# diagnostic: the engine library as of a git revision, for A/B runs through CN_LIB_PATH (tools/ab_c2.sh, abn.sh)
#   bash tools/build_rev_variant.sh <rev> <name>   -> crowdnav_dsrnn_amd/lib/variants/libcn_<name>.so
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d /tmp/cnrev.XXXXXX)
# the revision's sources and every header it has, in sub-directories of csrc/ too
for f in $(git -C $R ls-tree -r --name-only $1 crowdnav_dsrnn_amd/csrc include); do
  mkdir -p $T/$(dirname $f) && git -C $R show $1:$f > $T/$f
done
cd $R && python -m crowdnav_dsrnn_amd.build --root $T --out $R/crowdnav_dsrnn_amd/lib/variants/libcn_$2.so --tag rev-$1
rm -rf $T
