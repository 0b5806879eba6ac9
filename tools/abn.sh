# A/B/n: bench.py with each library in turn (CN_LIB_PATH; "tree" = the in-tree library), R rounds
#   bash tools/abn.sh <rounds> "<lib1> <lib2> ..." [bench args...]
# ABN_DUMP=1: every run also dumps its last outputs (bench.py --dump-outputs, into a temporary directory, or under
# ABN_DUMP_DIR), and each later dump is compared byte for byte with the first run's (exit 3 on a difference)
set -o pipefail
mkdir -p gpurun_out
R=$1; LIBS=$2; shift 2
BASE=("$@")
if [ -n "$ABN_DUMP" ]; then DD=${ABN_DUMP_DIR:-$(mktemp -d)}; mkdir -p $DD; fi
first=""
for k in $(seq 1 $R); do
  for L in $LIBS; do
    tag=$(basename $L .so)
    if [ "$L" = tree ]; then env_lib=""; else env_lib="CN_LIB_PATH=$L"; fi
    if [ -n "$ABN_DUMP" ]; then
      if [ -z "$first" ]; then first=$DD/first_${tag}; ddir=$first; else ddir=$DD/cur_${tag}; fi
      rm -rf $ddir; set -- "${BASE[@]}" --dump-outputs $ddir
    fi
    env $env_lib timeout -k 10 200 python -u bench.py --no-cpu-baseline "$@" > gpurun_out/abn_${tag}_$k.log 2>&1 || exit $?
    echo "$tag $(tail -1 gpurun_out/abn_${tag}_$k.log | python3 -c 'import json,sys; d=json.loads(sys.stdin.read()); print(d["value"], d["ms_per_step"])')"
    if [ -n "$ABN_DUMP" ] && [ "$ddir" != "$first" ]; then
      for f in $first/*.npy; do cmp -s $f $ddir/$(basename $f) || { echo "$tag round $k: $(basename $f) differs from the first run's"; exit 3; }; done
      echo "$tag round $k: outputs equal to the first run's"
    fi
  done
done
