# same-box A/B of two builds, alternating: REF=<path to the other .so> bash tools/gpu_ab_lib.sh TAG [bench args]
# (the config-3 headline with the config2 / config3 sub-records, sc4dvar and J); writes under $VV_OUT/TAG (default bench_out/TAG)
#   REF_TREE=<checkout of the other commit, built>  run the reference from its own tree instead (its Python with its
#            library: needed when the two libraries do not export the same entry points); REF is then not used
#   PAIRS=<n>                                        ref / new pairs (default 2)
#   AB_ARGS="..."                                    bench.py arguments in place of the default --full set
#   DUMP=1                                           every run also writes its --dump-outputs to ref_<i>.out / new_<i>.out
# Each run has its own time limit and a failing run ends the script.
set -e
T=${1:-ab}
shift || true
O=${VV_OUT:-bench_out}/$T
mkdir -p $O
O=$(cd $O && pwd)
HERE=$(pwd)
ARGS=${AB_ARGS:---full --no-cpu-baseline --no-profile --no-exact-f32 --no-config4 --no-config5 --steps 2}
for i in $(seq 1 ${PAIRS:-2}); do
  DR=${DUMP:+--dump-outputs $O/ref_$i.out}
  DN=${DUMP:+--dump-outputs $O/new_$i.out}
  if [ -n "$REF_TREE" ]; then
    (cd $REF_TREE && timeout -k 10 240 python bench.py $ARGS $DR "$@" > $O/ref_$i.json 2>/dev/null)
  else
    VAEVAR_LIB=$REF timeout -k 10 240 python bench.py $ARGS $DR "$@" > $O/ref_$i.json 2>/dev/null
  fi
  (cd $HERE && timeout -k 10 240 python bench.py $ARGS $DN "$@" > $O/new_$i.json 2>/dev/null)
done
