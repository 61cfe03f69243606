# same-box A/B of two library builds: REF=<path to the other .so> bash tools/gpu_ab_lib.sh TAG [bench args]
# (the config-3 headline with the config2 / config3 sub-records, sc4dvar and J); writes under $VV_OUT/TAG (default bench_out/TAG)
set -e
T=${1:-ab}
shift || true
O=${VV_OUT:-bench_out}/$T
mkdir -p $O
for i in 1 2; do
  VAEVAR_LIB=$REF timeout -k 10 240 python bench.py --full --no-cpu-baseline --no-profile --no-exact-f32 --no-config4 --no-config5 --steps 2 "$@" > $O/ref_$i.json 2>/dev/null
  timeout -k 10 240 python bench.py --full --no-cpu-baseline --no-profile --no-exact-f32 --no-config4 --no-config5 --steps 2 "$@" > $O/new_$i.json 2>/dev/null
done
