# one --full bench line (+ optional extra args) and a rocprofv3 --stats profile of a short --full run; usage:
#   bash tools/gpu_bench.sh TAG [bench args...]     writes under $VV_OUT/TAG (default bench_out/TAG)
set -e
T=${1:-b}
shift || true
ROOT=$PWD
O=${VV_OUT:-bench_out}/$T
mkdir -p $O
O=$(cd $O && pwd)
timeout -k 10 600 python bench.py --full "$@" > $O/bench.json 2> $O/bench.err
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o run -- python3 $ROOT/bench.py --full --no-cpu-baseline --no-config4 --no-config5 --no-exact-f32 --no-profile --steps 2 --warmup 1 > $O/prof_bench.json 2> $O/prof.err
