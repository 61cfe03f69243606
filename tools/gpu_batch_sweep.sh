# analyses per GPU B = 1, 2, 4, 8 for config 2 and config 4 (one GPU); usage: bash tools/gpu_batch_sweep.sh TAG
# writes under $VV_OUT/TAG (default bench_out/TAG)
set -e
T=${1:-bsw}
O=${VV_OUT:-bench_out}/$T
mkdir -p $O
for B in 1 2 4 8; do
  timeout -k 10 300 python bench.py --config 2 --batch $B --steps 1 --warmup 1 > $O/c2_b$B.json 2> $O/c2_b$B.err
done
for B in 1 2 4 8; do
  timeout -k 10 400 python bench.py --config 4 --batch $B --steps 1 --warmup 1 > $O/c4_b$B.json 2> $O/c4_b$B.err
done
