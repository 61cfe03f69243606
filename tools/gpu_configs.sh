# bench lines for BASELINE configs 3, 4, 5 (1 GPU, --full without the CPU baseline) + the 0.25-degree forecast timing;
# writes under $VV_OUT/cfg (default bench_out/cfg)
set -e
O=${VV_OUT:-bench_out}/cfg
mkdir -p $O
timeout -k 10 300 python bench.py --full --config 3 --no-cpu-baseline > $O/c3.json 2> $O/c3.err
echo c3
timeout -k 10 400 python bench.py --full --config 4 --no-cpu-baseline > $O/c4.json 2> $O/c4.err
echo c4
timeout -k 10 300 python bench.py --full --config 5 --steps 5 --no-cpu-baseline > $O/c5.json 2> $O/c5.err
echo c5
timeout -k 10 300 python tools/fcst_time.py > $O/fcst.log 2>&1
echo fcst
