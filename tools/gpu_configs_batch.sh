# bench lines for configs 3 / 4 / 5 and the batched config-2 / config-4 lines (1 GPU) on the current tree;
# writes under $VV_OUT/cfg (default bench_out/cfg), beside tools/gpu_configs.sh's lines
set -e
O=${VV_OUT:-bench_out}/cfg
bash tools/gpu_configs.sh
timeout -k 10 300 python bench.py --full --batch 8 --steps 1 --warmup 1 --no-cpu-baseline --no-exact-f32 --no-profile --no-config4 --no-config5 --no-sc4dvar > $O/c2_b8.json 2> $O/c2_b8.err
echo c2b8
timeout -k 10 400 python bench.py --full --config 4 --batch 8 --steps 1 --warmup 1 --no-cpu-baseline --no-exact-f32 --no-profile --no-sc4dvar > $O/c4_b8.json 2> $O/c4_b8.err
echo c4b8
