#!/bin/bash
# the bench lines committed under profiles/ at the end of a round (GPU box): tools/final_bench.sh <output dir>
OUT=${1:?usage: tools/final_bench.sh <output dir>}
mkdir -p $OUT
python bench.py --full > $OUT/bench_r06_256_szel.json 2> $OUT/e1.txt
python bench.py --full --size 512 --no-cpu-baseline --no-extras > $OUT/bench_r06_512_szel_1gpu.json 2> $OUT/e2.txt
python bench.py --workload hydro > $OUT/bench_r06_hydro_2x128.json 2> $OUT/e3.txt
python bench.py --workload hydro --size 256 --sph pe > $OUT/bench_r06_hydro_2x256_pe_1gpu.json 2> $OUT/e4.txt
MPG_FORCE_MGPU=1 MASTER_ADDR=127.0.0.1 MASTER_PORT=29611 python bench.py --gpus 1 --no-cpu-baseline > $OUT/bench_r06_256_szel_1rank_rccl.json 2> $OUT/e5.txt
tail -c 600 $OUT/e*.txt; wc -c $OUT/*.json
