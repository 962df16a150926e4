# Round evidence, part 3 (run on the GPU box from the repo root; NVO_COMMIT = the commit the tree was built from): the
# occupancy-grid back-end after the second half of round 4 -- profiled step + 1200x680 inference, rocprofv3 kernel
# statistics of the graph-replayed steps, HBM traffic (FETCH_SIZE / WRITE_SIZE in separate passes), the driver-style line.
# Outputs under $OUT.
set -x
R=${ROUND:-r4}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${OUT:?set OUT to the directory for the outputs}" && cd "$OUT" && pwd)
python tools/ngp_bench.py --steps 300 --profile --render-frames 3 > $OUT/${R}_ngp_bench.txt 2>&1; grep -E "ms/step|render 1200" $OUT/${R}_ngp_bench.txt
python bench.py --full --steps 20 --warmup 5 > $OUT/${R}_bench_n1_driver_style.json 2> $OUT/${R}_bench_n1_driver_style.err; echo "rc=$?"; grep -o "\"ms_per_step\": [0-9.]*" $OUT/${R}_bench_n1_driver_style.json
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${R}_prof_ngp -- python3 $ROOT/tools/ngp_bench.py --steps 200 > $OUT/${R}_prof_ngp.log 2> $OUT/${R}_prof_ngp.err
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/${R}_pmc_ngp_fetch -- python3 $ROOT/tools/ngp_bench.py --steps 40 --warmup 20 > /dev/null 2> $OUT/${R}_pmc_ngp_fetch.err
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/${R}_pmc_ngp_write -- python3 $ROOT/tools/ngp_bench.py --steps 40 --warmup 20 > /dev/null 2> $OUT/${R}_pmc_ngp_write.err
cd $ROOT
python tools/rocprof_clean_stats.py $OUT/${R}_prof_ngp --head k_rays_given --skip-first 320 > $OUT/${R}_ngp_kernel_stats.csv
head -24 $OUT/${R}_ngp_kernel_stats.csv
python tools/pmc_traffic.py $OUT/${R}_pmc_ngp_fetch $OUT/${R}_pmc_ngp_write $OUT/${R}_pmc_ngp_fetch_write_per_kernel.json 60
for d in ${R}_prof_ngp ${R}_pmc_ngp_fetch ${R}_pmc_ngp_write; do find $OUT/$d -name "*kernel_trace.csv" -delete; find $OUT/$d -name "*counter_collection.csv" -size +20M -delete; done
