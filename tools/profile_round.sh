# One measurement round on the GPU box: bench line, kernel trace, the two PMC passes.
#   bash tools/profile_round.sh r2_a <commit> <output directory, relative to the repository root>
# Every profiled run is a plain bench.py run (no --full): nothing but the timed steps, in particular no
# clock / power sampling while rocprofv3's preload is in the environment.
set -x
TAG=${1:-r2_a}
COMMIT=${2:-unrecorded}
OUT=${3:?usage: bash tools/profile_round.sh TAG COMMIT OUTPUT_DIR}
R=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
cd $R
mkdir -p $OUT
python bench.py --full --steps 20 --warmup 3 > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
tail -c 1500 $OUT/bench_$TAG.json
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -- python3 bench.py --steps 2 --warmup 1 > $OUT/prof_$TAG.log 2>&1
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch_$TAG -- python3 bench.py --steps 1 --warmup 1 > $OUT/pmc_fetch_$TAG.json 2> $OUT/pmc_fetch_$TAG.err
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write_$TAG -- python3 bench.py --steps 1 --warmup 1 > $OUT/pmc_write_$TAG.log 2>&1
F=$(find $OUT/pmc_fetch_$TAG -name "*counter_collection.csv" | head -1)
W=$(find $OUT/pmc_write_$TAG -name "*counter_collection.csv" | head -1)
S=$(find $OUT/prof_$TAG -name "*kernel_stats.csv" | head -1)
# the same two passes over BASELINE configs[3] (N-ImageNet @336: the row-band events kernel, the 480 x 640 -> 336
# preprocess, attention at S = 577), one quarter of its global batch on this one GPU
C3="--config 3 --batch 512 --steps 1 --warmup 1"
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch_c3_$TAG -- python3 bench.py $C3 > $OUT/pmc_fetch_c3_$TAG.json 2> $OUT/pmc_fetch_c3_$TAG.err
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write_c3_$TAG -- python3 bench.py $C3 > $OUT/pmc_write_c3_$TAG.log 2>&1
F3=$(find $OUT/pmc_fetch_c3_$TAG -name "*counter_collection.csv" | head -1)
W3=$(find $OUT/pmc_write_c3_$TAG -name "*counter_collection.csv" | head -1)
python tools/traffic_summary.py $F $W $OUT/pmc_fetch_$TAG.json $COMMIT --config 3 $F3 $W3 $OUT/pmc_fetch_c3_$TAG.json > $OUT/traffic_$TAG.json
cp $S $OUT/${TAG}_kernel_stats.csv
# the tolerance mode's own kernel table (eventclip_amd.clip.TOLERANCE_MODE on 16-bit-representable weights)
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_tol_$TAG -- python3 bench.py --steps 2 --warmup 1 --tolerance-mode --f16-weights > $OUT/prof_tol_$TAG.log 2>&1
cp $(find $OUT/prof_tol_$TAG -name "*kernel_stats.csv" | head -1) $OUT/${TAG}_tolerance_kernel_stats.csv
ls -la $OUT/*$TAG*
