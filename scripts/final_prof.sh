# Everything behind profiles/r02_*: the bench line, its rocprofv3 kernel stats, three PMC passes, the small-batch
# kernel stats.  usage (on a machine with the GPU): bash scripts/final_prof.sh <tag> [output dir, default prof_out/]
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
V=${1:-r04}
O=$(mkdir -p "${2:-$R/prof_out}" && cd "${2:-$R/prof_out}" && pwd)
cd /tmp && export TMPDIR=/tmp
timeout -k 10 500 python $R/bench.py --full > $O/bench_$V.json 2> $O/bench_$V.err
echo "bench done"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$V -o $V -- python $R/bench.py --steps 5 --full --no-cpu-baseline --no-secondary --no-alone > $O/bench_${V}p.json 2> $O/bench_${V}p.err
echo "kernel stats done"
for G in "FETCH_SIZE" "TCC_HIT_sum TCC_MISS_sum" "SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE"; do
  N=$(echo $G | cut -d' ' -f1)
  timeout -k 10 300 rocprofv3 --pmc $G --kernel-trace --output-format csv -d $O/pmc_$V/$N -o x -- python $R/bench.py --steps 2 --warmup 1 > $O/pmc_${V}_$N.log 2>&1
  echo "pmc $N done"
done
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_${V}_b32 -o b32 -- python $R/scripts/hbm_roofline.py 10000000 > $O/hbm_$V.json 2> $O/hbm_$V.err
echo "small batch done"
cut -c1-300 $O/bench_$V.json
