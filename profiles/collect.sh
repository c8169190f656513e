#!/bin/bash
# Evidence run behind profiles/<tag>_*: GPU tests, bench lines, rocprofv3 kernel stats, FETCH / WRITE PMC passes.
# usage (on an MI355X machine): bash profiles/collect.sh r01_k   -> $OUT_DIR/<tag>/, default prof_out/<tag>/ (copy the summaries
# into profiles/).  Every bench.py call runs with --full: the counters and the evidence cover the report passes too.
tag=${1:-r01_j}
cd "$(dirname "$0")/.."; export TMPDIR=/tmp
out=${OUT_DIR:-prof_out}/$tag
mkdir -p $out
# SKIP_PYTEST=1: the GPU suite of the same tree ran in its own call (its tail is copied to profiles/<tag>_pytest.txt by hand)
[ -n "$SKIP_PYTEST" ] || timeout 2400 python -m pytest tests -q -m gpu --durations=8 2>&1 | tail -16 > $out/pytest.txt
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $out/stats -o s -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-fp32-pass --cell-streams 1 --no-extras --no-dropin --no-force-exchange --no-pipeline --no-trained > $out/stats.log 2>&1
trace=$(find $out/stats -name "s_kernel_trace.csv" | head -1)
python profiles/summarize.py $trace $out/kernel_stats.md "$tag: python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-fp32-pass --cell-streams 1 --no-extras --no-dropin --no-force-exchange --no-pipeline --no-trained (12k cells + 1k queries, 1 x MI355X)" > /dev/null
timeout 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $out/fetch -o p -- python bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-fp32-pass --cell-streams 1 --no-extras --no-dropin --no-force-exchange --no-pipeline --no-trained > $out/fetch.log 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $out/write -o p -- python bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-fp32-pass --cell-streams 1 --no-extras --no-dropin --no-force-exchange --no-pipeline --no-trained > $out/write.log 2>&1
python profiles/pmc_traffic.py $out/fetch $out/write $out/pmc_traffic.json > /dev/null
# matrix-pipe utilisation of the kernels (own pass: counters are never combined with tracing)
timeout 600 rocprofv3 --kernel-trace --pmc SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY --output-format csv -d $out/sq -o p -- python bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-fp32-pass --cell-streams 1 --no-extras --no-dropin --no-force-exchange --no-pipeline --no-trained > $out/sq.log 2>&1
python profiles/pmc_summary.py $(dirname $(find $out/sq -name "p_counter_collection.csv" | head -1)) p 10 > $out/pmc_sq.txt 2>&1
# effective shader clock per kernel (is a kernel held by the 1,400 W package power cap?) + the power probe itself
timeout 600 rocprofv3 --kernel-trace --pmc GRBM_GUI_ACTIVE --output-format csv -d $out/grbm -o p -- python bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-fp32-pass --cell-streams 1 --no-extras --no-dropin --no-force-exchange --no-pipeline --no-trained > $out/grbm.log 2>&1
python profiles/pmc_clock.py $(dirname $(find $out/grbm -name "p_counter_collection.csv" | head -1)) p 14 > $out/pmc_clock.txt 2>&1
bash profiles/power_probe.sh $out/power > $out/power_probe.txt 2>&1
# the bench line quotes the HBM traffic and the MFMA-busy fraction of the dominant kernel from the newest profiles/*_evidence.json
# (stamped with the kernel sources' hashes; bench.py refuses figures whose kernel source changed since): this run's
cp $out/pmc_traffic.json profiles/${tag}_pmc_traffic.json
python profiles/evidence.py $out/pmc_traffic.json $out/sq $out/grbm $out/evidence.json $tag > $out/evidence.txt 2>&1
cp $out/evidence.json profiles/${tag}_evidence.json
timeout 900 python bench.py --full --steps 20 --warmup 5 2> $out/bench.err | tail -1 > $out/bench.json
# the default sizes and steps with every report pass: how long the whole run takes, wall clock
t0=$SECONDS; timeout 900 python bench.py --full 2> $out/bench_default.err | tail -1 > $out/bench_default.json; echo "python bench.py --full: $((SECONDS - t0)) s wall" > $out/bench_default_wall.txt
timeout 600 python bench_fine.py 2> $out/bench_fine.err | tail -1 > $out/bench_fine.json
# keep the merge small: drop the raw traces
cp $trace $out/kernel_trace.csv 2>/dev/null   # (kept for re-summarising; not committed)
find $out -name "*.db" -delete; find $out -mindepth 2 -name "*.csv" -delete
cat $out/pytest.txt $out/bench_default_wall.txt 2>/dev/null; cut -c1-400 $out/bench.json; head -12 $out/kernel_stats.md
