# tests + bench (both batches, both GEMM modes, synthesis) + rocprofv3 kernel stats; outputs under the directory given
R=$PWD; OUT=$(mkdir -p "${1:?usage: $0 OUT_DIR}" && cd "$1" && pwd)
python -m pytest tests -m gpu -x -q > $OUT/r1_tests.log 2>&1; echo "tests rc=$?"; tail -2 $OUT/r1_tests.log
python bench.py --full > $OUT/r1_bench64.log 2>$OUT/r1_bench64.err; echo "b64 rc=$?"; tail -c 400 $OUT/r1_bench64.err
python bench.py --full --batch 16 --no-cpu-baseline --no-roofline > $OUT/r1_bench16.log 2>&1; echo "b16 rc=$?"
python bench.py --full --gemm f32 --steps 10 --no-cpu-baseline --no-roofline > $OUT/r1_bench64_f32.log 2>&1; echo "b64 f32 rc=$?"
python bench.py --mode synth > $OUT/r1_synth.log 2>&1; echo "synth rc=$?"
cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r1_prof -- python $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/r1_prof.log 2>&1; echo "prof rc=$?"
cd $R; for f in $OUT/r1_bench64.log $OUT/r1_bench16.log $OUT/r1_bench64_f32.log $OUT/r1_synth.log; do tail -1 $f | cut -c1-330; done
