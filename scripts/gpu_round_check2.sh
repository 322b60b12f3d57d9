# end-of-round check after the ping-pong main loop: tests, the bench line (twice), kernel stats;
# outputs under the directory given
R=$PWD; OUT=$(mkdir -p "${1:?usage: $0 OUT_DIR}" && cd "$1" && pwd)
python -m pytest tests -m gpu -x -q > $OUT/r1e_tests.log 2>&1; echo "tests rc=$?"; tail -2 $OUT/r1e_tests.log
python bench.py --full > $OUT/r1e_bench64.log 2>$OUT/r1e_bench64.err; echo "b64 rc=$?"; tail -c 300 $OUT/r1e_bench64.err
python bench.py --full --no-cpu-baseline --no-roofline > $OUT/r1e_bench64_b.log 2>&1; echo "b64 (2nd) rc=$?"
cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r1e_prof -- python $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/r1e_prof.log 2>&1; echo "prof rc=$?"
cd $R; for f in $OUT/r1e_bench64.log $OUT/r1e_bench64_b.log; do tail -1 $f | cut -c1-400; done
