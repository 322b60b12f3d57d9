# round end in one call: smoke, the full GPU suite, the --full bench line; outputs under the directory given
OUT=${1:?usage: $0 OUT_DIR}; mkdir -p $OUT
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/final_smoke.log 2>&1; echo "smoke rc=$?"; tail -1 $OUT/final_smoke.log
timeout 1200 python -m pytest tests -m gpu -x -q > $OUT/final_tests.log 2>&1; echo "tests rc=$?"; tail -3 $OUT/final_tests.log
timeout 900 python bench.py --full > $OUT/final_bench.log 2> $OUT/final_bench.err; echo "bench rc=$?"; tail -c 600 $OUT/final_bench.log
