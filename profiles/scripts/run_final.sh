# GPU suite, smoke, the --full bench line; output under $1 (bench_out).  Each GPU step has its own time limit and the
# first one that fails ends the script: nothing more is started on the card.
set -o pipefail
O=${1:-bench_out}
mkdir -p $O
timeout -k 10 1200 python -m pytest tests -m gpu -x -q > $O/pytest_gpu_final.log 2>&1; rc=$?
echo "pytest rc=$rc" >> $O/pytest_gpu_final.log
grep -E "passed|failed|rc=" $O/pytest_gpu_final.log | tail -3
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2 || exit $?
timeout -k 10 600 python bench.py --full > $O/bench_final.json 2> $O/bench_final.err || exit $?
tail -c 1500 $O/bench_final.json
