# full GPU suite + smoke + the driver's bench command with --full (the lines read below); output under $1 (bench_out).
# Every GPU step has its own time limit, and the first one that fails (fault, abort, time-out, failing tests) ends
# the script: nothing more is started on the card.
set -o pipefail
O=${1:-bench_out}/validate
mkdir -p $O
timeout -k 10 1500 python -m pytest tests -m gpu -x -q > $O/pytest_gpu.log 2>&1; rc=$?
grep -E "passed|failed|^E " $O/pytest_gpu.log | tail -4
[ $rc -eq 0 ] || { echo "GPU suite: status $rc, stopping"; exit $rc; }
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1 || exit $?
timeout -k 10 600 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $O/bench_driver.json 2> $O/bench_driver.err || exit $?
python profiles/scripts/benchline.py driver20 < $O/bench_driver.json
O=$O python - <<'P'
import json, os
j=json.loads(open(os.path.join(os.environ["O"], "bench_driver.json")).read().strip().splitlines()[-1])
r=j["roofline"]
print("bound", r["bound"], "frac", round(r["frac"],3), "walked", round(r["walked"]["frac"],3), "hbm_measured", round(r["hbm_measured"]["frac"],3), "valu", round(r["valu"]["issue_cycle_frac"],3), "insts/pair", round(r["valu"]["valu_insts_per_pair"],1))
print("cpu", j["cpu_baseline"]["value"], j["cpu_baseline"]["sample"][:160], "| c_port", j["cpu_baseline"].get("c_port",{}).get("value"))
print({k: j["config"][k] for k in ("quat_check","sort_ranking","early_rank","depth_channel")})
print("eval", round(j["eval_images_per_s"]["value"],1), "fused", round(j["fused_path"]["value"],1), "syncs", round(j["with_caller_syncs"]["value"],1), "deferred", round(j["deferred_check"]["value"],1))
P
