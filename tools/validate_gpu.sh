# Validation on a GPU box (bash tools/validate_gpu.sh OUTDIR): GPU suite (plain, then once more with poisoned allocations), smoke, the bench command with every leg (--full)
set -o pipefail
O=${1:?usage: tools/validate_gpu.sh OUTDIR}
mkdir -p "$O"
timeout -k 10 900 python -m pytest tests -m gpu -x -q > "$O/pytest.log" 2>&1; rc=$?; echo "pytest rc=$rc"; tail -3 "$O/pytest.log"
[ $rc -eq 0 ] || exit 1
BGS_DEBUG_POISON=1 timeout -k 10 900 python -m pytest tests -m gpu -x -q > "$O/pytest_poison.log" 2>&1; rc=$?; echo "pytest poison rc=$rc"; tail -3 "$O/pytest_poison.log"
[ $rc -eq 0 ] || exit 1
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2 || exit 1
timeout -k 10 600 python bench.py --gpus 1 --steps 20 --warmup 5 --full > "$O/bench_k20.json" 2> "$O/bench_k20.err"; echo "bench rc=$?"
python - "$O/bench_k20.json" <<'P'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline']['sustained'], d['cpu_baseline']['value'], d['s_surv']['default']['mpixels_per_s'])
P
