# The GPU tier, smoke() and the full bench line, each log under OUT (first argument; default bench_logs/).  Every step has
# a time limit of its own, and the first one that fails ends the script.
OUT=${1:-bench_logs}
mkdir -p "$OUT"
step() { # seconds, log, command...
  local limit=$1 log=$2; shift 2
  timeout -k 10 "$limit" "$@" > "$log" 2>&1; local rc=$?
  tail -5 "$log"; return $rc
}
step 5400 "$OUT"/gpu_tier.log python -m pytest tests/ -x -q -m gpu || exit
step 600 "$OUT"/smoke.log python -c "import __graft_entry__ as g; g.smoke()" || exit
timeout -k 10 900 python bench.py --gpus 1 --full > "$OUT"/bench_full.json 2> "$OUT"/bench_full.err; rc=$?
tail -c 1500 "$OUT"/bench_full.json; exit $rc
