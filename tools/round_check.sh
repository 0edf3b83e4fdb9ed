# Round-end check on one MI355X: the GPU suite, the full bench line (live PMC traffic, CPU baseline), and a
# rocprofv3 kernel trace of the bench. Every GPU step has its own time limit; the first failure ends the script.
# Output goes to $OUT_DIR (default bench_out/, ignored by git).
set -o pipefail
O=${OUT_DIR:-bench_out}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
timeout -k 10 500 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $O/gputests.log 2>&1 || exit 11
timeout -k 10 600 python bench.py --full > $O/bench_full.json 2> $O/bench_full.err || exit 12
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o run -- python3 bench.py --full --no-pmc --no-cpu-baseline > $O/bench_prof.json 2> $O/bench_prof.err || exit 13
timeout -k 10 240 python bench.py --ngram 5 --steps 20 --warmup 5 --full --no-pmc --no-cpu-baseline > $O/bench5.json 2> $O/bench5.err || exit 14
