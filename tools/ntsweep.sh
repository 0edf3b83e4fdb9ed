# Cache-policy A/B of the bench step: each entry "flags:head" runs bench.py (200 steps, --full for the per-launch
# time, no PMC / CPU baseline) with PG_SPMM_FLAGS=flags and PG_HEAD_NT=head, twice over, appending "rep flags head
# ms_per_step avg_launch_ms" lines to $OUT_DIR/ntsweep.txt (default bench_out/, ignored by git).
# usage: CASES="0:0 0x400:0 0:1" bash tools/ntsweep.sh
set -o pipefail
O=${OUT_DIR:-bench_out}
mkdir -p $O
for rep in 1 2; do
for c in ${CASES:-0:0 0x400:0 0:1}; do
  f=${c%%:*}; h=${c##*:}
  PG_SPMM_FLAGS=$f PG_HEAD_NT=$h timeout -k 10 120 python bench.py --full --no-pmc --no-cpu-baseline --steps 200 --warmup 50 > $O/b_${f}_$h.json 2>/dev/null || exit 1
  echo "$rep $f $h $(python -c "import json;d=json.loads(open('$O/b_${f}_$h.json').read().strip().splitlines()[-1]);print(d['ms_per_step'], d['roofline']['avg_launch_ms'])")" >> $O/ntsweep.txt
done
done
