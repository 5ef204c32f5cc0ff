set -u
OUT=${1:?usage: tools/_session_final.sh <output directory, relative to the repository root>}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 1000 python bench.py --full --steps 50 --warmup 5 > "$OUT/bench.log" 2> "$OUT/bench.err"
rc=$?
echo "bench rc=$rc"; tail -3 "$OUT/bench.err"
[ $rc -eq 0 ] || exit 1
for c in 1 3 4; do
  B="python bench.py --config $c --steps 20 --warmup 3 --cpu-baseline off --host-calls off --plugin-frame off --other-configs off --adapter-frame off"
  timeout -k 10 -s KILL 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$PWD/$OUT/stats$c" -o run -- $B > "$OUT/stats$c.log" 2>&1
  echo "stats$c rc=$?"
done
SLACKS=8 bash tools/_session_mig.sh "$OUT"
