set -u
OUT=${1:?usage: tools/_session_mig.sh <output directory>}
mkdir -p "$OUT"
export TMPDIR=/tmp
for S in ${SLACKS:-8}; do
  NFGPU_BENCH_TRACE=1 NFGPU_TRACE_MEMBERSHIP=1 NFGPU_TRACE_SHARD=1 timeout -k 10 300 python bench.py --full --self-migrate --steps 40 --warmup 10 --cpu-baseline off --host-calls off --plugin-frame off --adapter-frame off --other-configs off --slack $S > "$OUT/selfmig_s$S.log" 2> "$OUT/selfmig_s$S.err" || { echo "selfmig $S failed"; tail -5 "$OUT/selfmig_s$S.err"; exit 1; }
  python -c "
import json; d=json.loads(open('$OUT/selfmig_s$S.log').read().strip().splitlines()[-1])
print('slack $S', round(d['ms_per_step']*1000,1), {k: round(v['avg_us'],1) for k,v in d['kernels'].items()}, d['migrations'])"
  grep "apply_membership\|shard rows" "$OUT/selfmig_s$S.err" | tail -4 | cut -c1-300
  grep host_ms_per_frame "$OUT/selfmig_s$S.err" | tail -1 | cut -c1-600
done
