set -e
OUT=${1:?usage: tools/sizes_probe.sh <output directory>}
mkdir -p "$OUT"
for n in 458752 917504 1048576 1376256; do
  g=$((n/256))
  timeout -k 10 200 python bench.py --full --steps 30 --warmup 5 --cpu-baseline off --entities $n --groups $g > "$OUT/b$n.log" 2>&1
  python -c "
import json,sys; d=json.loads(open('$OUT/b$n.log').read().strip().splitlines()[-1]); print($n, d['ms_per_step'], d['kernels']['k_tick']['avg_us'], d['roofline']['frac'])"
done
ABL=0,4,512,2048 timeout -k 10 300 python tools/ablate.py --variants 0,4,512,2048 > "$OUT/abl.log" 2>&1
python -c "
import json; t=open('$OUT/abl.log').read(); d=json.loads(t[t.index('{'):])
for k,v in d.items(): print(k, v['k_tick']['median_us'])"
