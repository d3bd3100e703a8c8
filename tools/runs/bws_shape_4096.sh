set -o pipefail
O=${BENCH_OUT:-bench_out}; mkdir -p $O
for r in 1 2; do for v in auto pairs2 rows2; do
  o=$O/bws_$v.$r
  timeout -k 10 200 python bench.py --steps 10 --batch-per-gpu 4096 --full --no-cpu-baseline --no-north-star --bws-variant $v > $o.json 2> $o.err || { tail -3 $o.err; exit 1; }
  python -c "import json; d=json.load(open('$o.json')); print('$v', $r, round(d['value']), round(d['ms_per_step'],3), {k: round(v['avg_launch_ms'],4) for k, v in d['roofline']['per_kernel'].items()})"
done; done
