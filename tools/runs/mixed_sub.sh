set -o pipefail
O=${BENCH_OUT:-bench_out}; mkdir -p $O
for r in 1 2; do for n in 0 2 3 6; do
  o=$O/ms_$n.$r
  timeout -k 10 200 python bench.py --steps 10 --workload mixed --full --no-cpu-baseline --no-north-star --sub-batches $n > $o.json 2> $O/ms.err || { tail -3 $O/ms.err; exit 1; }
  python -c "import json; d=json.load(open('$o.json')); print('sub', $n, $r, round(d['value']), round(d['ms_per_step'],2), 'serial', round(d['serial_homogeneous']['value']))"
done; done
