# bench every variant library under _build/var (or the names given) at BATCHES; result lines
# go to $BENCH_OUT/var (default bench_out/var)
set -o pipefail
O=${BENCH_OUT:-bench_out}/var
mkdir -p $O
V=mhpc_minimal_env_amd/csrc/_build/var
names=${@:-$(ls $V)}
for n in $names; do
  for b in ${BATCHES:-1024 4096}; do
    o=$O/$n.$b
    MHPC_AMD_LIB=$V/$n/libmhpc_amd.so timeout -k 10 300 python bench.py --steps 3 --warmup 1 --batch-per-gpu $b --full --no-cpu-baseline > $o.json 2> $o.err || { echo "$n $b FAILED"; tail -3 $o.err; exit 1; }
    python -c "import json; d=json.load(open('$o.json')); print('$n', $b, round(d['value']), {k.split('(')[0]: round(v, 2) for k, v in d['kernel_ms_per_step'].items()})"
  done
done
