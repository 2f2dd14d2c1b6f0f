# FETCH_SIZE and WRITE_SIZE of the configs[1] kernels, one rocprofv3 counter pass each, written into OUTDIR:
#   bash tools/pmc_fetch_write.sh OUTDIR
mkdir -p "${1:?usage: bash tools/pmc_fetch_write.sh OUTDIR}" && out=$(cd "$1" && pwd) && cd "$(dirname "$0")/.." && export TMPDIR=${TMPDIR:-/tmp}
for set in FETCH_SIZE WRITE_SIZE; do
  rm -rf $TMPDIR/pmc_$set
  timeout 400 rocprofv3 --kernel-trace --pmc $set --output-format csv -d $TMPDIR/pmc_$set -o p -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu --no-lut-opt --no-sw > $out/pmc_bench_$set.json 2>/dev/null
  f=$(ls $TMPDIR/pmc_$set/*counter_collection.csv | head -1)
  for k in k_rt_lw_bb_mirror k_gas_prep_lw_mirror k_scatter_column_halves k_reorder_key_lw_fast; do python3 tools/pmc_summary.py $k $f | sed "s#^.*csv: #$k $set: #"; done
  cp $f $out/pmc_$set.csv
done
