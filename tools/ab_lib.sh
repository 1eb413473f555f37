# interleaved bench A/B of the in-tree build against variant libraries (tools/variant.sh):
#   [OUT=<dir for the runs' lines>] tools/ab_lib.sh "<bench args>" <rounds> <variant>...
ARGS=$1; R=$2; shift 2
OUT=${OUT:-_scratch/ab}
mkdir -p $OUT
for r in $(seq 1 $R); do
  for v in base "$@"; do
    if [ $v = base ]; then L=""; else L=tiny_mp2v_dec_amd/_var/$v/libmp2vg.so; fi
    MP2VG_LIB=$L timeout -k 10 200 python bench.py --full --no-cpu-baseline $ARGS > $OUT/$v.json 2> $OUT/$v.err || { tail -5 $OUT/$v.err; exit 1; }
    echo "$v $(python3 -c "import json;d=json.loads(open('$OUT/$v.json').read().strip().splitlines()[-1]);print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['frame_digest_of_digests'])")"
  done
done
