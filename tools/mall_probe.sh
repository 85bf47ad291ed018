set -e
OUT=${1:?usage: tools/mall_probe.sh <output directory>}
mkdir -p "$OUT"
for f in 16 32 48 64 128 256; do
  python bench.py --frames $f --steps 60 --warmup 5 --full --no-extra --no-cpu-baseline --no-verify > "$OUT/f$f.json" 2> "$OUT/f$f.err"
  echo done $f
done
