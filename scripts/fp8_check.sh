#!/bin/bash
# fp8 backbone mode: kernel + stage tests, then the bench with and without --fp8 (same box, back to back)
cd "$(dirname "$0")/.."
O=${OUT_DIR:-$(mktemp -d)}; mkdir -p "$O"; echo "outputs in $O"
python -m pytest tests/test_kernels_gpu.py tests/test_stages_gpu.py -x -q -m gpu -k "fp8" 2>&1 | tail -15
python bench.py --full --no-cpu-baseline --fp8 --layers $O/fp8_layers.tsv > $O/fp8_bench.json 2> $O/fp8_bench.err; tail -3 $O/fp8_bench.err; cat $O/fp8_bench.json
python bench.py --full --no-cpu-baseline --no-accuracy > $O/bf16_bench.json 2>/dev/null; cat $O/bf16_bench.json
