#!/bin/bash
# The end-of-round pass on a GPU box: the GPU suite (plain and with poisoned buffers), the measured peaks, the PMC passes,
# the full bench line and a kernel-trace profile of it.   usage: tools/final_pass.sh OUTDIR
set -o pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="$(mkdir -p "${1:?usage: tools/final_pass.sh OUTDIR}" && cd "$1" && pwd)"
cd "$ROOT"
timeout -k 10 900 python -m pytest tests -x -q -m gpu > "$OUT/gpu_tests.log" 2>&1 || { tail -20 "$OUT/gpu_tests.log"; exit 1; }
PHASM_POISON=0xA5 timeout -k 10 600 python -m pytest tests/test_gpu_parity.py tests/test_gpu_streamed.py tests/test_gpu_extend.py tests/test_gpu_layout.py -x -q -m gpu > "$OUT/gpu_tests_poison.log" 2>&1 || { tail -20 "$OUT/gpu_tests_poison.log"; exit 1; }
timeout -k 10 300 python tools/ubench.py > "$OUT/ubench.json" 2> "$OUT/ubench.err" || exit 1
timeout -k 10 900 tools/collect_pmc.sh "$OUT/pmc" 2> "$OUT/collect.err"
python3 tools/pmc_to_traffic.py "$OUT/pmc" "$OUT/pmc_profiles" > "$OUT/to_traffic.log" 2>&1 || exit 1
cp profiles/traffic.json "$OUT/traffic.json"
timeout -k 10 600 python bench.py --steps 20 --warmup 3 --full > "$OUT/bench.json" 2> "$OUT/bench.err" || { tail -5 "$OUT/bench.err"; exit 1; }
# (the profiler run starts outside the tree: rocprofv3 writes its scratch files into the working directory)
cd "$(mktemp -d)"
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -- python3 "$ROOT/bench.py" --steps 20 --warmup 3 --full --no-cfg4 --no-tuples --no-cpu-baseline > "$OUT/prof_bench.json" 2> "$OUT/prof.err"
cd "$ROOT"
tail -2 "$OUT/gpu_tests.log"; tail -2 "$OUT/gpu_tests_poison.log"
ls "$OUT"/prof/* | head
