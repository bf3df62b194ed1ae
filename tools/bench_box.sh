#!/bin/bash
# One fresh box's answer to the driver's invocation with everything the line can carry, kept as a file of its own:
#   OUT=<dir> bash tools/bench_box.sh   ->   <dir>/${ROUND:-r06}_box_<UTC time>.json
# tools/bench_boxes_table.py turns the collected files into profiles/r05_bench_boxes.txt.
mkdir -p "${OUT:?set OUT to the directory the line goes to}"
stamp=$(date -u +%Y%m%dT%H%M%SZ)
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $OUT/${ROUND:-r06}_box_$stamp.json 2> $OUT/${ROUND:-r06}_box_$stamp.err
echo "rc=$? $(cut -c1-200 $OUT/${ROUND:-r06}_box_$stamp.json)"
