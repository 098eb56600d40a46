#!/bin/bash
# one calibration sample: a short bench line (calibration probes + 12 timed steps + the one-stream event pass) on stdout;
# save it as cal_<tag>.json, tools/cal_show.py tabulates such files
set -o pipefail
timeout -k 10 600 python bench.py --full --steps 12 --warmup 3 --no-extra-modes --no-cpu-baseline 2>/dev/null || exit 1
