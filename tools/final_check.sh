#!/bin/bash
# Developer helper (GPU box): the end-of-change checks -- the GPU tests, smoke(), and the full bench line (--full: roofline,
# CPU baseline, secondary configs).  Usage: tools/final_check.sh OUT_DIR (logs and the bench line go there).
# A step that hit its time limit, aborted or faulted ends the script: no further GPU step is started after it.
OUT=$(mkdir -p "${1:?usage: tools/final_check.sh OUT_DIR}" && cd "$1" && pwd)
cd "$(dirname "$0")/.."
timeout -k 10 900 python -m pytest tests -m gpu -q -x > $OUT/final_tests.log 2>&1; rc=$?; echo "tests rc=$rc"; tail -3 $OUT/final_tests.log
case $rc in 124|134|137|139) echo "tests ended by a time limit, abort or fault (status $rc); stopping"; exit $rc;; esac
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/final_smoke.log 2>&1; rc=$?; echo "smoke rc=$rc"; tail -2 $OUT/final_smoke.log
[ $rc -eq 0 ] || { echo "smoke failed (status $rc); stopping"; exit $rc; }
timeout -k 10 600 python bench.py --full > $OUT/final_bench.json 2> $OUT/final_bench.err; rc=$?; echo "bench rc=$rc"
[ $rc -eq 0 ] && OUT=$OUT python -c "import json, os; d=json.load(open(os.path.join(os.environ['OUT'], 'final_bench.json'))); print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline']['step']['frac'], d['cpu_baseline']['value']); print({k: {kk: vv for kk, vv in v.items() if kk in ('ms', 'value', 'frac')} if isinstance(v, dict) else v for k, v in d.get('secondary', {}).items()})"
exit $rc
