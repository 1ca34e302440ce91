#!/bin/bash
# One GPU-box visit (stages picked on the command line; any other argument is a command line run verbatim); everything that should come back goes under $OUT_DIR (relative to the repository, default out/).
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
O=${OUT_DIR:-out}
mkdir -p $O
export TMPDIR=/tmp
for STAGE in "$@"; do
case "$STAGE" in
  probe)
    timeout 60 build/probe_fp8 > $O/probe_fp8.log 2>&1; echo "exit $?" >> $O/probe_fp8.log ;;
  test)
    timeout 1200 python -m pytest tests -m gpu -q --timeout 900 -x -s > $O/pytest_gpu.log 2>&1
    echo "pytest exit $?" >> $O/pytest_gpu.log ;;
  testall)
    timeout 1200 python -m pytest tests -m gpu -q --timeout 900 > $O/pytest_gpu.log 2>&1
    echo "pytest exit $?" >> $O/pytest_gpu.log ;;
  acc)
    timeout 900 python tests/accuracy_report.py --x6 > $O/accuracy_x6.txt 2>&1 ;;
  bench)
    timeout 900 python bench.py --full --steps 50 --warmup 5 --profile-out $O/ops_b32.json > $O/bench.log 2>&1
    echo "bench exit $?" >> $O/bench.log ;;
  benchlean)
    timeout 600 python bench.py --full --steps 50 --warmup 5 --no-cpu-baseline --profile-out $O/ops_b32.json > $O/bench.log 2>&1
    echo "bench exit $?" >> $O/bench.log ;;
  prof)
    (cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OLDPWD/$O/prof" -o run -- \
       python "$OLDPWD/bench.py" --steps 10 --warmup 3 --no-cpu-baseline --lean > "$OLDPWD/$O/rocprof.log" 2>&1)
    find $O/prof -name "*stats*" | head >> $O/rocprof.log
    find $O/prof -type f ! -name "*stats*" -size +2M -delete 2>/dev/null ;;
  traffic)
    R="$PWD"
    for C in FETCH_SIZE WRITE_SIZE; do
      (cd /tmp && timeout 600 rocprofv3 --pmc $C -d "$R/$O/traffic_$C" -o t --output-format csv -- \
         python "$R/bench.py" --steps 2 --warmup 1 --no-cpu-baseline --lean > "$R/$O/traffic_$C.log" 2>&1)
    done
    python tools/hbm_traffic.py $O/traffic_FETCH_SIZE $O/traffic_WRITE_SIZE YOLOV5X6_MD:32:1280 $O/hbm_traffic.json > $O/hbm_traffic.log 2>&1
    find $O/traffic_FETCH_SIZE $O/traffic_WRITE_SIZE -type f -size +1M -delete 2>/dev/null ;;
  *)
    # anything else: a command line to run verbatim, output to $O/cmd.log (appended)
    echo "== $STAGE" >> $O/cmd.log
    timeout 900 bash -c "$STAGE" >> $O/cmd.log 2>&1
    echo "exit $?" >> $O/cmd.log ;;
esac
done
ls -la $O > $O/ls.log
