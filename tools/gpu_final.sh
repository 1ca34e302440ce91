#!/bin/bash
# Final measurement session of a round (everything committed under profiles/r<N>_* comes from gpurun_out/final<N>/ of ONE box):
# bench tile lists, the GPU test suite (with the printed parity numbers) and smoke, bench lines (headline with extra_configs, per-op profile, fp8, fp16, small
# batches, real shapes, PCIe-inclusive, NMS stream A/B), rocprofv3 kernel trace, the counter passes (separate runs, counters
# only).  usage on the GPU box:  ROUND=4 bash tools/gpu_final.sh      (tables are NOT re-tuned here: tools/retune_all.sh)
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
R=${ROUND:-6}
O=gpurun_out/final$R
mkdir -p $O
export TMPDIR=/tmp
T0=$(date +%s); T_MAX=${T_MAX:-2100}
left() { [ $(( $(date +%s) - T0 )) -lt $T_MAX ]; }
stamp() { echo "$1 at $(( $(date +%s) - T0 )) s" >> $O/timing.log; }
(rocminfo | grep -E "Marketing Name|gfx|Compute Unit" | head -6; nproc) > $O/env.txt 2>&1
timeout 300 python tools/dump_bench_tiles.py > $O/dump_tiles.log 2>&1; cp tests/golden/bench_tiles.json $O/bench_tiles.json
stamp "tile lists"
# ---- tests and smoke ----
timeout 1500 python -m pytest tests -m gpu -q -rP --timeout 900 > $O/pytest_gpu_full.log 2>&1; echo "pytest exit $?" >> $O/pytest_gpu_full.log
# (the committed log: the progress lines, the parity numbers the tests print, the summary)
grep -E "^\.|passed|failed|pytest exit|x6 checkpoint|sparse x6|worst|predictions:|fp8 x6|conf|tile configurations" $O/pytest_gpu_full.log | cut -c1-600 > $O/pytest_gpu.log
timeout 300 python __graft_entry__.py smoke > $O/smoke.log 2>&1; echo "smoke exit $?" >> $O/smoke.log
stamp "tests"
# ---- bench lines ----
timeout 600 python bench.py --full --steps 100 --warmup 10 --profile-out $O/ops_b32.json > $O/bench.log 2>&1
timeout 300 python bench.py --full --dtype fp8 --batch 64 --steps 50 --warmup 5 --no-cpu-baseline --no-extra-configs --profile-out $O/ops_fp8_b64.json > $O/bench_fp8_b64.log 2>&1
timeout 300 python bench.py --full --dtype fp16 --steps 50 --warmup 5 --no-cpu-baseline --no-extra-configs > $O/bench_fp16.log 2>&1
timeout 300 python bench.py --full --steps 50 --warmup 5 --no-cpu-baseline --no-extra-configs --nms-inline > $O/bench_nms_inline.log 2>&1
timeout 300 python bench.py --full --steps 50 --warmup 5 --no-cpu-baseline --no-extra-configs > $O/bench_nms_own.log 2>&1
stamp "main benches"
# ---- rocprofv3: kernel trace of the bench command, then the counter passes ----
(cd /tmp && timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OLDPWD/$O/prof" -o r$R -- \
   python "$OLDPWD/bench.py" --steps 10 --warmup 3 --no-cpu-baseline --lean > "$OLDPWD/$O/rocprof.log" 2>&1)
find $O/prof -type f ! -name "*stats*" -size +2M -delete 2>/dev/null
RP="$PWD"
for C in FETCH_SIZE WRITE_SIZE; do
  (cd /tmp && timeout 300 rocprofv3 --pmc $C -d "$RP/$O/traffic_$C" -o t --output-format csv -- \
     python "$RP/bench.py" --steps 2 --warmup 1 --no-cpu-baseline --lean > "$RP/$O/traffic_$C.log" 2>&1)
done
python tools/hbm_traffic.py $O/traffic_FETCH_SIZE $O/traffic_WRITE_SIZE YOLOV5X6_MD:32:1280 $O/hbm_traffic.json $O/ops_b32.json $O/hbm_traffic_by_kernel.txt > $O/hbm_traffic.log 2>&1
# (the per-dispatch CSVs are kept when small enough: they are what the per-op alignment reads)
find $O/traffic_FETCH_SIZE $O/traffic_WRITE_SIZE -type f -size +8M -delete 2>/dev/null
# L2 hit rate per kernel (why the reads are 1.6x the algorithmic bytes: VERDICT r5 item 3): its own counters-only pass
(cd /tmp && timeout 300 rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum -d "$RP/$O/tcc" -o t --output-format csv -- \
   python "$RP/bench.py" --steps 2 --warmup 1 --no-cpu-baseline --lean > "$RP/$O/tcc.log" 2>&1)
python - "$O/tcc" > $O/l2_hit_rate_by_kernel.txt 2>&1 <<'PY'
import collections, csv, glob, re, sys
acc = collections.defaultdict(lambda: [0.0, 0.0, 0])
for f in glob.glob(sys.argv[1] + '/**/*counter_collection.csv', recursive=True):
    for r in csv.DictReader(open(f)):
        name = re.sub(r'\(.*', '', r['Kernel_Name']).replace('void ', '').replace('mdhip::st_bf16::', '').replace('mdhip::', '')
        if r['Counter_Name'] == 'TCC_HIT_sum': acc[name][0] += float(r['Counter_Value']); acc[name][2] += 1
        if r['Counter_Name'] == 'TCC_MISS_sum': acc[name][1] += float(r['Counter_Value'])
print('# L2 (TCC) hit rate per kernel instantiation over a 3-step bench run (rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum, counters only): hits / (hits + misses)')
for name, (h, m, n) in sorted(acc.items(), key=lambda kv: -(kv[1][0] + kv[1][1])):
    if h + m > 0: print('{:7.4f}  {:12.0f} requests per dispatch  {:4d} dispatches  {}'.format(h / (h + m), (h + m) / max(n, 1), n, name))
PY
find $O/tcc -type f -size +1M -delete 2>/dev/null
stamp "trace + traffic + L2 hit rate"
left && { bash tools/pmc_bench.sh final$R > $O/pmc_bench.log 2>&1; cp gpurun_out/pmc_final$R.txt gpurun_out/pmc_final$R.json $O/ 2>/dev/null; }
stamp "pmc"
left && timeout 300 python bench.py --full --steps 50 --warmup 5 --no-cpu-baseline --no-extra-configs --src 1536x2048 > $O/bench_real43.log 2>&1
left && timeout 300 python bench.py --full --steps 50 --warmup 5 --no-cpu-baseline --no-extra-configs --src 1080x1920 > $O/bench_video_1080p.log 2>&1
left && timeout 300 python bench.py --full --steps 50 --warmup 5 --no-cpu-baseline --no-extra-configs --src 1600x2400 > $O/bench_real32.log 2>&1
for s in 1080x1920 1536x2048 1600x2400; do
  left && timeout 200 python bench.py --dtype fp16 --src $s --steps 30 --warmup 5 --no-cpu-baseline --no-extra-configs --lean > $O/bench_fp16_$s.log 2>&1
done
for b in 1 2 4 8 16; do
  left && timeout 200 python bench.py --batch $b --steps 60 --warmup 10 --no-cpu-baseline --lean > $O/bench_b$b.log 2>&1
done
left && timeout 300 python bench.py --full --steps 50 --warmup 5 --no-cpu-baseline --no-extra-configs --host-fed > $O/bench_hostfed.log 2>&1
left && timeout 300 python tests/accuracy_report.py --x6 > $O/accuracy_x6.txt 2>&1
stamp "all done"
ls -laR $O > $O/ls.log
# ---- the multi-rank code path of bench.py on this one GPU (gloo test hook), the end-to-end feed on JPEG files ----
left && MDHIP_BENCH_ONE_GPU=1 timeout 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 \
    bench.py --full --gpus 2 --batch 8 --steps 30 --warmup 5 > $O/bench_2rank_one_gpu_gloo.log 2>&1
# the self-launching form (`python bench.py --gpus 2`, no launcher) and a pinned single-GPU run (placement.pin_worker(force))
left && MDHIP_BENCH_ONE_GPU=1 timeout 300 python bench.py --full --gpus 2 --batch 8 --steps 30 --warmup 5 > $O/bench_selflaunch_2rank.log 2> $O/bench_selflaunch_2rank.err
left && timeout 300 python bench.py --full --steps 50 --warmup 5 --no-cpu-baseline --no-extra-configs --pin-cpus > $O/bench_pinned.log 2> $O/bench_pinned.err
left && MDHIP_BENCH_ONE_GPU=1 timeout 400 python bench.py --full --gpus 8 --batch 2 --steps 20 --warmup 3 > $O/bench_8rank_one_gpu_gloo.log 2> $O/bench_8rank_one_gpu_gloo.err
# a REAL RCCL failure: both ranks on device 0 with the RCCL attempt made (RCCL refuses the duplicate device) -> the line must come out over gloo, with the reason
left && MDHIP_BENCH_ONE_GPU=try timeout 300 python bench.py --full --gpus 2 --batch 8 --steps 30 --warmup 5 > $O/bench_2rank_rccl_refused.log 2> $O/bench_2rank_rccl_refused.err
left && timeout 200 python tools/letterbox_bench.py > $O/letterbox_bench.txt 2>&1
left && timeout 400 python tools/e2e_feed_bench.py --n 4096 --workers 16,24 --out $O/e2e_feed.json > $O/e2e_feed.log 2>&1
# the NUMA placement code on this box's topology (8 GPUs asked for: what the planner does with the GPUs it cannot see)
left && python -c "
from megadetector_amd import placement as P
t = P.read_topology(8); print('topology', t)
plan = P.plan(8, t); print('cpus per worker', [len(c) for c in plan]); print('disjoint', len(set(c for w in plan for c in w)) == sum(len(c) for c in plan))
print('pin_worker(3, 8) ->', len(P.pin_worker(3, 8, verbose=True)), 'cpus')
import os; print('affinity of every thread now', sorted({len(os.sched_getaffinity(int(t))) for t in os.listdir('/proc/self/task')}))
" > $O/placement_box.txt 2>&1
stamp "2-rank + feed"
