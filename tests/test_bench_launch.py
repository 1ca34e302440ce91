"""
bench.py as a self-contained launcher (the reference's recipe is one command per GPU,
notebooks/manage_local_batch.py:617-621): `python bench.py --gpus N` without a launcher starts N ranks through
torch.distributed.run on 127.0.0.1 and prints ONE line with n_gpus == N; under a launcher the world size must equal
--gpus.  The rendezvous check stops before anything touches a GPU, so this runs in the CPU suite (gloo, world 2).
Also here: the cpu_baseline leg (thread sweep, forward / NMS split) on a small family member, and the forced
single-worker CPU pinning.
"""

import json
import os
import subprocess
import sys

import pytest

from conftest import REPO


def _env():
    env = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'LOCAL_WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    env['OMP_NUM_THREADS'] = '1'
    return env


def test_bench_gpus_n_launches_its_own_ranks():
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '2', '--rendezvous-check'],
                       env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout                       # ONE JSON line, from rank 0
    line = json.loads(lines[0])
    assert line['n_gpus'] == 2 and sorted(line['ranks']) == [0, 1]
    assert 'torch.distributed.run' in r.stderr and '--nproc-per-node 2' in r.stderr
    # the launcher picks its own rendezvous port (no bind-then-release probe that another process could win)
    assert '--standalone' in r.stderr and '--master-port' not in r.stderr


def test_bench_without_gpus_takes_the_launchers_world_size():
    # `torchrun --nproc-per-node 2 bench.py` (no --gpus): two ranks, one line; an explicit --gpus must still agree
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--standalone', '--local-addr', '127.0.0.1', '--nnodes=1',
                        '--nproc-per-node', '2', os.path.join(REPO, 'bench.py'), '--rendezvous-check'],
                       env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1 and json.loads(lines[0])['n_gpus'] == 2


_CONTROL_PLANE_RANK = r'''
import os, sys, json
sys.path.insert(0, {repo!r})
import torch, bench
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
if os.environ.get('FAIL_ON_RANK') == str(rank):
    # one rank alone cannot start the device plane, and fails before the group exists: every rank has to end up on
    # the host plane -- none may be left waiting in an RCCL collective for it
    import torch.distributed as d
    real = d.new_group
    def broken(*a, **k):
        if k.get('backend') == 'nccl':
            raise RuntimeError('injected: no RCCL on this rank')
        return real(*a, **k)
    d.new_group = broken
dist, group, on_host, name, why = bench.init_control_plane(torch, rank, world, 0, os.environ.get('FORCE_GLOO') == '1',
                                                           timeout_s=120, nccl_timeout_s=20)
t = torch.tensor([float(rank + 1)], dtype=torch.float64)
dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
dist.barrier(group=group)
allr = [None] * world
dist.all_gather_object(allr, [name, on_host, why])
if rank == 0:
    print(json.dumps({{'planes': allr, 'max': float(t.item())}}))
dist.destroy_process_group()
'''


@pytest.mark.parametrize('mode', ['no_device_plane', 'one_rank_fails', 'forced'])
def test_control_plane_falls_back_to_gloo_on_every_rank(tmp_path, mode):
    """bench.py's N > 1 process group (init_control_plane): RCCL is tried as a second group and adopted only if EVERY rank
    got through; here no rank can (no GPU) / one rank is made to fail / the attempt is skipped -- the barriers and the MAX
    over ranks must work over gloo on all ranks either way, and every rank must report the same plane."""
    script = tmp_path / 'rank.py'
    script.write_text(_CONTROL_PLANE_RANK.format(repo=REPO))
    env = _env()
    if mode == 'one_rank_fails':
        env['FAIL_ON_RANK'] = '1'
    if mode == 'forced':
        env['FORCE_GLOO'] = '1'
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--standalone', '--local-addr', '127.0.0.1', '--nnodes=1',
                        '--nproc-per-node', '2', str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    assert out['max'] == 2.0
    assert [p[0] for p in out['planes']] == ['gloo', 'gloo'] and all(p[1] for p in out['planes'])
    assert all(p[2] for p in out['planes'])                 # each rank says why RCCL is not carrying the barriers
    if mode == 'one_rank_fails':                             # the injected failure is the one rank 1 reports
        assert out['planes'][1][2].startswith('RuntimeError: injected'), out['planes']


def test_bench_refuses_a_world_size_that_is_not_gpus():
    env = _env()
    env.update(WORLD_SIZE='2', RANK='0', LOCAL_RANK='0')
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '4', '--rendezvous-check'],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and 'WORLD_SIZE=2' in r.stderr
    # and the driver's N = 1 command stays a plain one-process run
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--rendezvous-check'],
                       env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and json.loads(r.stdout.strip())['n_gpus'] == 1


def test_cpu_baseline_reports_the_best_thread_count_and_the_split():
    import torch
    import bench
    from megadetector_amd import weights_io, yolo_yaml
    w = weights_io.synthetic_weights(yolo_yaml.YOLOV5N6_TEST, seed=0)
    before = torch.get_num_threads()
    res = bench.cpu_baseline(w, 128, 0.2, budget_s=2.0, single_thread=True)
    assert torch.get_num_threads() == before
    assert res['kind'] == 'port' and res['unit'] == 'images/s' and res['value'] > 0
    assert str(res['cores']) in res['thread_sweep_images_per_s'] and res['cores'] <= res['host_threads_available']
    assert res['forward_s_per_image'] > 0 and res['nms_format_s_per_image'] >= 0
    assert res['single_thread']['cores'] == 1


@pytest.mark.skipif(not hasattr(os, 'sched_setaffinity'), reason='no affinity API')
def test_a_lone_worker_is_pinned_only_when_asked():
    from megadetector_amd import placement as P
    code = r'''
import os, sys, json
sys.path.insert(0, {repo!r})
from megadetector_amd import placement as P
allowed = sorted(os.sched_getaffinity(0))
topo = {{'gpu_node': [0], 'node_cpus': {{0: allowed[:max(1, len(allowed) // 2)]}}, 'allowed': allowed}}
a = P.pin_worker(0, 1, topology=topo, verbose=False)
b = P.pin_worker(0, 1, topology=topo, verbose=False, force=True)
print(json.dumps([a == allowed, b, sorted(os.sched_getaffinity(0)), allowed]))
'''.format(repo=REPO)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=60, env=_env())
    assert r.returncode == 0, r.stderr
    untouched, pinned, mask, allowed = json.loads(r.stdout.strip().splitlines()[-1])
    assert untouched
    assert pinned == allowed[:max(1, len(allowed) // 2)] == mask


def test_cpu_baseline_thread_sweep_stops_past_the_optimum_and_inside_the_budget():
    """bench.thread_sweep: the thread-count sweep of the CPU baseline (north_star: the CPU path "timed on the same box's host
    cores in the same run") must not be what an N > 1 line dies of.  Round 6: on a 256-thread host one image at 256 threads
    took 117 s and the two-rank launch ran into its timeout.  With the timings of that host the sweep stops at 64 threads
    (1.5x off the best); with a slow host it stops when the budget is nearly used; and it always tries two counts."""
    import importlib
    bench = importlib.import_module('bench')
    host = {8: 1.02, 16: 0.87, 32: 0.99, 64: 1.58, 128: 3.3, 256: 117.0}
    tried = []
    now = [0.0]

    def time_at(c):
        tried.append(c)
        now[0] += host[c]
        return host[c]

    sweep = bench.thread_sweep(256, time_at, 30.0, clock=lambda: now[0])
    assert tried == [8, 16, 32, 64] and min(sweep, key=sweep.get) == 16, (tried, sweep)
    # a host where every count takes 9 s: after two counts 18 s + 2 x 9 s > 0.7 x 30 s -> no third count
    tried.clear()
    now[0] = 0.0
    slow = lambda c: (tried.append(c), now.__setitem__(0, now[0] + 9.0), 9.0)[2]
    sweep = bench.thread_sweep(128, slow, 30.0, clock=lambda: now[0])
    assert tried == [8, 16], tried
    # a small host: its only count
    tried.clear()
    assert list(bench.thread_sweep(4, lambda c: (tried.append(c), 1.0)[1], 30.0, clock=lambda: 0.0)) == [4]


def test_dump_outputs_writes_the_formatted_detections_of_a_step(tmp_path, monkeypatch):
    """bench.py --dump-outputs DIR: the (detections, max_conf) per image of the last timed step as float64 arrays, NaN past
    each image's count; above the size cap a fixed seeded sample of the images"""
    import importlib
    import numpy as np
    bench = importlib.import_module('bench')
    from megadetector_amd.postprocess import format_detections
    rng = np.random.default_rng(3)
    results = []
    raw, counts = np.zeros((3, 300, 6), dtype=np.float32), np.zeros(3, dtype=np.int32)
    for b, k in enumerate((5, 0, 300)):
        det = np.zeros((k, 6), dtype=np.float32)
        det[:, :2] = rng.uniform(0, 600, (k, 2))
        det[:, 2:4] = det[:, :2] + rng.uniform(1, 600, (k, 2))
        det[:, 4] = np.sort(rng.uniform(1e-5, 1, k))[::-1]
        det[:, 5] = rng.integers(0, 3, k)
        results.append(format_detections(det, (1280, 1280), (1280, 1280, 3), (1280, 1280, 3), 1e-5))
        raw[b, :k], counts[b] = det, k
    raw[0, 5:] = 7.0                                          # slot contents past the count are not output
    bench.dump_outputs(str(tmp_path / 'all'), results, nms=(raw, counts))
    got = {n: np.load(str(tmp_path / 'all' / (n + '.npy')))
           for n in ('image_index', 'num_detections', 'max_conf', 'category', 'conf', 'bbox', 'nms_det', 'nms_num_detections')}
    assert all(a.dtype == np.float64 for n, a in got.items() if n != 'nms_det') and got['nms_det'].dtype == np.float32
    assert got['nms_num_detections'].tolist() == [5, 0, 300] and got['nms_det'].shape == (3, 300, 6)
    for b, k in enumerate((5, 0, 300)):
        assert np.array_equal(got['nms_det'][b, :k], raw[b, :k]) and np.isnan(got['nms_det'][b, k:]).all()
    assert got['image_index'].tolist() == [0, 1, 2]
    assert got['bbox'].shape == (3, 300, 4) and got['conf'].shape == got['category'].shape == (3, 300)
    for i, (dets, max_conf) in enumerate(results):
        n = len(dets)
        assert got['num_detections'][i] == n and got['max_conf'][i] == max_conf
        assert got['conf'][i, :n].tolist() == [d['conf'] for d in dets]
        assert got['category'][i, :n].tolist() == [float(d['category']) for d in dets]
        assert got['bbox'][i, :n].tolist() == [d['bbox'] for d in dets]
        assert np.isnan(got['conf'][i, n:]).all() and np.isnan(got['bbox'][i, n:]).all()
    # the cap: room for two images -> the same two every time
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 2 * (3 + 6 * 300) * 8)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), results)
    a, b = (np.load(str(tmp_path / d / 'image_index.npy')) for d in ('a', 'b'))
    assert len(a) == 2 and a.tolist() == b.tolist()
    i = int(a[0])
    assert np.array_equal(np.load(str(tmp_path / 'a' / 'conf.npy'))[0], got['conf'][i], equal_nan=True)


def test_bench_refuses_zero_timed_steps():
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--steps', '0', '--rendezvous-check'],
                       env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and '--steps' in r.stderr


@pytest.mark.gpu
def test_dump_outputs_holds_the_last_timed_step(tmp_path):
    """bench.py --steps 3 --dump-outputs: the dump is the NMS output of the batch of the LAST timed step (seeded batch
    (3 - 1) % 8), recomputed here through the C ABI on a context of its own, and the formatted detections are those rows
    formatted"""
    import numpy as np
    import torch
    from megadetector_amd import weights_io, yolo_yaml
    from megadetector_amd.hip_backend import HipContext
    from megadetector_amd.postprocess import format_detections, letterbox_geometry
    B, S, steps, thr = 4, 256, 3, 1e-5
    out = tmp_path / 'dump'
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '1',
                        '--batch', str(B), '--size', str(S), '--model', 'YOLOV5N6_TEST', '--dtype', 'fp16', '--lean',
                        '--no-cpu-baseline', '--no-extra-configs', '--dump-outputs', str(out)],
                       env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])['steps'] == steps
    got = {p.stem: np.load(str(p)) for p in out.glob('*.npy')}

    ctx = HipContext(weights_io.synthetic_weights(yolo_yaml.YOLOV5N6_TEST, seed=0), device=0, dtype='fp16', max_batch=B,
                     max_h=S, max_w=S)
    try:
        gen = torch.Generator(device='cuda')
        gen.manual_seed((steps - 1) % 8)
        batch = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device='cuda', generator=gen)
        lb = letterbox_geometry((S, S), new_shape=S, stride=64, auto=True, scaleup=True)
        Hn, Wn = lb['out_hw']
        ctx.preprocess([int(batch[i].data_ptr()) for i in range(B)], [(S, S, lb['new_unpad'][1], lb['new_unpad'][0],
                                                                       lb['top'], lb['left'])] * B, Hn, Wn)
        ctx.forward(B, Hn, Wn)
        det, counts = ctx.nms(B, thr, 0.45, 300)
        torch.cuda.synchronize()
    finally:
        ctx.close()
    assert got['nms_num_detections'].tolist() == counts.tolist() and counts.sum() > 0
    for b in range(B):
        k = int(counts[b])
        assert np.array_equal(got['nms_det'][b, :k], det[b, :k]), b
        dets, max_conf = format_detections(det[b, :k], (Hn, Wn), (S, S, 3), (S, S, 3), thr)
        assert got['num_detections'][b] == len(dets) and got['max_conf'][b] == max_conf
        assert got['conf'][b, :len(dets)].tolist() == [d['conf'] for d in dets]
        assert got['bbox'][b, :len(dets)].tolist() == [d['bbox'] for d in dets]


def test_bench_help_lists_full():
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--help'], env=_env(), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and '--full' in r.stdout, r.stderr[-2000:]


def test_bench_profile_out_needs_full(tmp_path):
    """the per-op timings --profile-out writes come from a pass of their own that only a --full run makes: asked for in a
    plain run, the run is refused before it starts, not left without its file"""
    ops = str(tmp_path / 'ops.json')
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--profile-out', ops, '--rendezvous-check'],
                       env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and '--profile-out needs --full' in r.stderr
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--full', '--profile-out', ops,
                        '--rendezvous-check'], env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and json.loads(r.stdout.strip())['n_gpus'] == 1


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_full_adds_the_rest(tmp_path):
    """a plain run: set-up, warm-up, timed steps, the line -- with the roofline of the timed steps' own events and none of
    the passes after the timed region; --full: the per-stage and per-op timings, --profile-out and the CPU baseline as
    before (extra_configs only belong to the default headline workload, not to this small one)"""
    args = [sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '4',
            '--size', '256', '--model', 'YOLOV5N6_TEST', '--dtype', 'fp16']

    def line(extra):
        r = subprocess.run(args + extra, env=_env(), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out = json.loads(r.stdout.strip().splitlines()[-1])
        assert out['unit'] == 'images/s' and out['higher_is_better'] is True and out['dtype'] == 'fp16'
        assert out['value'] > 0 and out['ms_per_step'] > 0 and out['steps'] == 3 and out['warmup'] == 1
        assert out['metric'].startswith('images/sec (whole node)')
        assert out['roofline']['kernel_ms_per_step'] > 0 and out['extra_configs'] is None
        return out

    plain = line([])
    assert plain['full'] is False and plain['stages'] == {} and plain['cpu_baseline'] is None
    assert plain['roofline']['per_op_conv_ms_per_step'] is None and 'dominant_kernel' not in plain['roofline']
    assert plain['roofline']['stages']['decode'] is None

    ops = tmp_path / 'ops.json'
    full = line(['--full', '--cpu-seconds', '2', '--no-cpu-single-thread', '--profile-out', str(ops)])
    assert full['full'] is True and full['stages']['forward_ms'] > 0 and full['cpu_baseline']['value'] > 0
    assert full['roofline']['per_op_conv_ms_per_step'] > 0 and 'dominant_kernel' in full['roofline']
    assert full['roofline']['stages']['decode'] is not None
    rows = json.loads(ops.read_text())
    assert rows and all('ms' in o for o in rows)
