"""bench.py --gpus N without torchrun (the driver's scaling command): the process becomes a
launcher of N rank processes (bench.launch_ranks) and itself never touches the GPU. CPU tests
with stub rank commands; the real two-rank run is tests/test_dist.py::test_bench_two_ranks_gloo_one_gpu
(-m gpu). Also the plain run's contract: the headline workload only, --extra refused without --full,
--dump-outputs (-m gpu)."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PARENT = r'''
import json, os, sys
sys.path.insert(0, {root!r})
sys.argv = ['bench.py', '--gpus', '{n}', '--steps', '1', '--warmup', '0']
import torch
import bench
stub = [sys.executable, '-c', {stub!r}]
orig = bench.launch_ranks
bench.launch_ranks = lambda n, argv: orig(n, argv, cmd=stub, poll_s=0.05)
code = 0
try:
    bench.main()
except SystemExit as e:
    code = e.code
# the launcher made no HIP call: no device context, the HIP library never loaded
print(json.dumps({{'parent_rc': code, 'cuda_initialized': torch.cuda.is_initialized(),
                  'hip_lib_loaded': bench._hip._LIB is not None}}))
'''

_RANK_OK = ("import os, json; print(json.dumps({k: os.environ[k] for k in "
            "('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}), flush=True)")
_RANK_FAILS = ("import os, sys, time\n"
               "if os.environ['RANK'] == '1': sys.exit(3)\n"
               "time.sleep(120)")


def _run_parent(n, stub, timeout=60):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT')}
    env['HIP_VISIBLE_DEVICES'] = ''
    src = _PARENT.format(root=ROOT, n=n, stub=stub)
    return subprocess.run([sys.executable, '-c', src], cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=timeout)


def test_launcher_starts_n_ranks_and_forwards_rank0():
    r = _run_parent(3, _RANK_OK)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    # stdout: rank 0's line (forwarded) then the parent's report; ranks 1, 2 went to stderr
    assert len(out) == 2, r.stdout
    rank0, parent = out
    assert rank0['RANK'] == '0' and rank0['LOCAL_RANK'] == '0' and rank0['WORLD_SIZE'] == '3'
    assert rank0['MASTER_ADDR'] == '127.0.0.1' and int(rank0['MASTER_PORT']) > 0
    others = [json.loads(ln) for ln in r.stderr.splitlines() if ln.startswith('{"RANK"')]
    assert sorted(o['RANK'] for o in others) == ['1', '2']
    assert all(o['MASTER_PORT'] == rank0['MASTER_PORT'] and o['WORLD_SIZE'] == '3' for o in others)
    assert parent == {'parent_rc': 0, 'cuda_initialized': False, 'hip_lib_loaded': False}


def test_launcher_fails_fast_when_a_rank_fails():
    t0 = time.time()
    r = _run_parent(2, _RANK_FAILS)
    assert time.time() - t0 < 40  # rank 0 (sleeping 120 s) was stopped, not waited for
    parent = json.loads(r.stdout.strip().splitlines()[-1])
    assert parent['parent_rc'] == 3 and not parent['cuda_initialized']
    assert 'rank 1 exited with 3' in r.stderr


def test_plain_run_refuses_extra_workloads():
    """Without --full the benchmark runs the headline workload only: asking for --extra workloads
    is an error (before any HIP call), not a silently shorter run."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES='')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--extra', 'c3:fp32'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and '--extra workloads run only with --full' in r.stderr, r.stderr[-2000:]


@pytest.fixture(scope='module')
def dump_runs(tmp_path_factory):
    """Two plain runs with the same arguments and --dump-outputs, each in a process of its own:
    [(completed process, output directory)] (run once, shared by the tests below)."""
    env = {k: v for k, v in os.environ.items()
           if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT', 'RSYS_DETERMINISTIC')}
    runs = []
    for i in range(2):
        out = tmp_path_factory.mktemp(f'dump{i}') / 'out'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '8', '--warmup',
                            '2', '--dump-outputs', str(out)], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=200)
        assert r.returncode == 0, r.stderr[-3000:]
        runs.append((r, out))
    return runs


@pytest.mark.gpu
def test_dumped_outputs_are_the_same_every_run(dump_runs):
    """Same arguments, same seeded model and batches: a --dump-outputs run steps through the
    fixed-order table-gradient kernels (bench.py sets RSYS_DETERMINISTIC=1 for it and reports
    config.deterministic), so after 3 eager and 10 replayed steps with dropout every dumped array
    is bitwise the same in two processes."""
    import numpy as np
    (r0, a), (r1, b) = dump_runs
    for r in (r0, r1):
        d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][0])
        assert d['config']['deterministic'] is True and d['config']['hip_graph'] is True
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for f in sorted(os.listdir(a)):
        x, y = np.load(a / f), np.load(b / f)
        assert x.shape == y.shape and np.array_equal(x, y), (f, float(np.abs(x - y).max()))


def _bench(*argv, **env_over):
    env = {k: v for k, v in os.environ.items()
           if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT', 'RSYS_DETERMINISTIC')}
    env.update(env_over)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'] + list(argv), cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return r, json.loads(lines[0])


@pytest.mark.gpu
def test_dump_from_the_default_kernels_on_request(tmp_path):
    """RSYS_DETERMINISTIC=0 in the environment is respected: the dump run keeps the float-atomic
    table gradients a plain run times (config.deterministic false) and writes the same files."""
    import numpy as np
    out = tmp_path / 'out'
    _, d = _bench('--steps', '2', '--warmup', '1', '--dump-outputs', str(out), RSYS_DETERMINISTIC='0')
    assert d['config']['deterministic'] is False and d['config']['hip_graph'] is True
    assert sorted(os.listdir(out)) == ['item_emb.npy', 'loss.npy', 'params.npy', 'user_emb.npy']
    assert all(np.isfinite(np.load(out / f)).all() for f in os.listdir(out))


@pytest.mark.gpu
def test_full_run_reports_kernels_and_rooflines():
    """--full (here without the CPU baselines and the extra workloads): the measured peaks, the
    instrumented pass's per-kernel times and every roofline object, in the stdout line's summary and
    in the whole record on stderr ({"bench_detail": ...}); the headline fields as in a plain run."""
    r, d = _bench('--steps', '3', '--warmup', '1', '--full', '--no-cpu-baseline', '--extra=')
    assert d['steps'] == 3 and d['ms_per_step'] > 0 and d['value'] > 0 and d['dtype'] == 'bf16'
    assert d['config']['deterministic'] is False
    assert d['roofline']['kernel'] and 0 < d['roofline']['frac'] <= 1
    assert d['gather_roofline']['rs_gather_fwd']['frac'] > 0 and d['step_roofline']['frac'] > 0
    assert d['peaks_measured']['hbm_copy_GBs'] > 0 and d['peaks_measured']['bf16_mfma_TFLOPs'] > 0
    assert d['cpu_baseline'] is None and 'extra' not in d
    det = [json.loads(ln)['bench_detail'] for ln in r.stderr.splitlines() if ln.startswith('{"bench_detail"')]
    assert len(det) == 1
    det = det[0]
    k = det['kernel_ms_per_step']
    assert len(k) > 10 and all(v >= 0 for v in k.values()) and det['roofline']['kernel'] in k
    for name in ('rs_gather_fwd', 'rs_gather_bwd', 'rs_attn_fwd', 'rs_attn_bwd', 'rs_tower_fwd', 'rs_tower_bwd'):
        assert k.get(name, 0) > 0, name
    # the instrumented kernels' event time is of the order of the timed step (towers serial there)
    assert 0.3 * det['ms_per_step'] < sum(k.values()) < 5 * det['ms_per_step']
    for obj in ('roofline', 'gather_roofline', 'batch_dot_roofline', 'softmax_roofline', 'step_roofline'):
        assert det[obj], obj
    assert det['ms_per_step'] == d['ms_per_step'] and det['peaks_measured']['how']


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_outputs(dump_runs):
    """A plain run (no --full) times the headline workload only: its line has the contract's fields
    and none of the --full objects, and nothing else is measured (no peaks, instrumented pass, extra
    workload or bench_detail record). --dump-outputs writes the last timed step's loss, tower
    outputs and updated parameters as float32 .npy files, within 64 MB in all."""
    import numpy as np
    r, out = dump_runs[0]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['steps'] == 8 and d['warmup'] == 2 and d['n_gpus'] == 1 and d['ms_per_step'] > 0 and d['value'] > 0
    assert d['unit'] == 'samples/s' and d['higher_is_better'] is True and d['dtype'] == 'bf16'
    assert abs(d['value'] - d['config']['global_batch'] / (d['ms_per_step'] * 1e-3)) <= 2e-3 * d['value']
    for k in ('roofline', 'gather_roofline', 'step_roofline', 'cpu_baseline', 'peaks_measured', 'extra'):
        assert k not in d, k
    assert 'bench_detail' not in r.stderr and 'instrumented' not in r.stderr and 'setting up' in r.stderr
    assert r.stderr.count('setting up') == 1  # one workload
    assert sorted(os.listdir(out)) == ['item_emb.npy', 'loss.npy', 'params.npy', 'user_emb.npy']
    a = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20
    B = d['config']['per_gpu_batch']
    assert a['loss'].shape == (1,) and a['loss'][0] > 0
    assert a['user_emb'].shape == a['item_emb'].shape and a['user_emb'].shape[0] == B and a['user_emb'].ndim == 2
    assert a['params'].ndim == 1 and a['params'].size > 100_000 and np.abs(a['params']).max() > 0


def test_bench_gpus_must_match_world(monkeypatch):
    """Under torchrun, --gpus must equal WORLD_SIZE (the line's n_gpus is the process group's)."""
    src = ("import sys; sys.path.insert(0, %r); sys.argv = ['bench.py', '--gpus', '2']\n"
           "import bench\n"
           "bench.rdist.init_from_env = lambda: None\n"
           "bench.main()\n") % ROOT
    env = dict(os.environ, WORLD_SIZE='1', HIP_VISIBLE_DEVICES='')
    r = subprocess.run([sys.executable, '-c', src], cwd=ROOT, env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and '--gpus 2 but the process group has 1 ranks' in r.stderr
