"""GPU tests that start child processes: sharded chains and sharded training across two processes on one GPU, bench.py starting
its own ranks, a multi-rank rehearsal of bench.py whose chains equal the one-rank run bit for bit, its timed regions and dumps, and
the single-rank RCCL rehearsal (FTHMC_FORCE_PG=1) of bench.py and train_step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from gpu_support import module_defaults

pytestmark = pytest.mark.gpu
_defaults = module_defaults()


# ---------------------------------------------------------------- two processes on one GPU
_WORKER = r'''
import os, sys, math
import numpy as np, torch
sys.path.insert(0, os.environ["FT_ROOT"])
from fthmc_amd import ops, parallel as P
import bench
rank, world, local = P.init()                       # FTHMC_DIST_BACKEND=gloo: both ranks share GPU 0
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
B, L, nl, beta, dt, nstep = 8, 16, 4, 4.0, 0.1, 5
gen = torch.Generator().manual_seed(5)
flow = bench.make_flow(gen, nl)
w = ops.pack_weights(flow, device=dev)
x_all = (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
xi_all = (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
lo, hi = P.shard_range(B, rank, world)
x = x_all[lo:hi].to(dev)
stats = P.RunStats.zeros(dev)
S, _, p, q = ops.ft_action(x, w, nl, beta)
state = torch.stack([S, p, q]).contiguous(); qold = q.clone()
dHs = []
for traj in range(3):
    seeds = P.chain_seeds(77, lo, hi, traj).to(dev)
    v, u = ops.random_momenta(seeds, x.shape)
    r = ops.ft_trajectory(x, v, u, w, nl, beta, dt, nstep, state_in=state)
    x = r["x_new"].clone(); state = r["state"].clone(); dHs.append(r["dH"].clone())
    stats.add(r["acc"], r["plaq"], r["Q"], r["Q"] - qold, r["dH"]); qold = r["Q"].clone()
    h = stats.reduce(async_op=world > 1)
    if h is not None: h.wait()
m = stats.means()
# training: train_step(fused=True) on this rank's share of a fixed prior draw (lr = 0: weights stay put)
from fthmc_amd import train as T
from fthmc_amd.config import TrainConfig
from fthmc_amd.utils import layers as Lyr, qed_helpers as qed
tc = TrainConfig(L=L, beta=beta, n_layers=nl, batch_size=hi - lo)
model = T.get_model(tc)
names = ["net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias"]
model.layers.load_state_dict({f"{li}.plaq_coupling.{n}": flow[li][pi].to(dev) for li in range(nl) for pi, n in enumerate(names)})
opt = torch.optim.SGD(model.layers.parameters(), lr=0.0)
met = T.train_step(model, tc, qed.BatchAction(beta), opt, hi - lo, xi=xi_all[lo:hi].to(dev), fused=True)
grads = torch.cat([p_.grad.reshape(-1) for p_ in model.layers.parameters()])
# the training LOOP object: every rank draws the prior of its own global chain ids on the device and steps the same weights
model2 = T.get_model(tc)
model2.layers.load_state_dict({f"{li}.plaq_coupling.{n}": flow[li][pi].to(dev) for li in range(nl) for pi, n in enumerate(names)})
tc2 = TrainConfig(L=L, beta=beta, n_layers=nl, batch_size=hi - lo, base_lr=1e-3)
tr = T.GraphTrainer(model2, tc2, T.make_optimizer(model2, tc2), hi - lo, seed=9)
for _ in range(3):
    tr.step()
mt = tr.metrics()
np.savez(os.environ["FT_OUT"] + f".{world}.{rank}.npz", lo=lo, hi=hi, x=x.cpu().numpy(), dH=torch.stack(dHs).cpu().numpy(),
         means=np.array([m[k] for k in sorted(m)]), grads=grads.cpu().numpy(), loss=met["loss_dkl"], ess=met["ess"],
         logq=met["logq"], logp=met["logp"], w_loop=Lyr.flow_weights(model2.layers).cpu().numpy(), loop_captured=tr.captured,
         loop_loss=mt["loss_dkl"], loop_ess=mt["ess"])
if world > 1:
    torch.distributed.destroy_process_group()
'''


def _run(world, out, extra_env=None):
    env = dict(os.environ, FT_ROOT=ROOT, FT_OUT=out, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(29700 + world + os.getpid() % 200),
               FTHMC_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', OMP_NUM_THREADS='2')
    env.update(extra_env or {})
    procs = [subprocess.Popen([sys.executable, '-c', _WORKER], env=dict(env, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    for p in procs:
        o, e = p.communicate(timeout=600)
        assert p.returncode == 0, e[-3000:]
    return [dict(np.load(f'{out}.{world}.{r}.npz')) for r in range(world)]


def test_two_process_sharding_equals_one_process(tmp_path):
    """Chains [0, B/2) + [B/2, B) in two fresh processes (HIP trajectories, per-chain Philox seeds, C1 all-reduce over
    gloo) == all B chains in one process, bit for bit; train_step(fused=True) on two half-batches (C2: gradient
    all-reduce, global loss mean and ESS logsumexp) == one process on the full batch."""
    one = _run(1, str(tmp_path / 'a'))[0]
    two = _run(2, str(tmp_path / 'b'))
    x2 = np.concatenate([t['x'] for t in two]); dH2 = np.concatenate([t['dH'] for t in two], axis=1)
    assert [int(t['lo']) for t in two] == [0, 4] and int(two[1]['hi']) == 8
    assert np.array_equal(x2, one['x']) and np.array_equal(dH2, one['dH'])
    for t in two:                                                  # every rank holds the global statistics
        np.testing.assert_allclose(t['means'], one['means'], rtol=1e-13, atol=1e-13)
    assert one['means'][sorted(['n', 'acc', 'plaq', 'q', 'q2', 'absdq', 'dh', 'exp_mdh', 'chi_q']).index('n')] == 24.0
    # training
    np.testing.assert_allclose(np.concatenate([t['logq'] for t in two]), one['logq'], rtol=1e-13)
    np.testing.assert_allclose(np.concatenate([t['logp'] for t in two]), one['logp'], rtol=1e-13)
    for t in two:
        np.testing.assert_allclose(t['loss'], one['loss'], rtol=1e-12)
        np.testing.assert_allclose(t['ess'], one['ess'], rtol=1e-12)
        scale = np.abs(one['grads']).max()
        np.testing.assert_allclose(t['grads'], one['grads'], rtol=1e-10, atol=1e-12 * scale)
    assert np.abs(one['grads']).max() > 0
    # GraphTrainer: captured without a group; over gloo (host-side collectives cannot be captured) the eager sequence -- the same
    # weights, loss and ESS on both ranks as the one process on the full batch (the draws are keyed by the global chain id)
    assert bool(one['loop_captured']) and not any(bool(t['loop_captured']) for t in two)
    for t in two:
        np.testing.assert_allclose(t['w_loop'], one['w_loop'], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(t['loop_loss'], one['loop_loss'], rtol=1e-10)
        np.testing.assert_allclose(t['loop_ess'], one['loop_ess'], rtol=1e-9)


def test_bench_self_launches_its_ranks(tmp_path):
    """`python bench.py --gpus 2` without torchrun starts two ranks itself (gloo rehearsal on this one GPU) and
    reports n_gpus 2; --scaling strong splits a fixed total."""
    env = dict(os.environ, FTHMC_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        env.pop(k, None)
    for scaling, total in (('weak', 32), ('strong', 16)):
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--config', '2', '--batch', '16',
                            '--scaling', scaling, '--steps', '2', '--warmup', '1', '--thermalize', '2', '--no-cpu-baseline', '--full'],
                           env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        line = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
        assert line['n_gpus'] == 2 and line['config']['chains_total'] == total and line['scaling'] == scaling
        assert line['value'] > 0 and line['roofline']['bound'] == 'mfma'


# ---------------------------------------------------------------- bench.py over several ranks == one rank, per chain
def _bench(tmp, tag, gpus, batch, extra=()):
    env = dict(os.environ, FTHMC_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', OMP_NUM_THREADS='2')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT'):
        env.pop(k, None)
    dump = str(tmp / tag)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', str(gpus), '--config', '2', '--batch', str(batch),
                        '--steps', '2', '--warmup', '1', '--thermalize', '3', '--regions', '1', '--no-cpu-baseline', '--dump', dump,
                        *extra], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
    parts = [dict(np.load(f'{dump}.{gpus}.{r}.npz')) for r in range(gpus)]
    return line, parts


def test_bench_multi_rank_rehearsal_equals_one_rank(tmp_path):
    """`bench.py --gpus 4 --config 2 --batch 4` (four ranks sharing this GPU, collectives over gloo: the code path of the
    driver's 8-GPU run up to the backend; at most 6 processes may use a GPU box's card, so 4 ranks here and 8 ranks in
    the CPU test tests/test_host_logic.py::test_eight_rank_gloo_equals_single_process) reports n_gpus 4 and 16 chains,
    and every chain ends where it ends in the one-rank run of the same 16 chains: start field, thermalisation, momenta
    and accept draws are keyed by the global chain id."""
    one, p1 = _bench(tmp_path, 'one', 1, 16)
    four, p4 = _bench(tmp_path, 'four', 4, 4)
    assert four['n_gpus'] == 4 and four['config']['chains_total'] == 16 and four['config']['chains_per_gpu'] == 4
    assert one['n_gpus'] == 1 and one['config']['chains_total'] == 16
    assert [(int(p['lo']), int(p['hi'])) for p in p4] == [(0, 4), (4, 8), (8, 12), (12, 16)]
    for key in ('x0', 'x', 'dH', 'acc', 'Q', 'plaq'):
        got = np.concatenate([p[key] for p in p4])
        assert np.array_equal(got, p1[0][key]), key
    # the global statistics (C1 all-reduce) agree with the one-rank run
    assert abs(four['acceptance'] - one['acceptance']) < 1e-12 and abs(four['plaq'] - one['plaq']) < 1e-9
    assert four['regions']['n'] == 1 and one['value'] > 0 and four['value'] > 0
    # strong scaling keeps the total
    strong, _ = _bench(tmp_path, 'strong', 2, 16, ('--scaling', 'strong'))
    assert strong['n_gpus'] == 2 and strong['config']['chains_total'] == 16 and strong['config']['chains_per_gpu'] == 8


def test_bench_times_several_regions_when_one_is_short(tmp_path):
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--config', '1', '--steps', '5', '--warmup', '2',
                        '--thermalize', '2', '--no-cpu-baseline', '--min-seconds', '0.02', '--full'], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
    reg = line['regions']
    # at least five regions when one is short, and as many as it takes to time --min-seconds of GPU work (default 6 s)
    assert reg['n'] >= 5 and len(reg['seconds']) == reg['n'] and line['steps'] == 5 and sum(reg['seconds']) >= 0.02
    med = sorted(reg['seconds'])[reg['n'] // 2]
    assert abs(line['ms_per_step'] - med / 5 * 1e3) < 1e-2 * line['ms_per_step']
    assert abs(line['value'] - line['config']['chains_total'] * 10 * 5 / med) < 1e-2 * line['value']


def test_bench_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """Without --full the bench times ONE region of exactly --steps trajectories and measures nothing else; --dump-outputs
    writes what the last timed trajectory returned, and two runs with the same arguments write the same arrays."""
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        env.pop(k, None)
    runs = []
    for tag in ('a', 'b'):
        d = tmp_path / tag
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--config', '2', '--steps', '3', '--warmup', '1',
                            '--thermalize', '2', '--dump-outputs', str(d)], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        line = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
        assert line['full'] is False and line['steps'] == 3 and line['regions']['n'] == 1
        assert line['roofline'] is None and line['cpu_baseline'] is None and line['stateless'] is None
        assert abs(line['ms_per_step'] - line['regions']['seconds'][0] / 3 * 1e3) < 1e-3 * line['ms_per_step']
        runs.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = runs
    assert set(a) == {'x_new', 'dH', 'acc', 'H0', 'H1', 'plaq', 'Q', 'state'}
    assert a['x_new'].shape == (32, 2, 16, 16) and a['state'].shape == (3, 32)
    for k in a:
        assert a[k].dtype == np.float64 and np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- single-rank RCCL rehearsal
def _bench_child(tmp_path, tag, env_extra):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', OMP_NUM_THREADS='2', **env_extra)
    env.pop('FTHMC_DIST_BACKEND', None)
    dump = str(tmp_path / tag)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--config', '2', '--steps', '3', '--warmup', '1',
                        '--no-cpu-baseline', '--regions', '1', '--dump', dump], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
    return line, dict(np.load(dump + '.1.0.npz'))


def test_single_rank_nccl_group_rehearses_the_multi_gpu_path(tmp_path):
    """FTHMC_FORCE_PG=1: bench.py creates a ONE-rank `nccl` (= RCCL) process group in a fresh process and takes every
    collective branch of the 8-GPU run -- communicator creation before the capture, the asynchronous C1 all-reduce after
    every graph replay, barrier(device_ids=...), the MAX-reduced region time -- and ends in the same chains, bit for bit,
    as the run without a group."""
    plain, d0 = _bench_child(tmp_path, 'plain', {})
    forced, d1 = _bench_child(tmp_path, 'forced', {'FTHMC_FORCE_PG': '1'})
    assert plain['config']['process_group'] is None and forced['config']['process_group'] == 'nccl'
    assert forced['n_gpus'] == 1 and forced['config']['launch'] == 'hipGraph replay'
    for k in ('x0', 'x', 'dH', 'acc', 'Q', 'plaq'):
        assert np.array_equal(d0[k], d1[k]), k
    assert plain['acceptance'] == forced['acceptance'] and plain['plaq'] == forced['plaq']


_TRAIN_WORKER = r'''
import os, sys, json, hashlib, math
sys.path.insert(0, os.environ['FTHMC_ROOT'])
import torch
from fthmc_amd import ops, parallel, train as T
from fthmc_amd.config import TrainConfig
from fthmc_amd.utils import layers as LY, qed_helpers as qed
parallel.init()
tc = TrainConfig(L=16, beta=4.0, n_layers=4, batch_size=32, base_lr=1e-3, print_freq=0)
torch.manual_seed(17)
model = T.get_model(tc)
opt = torch.optim.Adam(model.layers.parameters(), lr=tc.base_lr)
act = qed.BatchAction(tc.beta)
out = None
for k in range(3):
    xi = ops.random_uniform(parallel.chain_seeds(5, 0, 32, k).cuda(), (32, 2, 16, 16), -math.pi, math.pi)
    out = T.train_step(model, tc, act, opt, 32, xi=xi, fused=True)
# and the loop object: with a group its captured step carries the C2 collectives
tr = T.GraphTrainer(model, tc, T.make_optimizer(model, tc), 32, seed=5)
for _ in range(4):
    tr.step()
m = tr.metrics()
w = LY.flow_weights(model.layers).cpu().numpy()
print(json.dumps({'group': parallel.have_group(), 'backend': torch.distributed.get_backend() if parallel.have_group() else None,
                  'captured': tr.graph is not None, 'w': hashlib.sha256(w.tobytes()).hexdigest(),
                  'loss': float(out['loss_dkl']), 'ess': float(out['ess']), 'loss2': float(m['loss_dkl'])}))
if parallel.have_group():
    torch.distributed.destroy_process_group()
'''


def test_single_rank_nccl_group_train_step():
    """train_step(fused=True) and GraphTrainer under a one-rank `nccl` group: the C2 branches (gradient all-reduce, global
    loss mean, MAX + SUM all-reduces of the ESS logsumexp) run over RCCL -- in GraphTrainer as part of the CAPTURED step, replayed
    -- and leave the same weights, bit for bit, as no group."""
    res = {}
    for tag, extra in (('plain', {}), ('forced', {'FTHMC_FORCE_PG': '1'})):
        env = dict(os.environ, FTHMC_ROOT=ROOT, HSA_ENABLE_IPC_MODE_LEGACY='0', OMP_NUM_THREADS='2', **extra)
        env.pop('FTHMC_DIST_BACKEND', None)
        p = subprocess.run([sys.executable, '-c', _TRAIN_WORKER], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        res[tag] = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
    assert res['plain']['group'] is False and res['plain']['captured'] is True
    assert res['forced']['group'] is True and res['forced']['backend'] == 'nccl' and res['forced']['captured'] is True
    assert res['plain']['w'] == res['forced']['w']
    # with a group the loss mean and the ESS go through torch sums + all-reduces instead of the metrics kernel: rounding only
    for k in ('loss', 'loss2', 'ess'):
        assert abs(res['plain'][k] - res['forced'][k]) <= 1e-12 * max(1.0, abs(res['plain'][k])), k
