"""CPU-only tests: host logic of the package (config types, stripe masks, weight packing,
sharding, multi-process statistics over gloo) and that the C-ABI library loads and exports
every symbol include/fthmc_hip.h declares.  No compute calls: there is no GPU here."""
import os
import shutil
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden


def test_library_loads_and_exports_every_declared_symbol():
    from fthmc_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
    declared = set(re.findall(r'\b(fthmc_[a-z0-9_]+)\s*\(', header))
    assert len(declared) >= 25
    for name in sorted(declared):
        assert hasattr(lib, name), f'{name} declared in include/fthmc_hip.h but not exported'
        assert name in _lib.SIGNATURES, f'{name} has no ctypes signature'
    assert set(_lib.SIGNATURES) <= declared
    assert lib.fthmc_version().startswith(b'fthmc_hip')
    assert lib.fthmc_ws_bytes(None, 128, 64, 8) > 128 * 2 * 64 * 64 * 8 * 9
    # the net shape is an argument of the call (fthmc_arch_t), sizes follow it, limits are refused, nothing is remembered
    from fthmc_amd import ops
    assert lib.fthmc_arch_params(None) == 955 == lib.fthmc_arch_params(ops._arch(((8, 8), 3, 2)) or None)
    assert lib.fthmc_arch_params(ops._arch(((4, 6, 5), 5, 1))) == ops.arch_params(((4, 6, 5), 5, 1))
    assert lib.fthmc_ws_bytes(ops._arch(((16, 16), 3, 2)), 8, 16, 4) != lib.fthmc_ws_bytes(None, 8, 16, 4) > 0
    assert lib.fthmc_arch_params(ops._arch(((8, 8), 17, 2))) < 0 and lib.fthmc_ws_bytes(ops._arch(((8, 8), 4, 2)), 8, 16, 4) == 0
    assert lib.fthmc_arch_params(None) == 955
    assert b'workspace' in lib.fthmc_strerror(-4)


def test_compiled_torch_library_loads_and_defines_every_operator():
    """libfthmc_torch.so (csrc/torch_library.cpp, built by csrc/Makefile): the compiled TORCH_LIBRARY(fthmc_hip) loads on a CPU
    box, defines all eleven operators with the net shape in their schemas, and a CPU tensor is refused by the dispatcher."""
    so = os.path.join(ROOT, 'fthmc_amd', 'libfthmc_torch.so')
    if not os.path.exists(so):
        pytest.skip('libfthmc_torch.so not built (make -C fthmc_amd/csrc)')
    import fthmc_amd.torch_ops as T
    assert T.BACKEND == 'compiled'
    for name in T.__all__:
        op = getattr(torch.ops.fthmc_hip, name).default
        assert op._schema.name == 'fthmc_hip::' + name
    sch = str(torch.ops.fthmc_hip.fthmc_trajectory.default._schema)
    assert 'int[]? hidden=None' in sch and 'int kernel_size=3' in sch and 'int n_mix=2' in sch
    with pytest.raises(NotImplementedError):
        torch.ops.fthmc_hip.wilson_force(torch.zeros(1, 2, 8, 8, dtype=torch.float64), 1.0)


def test_no_cpu_fallback():
    from fthmc_amd import ops
    from fthmc_amd._lib import FthmcError
    with pytest.raises(FthmcError):
        ops.wilson_action_charge(torch.zeros(1, 2, 8, 8, dtype=torch.float64), 1.0)
    # nothing under fthmc_amd/ may import the oracle
    for dp, _, files in list(os.walk(os.path.join(ROOT, 'fthmc_amd'))) + list(os.walk(os.path.join(ROOT, 'fthmc'))):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dp, f)).read()
                assert 'oracle' not in src, f'{f} mentions the oracle'


def test_masks_match_reference():
    from fthmc_amd.utils import layers as Lyr
    g = load_golden('masks')
    for L in (8, 12):
        for mu in (0, 1):
            for off in range(4):
                pm = Lyr.make_plaq_masks((L, L), mu, off)
                k = f'L{L}_mu{mu}_off{off}_'
                assert np.array_equal(pm['active'], g[k + 'active'])
                assert np.array_equal(pm['frozen'], g[k + 'frozen'])
                assert np.array_equal(pm['passive'], g[k + 'passive'])
                assert np.array_equal(Lyr.make_2d_link_active_stripes((2, L, L), mu, off), g[k + 'link'])


def test_config_types():
    from fthmc_amd import config as C
    g = load_golden('plaq_exact')
    assert [C.PLAQ_EXACT[float(b)] for b in g['betas']] == list(g['values'])
    p = C.Param(beta=2.0, L=8, tau=1.0, nstep=10)
    assert p.dt == 0.1 and p.volume == 64 and p.shape == [2, 8, 8] and p.lat == [8, 8]
    assert p.uniquestr() == 't8x8_b2.0_n256_t1.0_s10'
    lf = C.lfConfig(tau=2.0, nstep=8)
    assert lf.dt == 0.25 and lf.uniquestr() == 't2.0_s8_dt0.25'
    cwd_before = set(os.listdir('.'))
    tc = C.TrainConfig(L=16, beta=4.0, n_layers=4)
    assert tc.volume == 256 and tc.hidden_sizes == [8, 8] and tc.n_s_nets == 2
    assert set(os.listdir('.')) == cwd_before          # no directories created (reference Q11)
    assert 'L16_b4.0' in tc.uniquestr()


def test_pack_weights_layout_and_checks():
    from fthmc_amd import ops
    from fthmc_amd._lib import FthmcError
    w = [torch.arange(144.).reshape(8, 2, 3, 3), torch.arange(8.), torch.arange(576.).reshape(8, 8, 3, 3),
         torch.arange(8.), torch.arange(216.).reshape(3, 8, 3, 3), torch.arange(3.)]
    flat = ops.pack_weights([w, w])
    assert flat.shape == (2 * 955,) and flat.dtype == torch.float64
    assert float(flat[144 + 3]) == 3.0 and float(flat[152 + 575]) == 575.0 and float(flat[954]) == 2.0
    back = ops.unpack_weight_grads(flat, 2)
    assert all(torch.equal(a.double(), b) for a, b in zip(w, back[1]))
    with pytest.raises(FthmcError):
        ops.pack_weights([[torch.zeros(16, 2, 3, 3)] + w[1:]])


def test_shard_ranges_and_chain_seeds():
    from fthmc_amd import parallel as P
    for n, ws in [(128, 8), (1024, 8), (10, 3), (5, 8)]:
        spans = [P.shard_range(n, r, ws) for r in range(ws)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    # a chain's seed depends on its global id and the trajectory only, not on the sharding
    full = P.chain_seeds(1331, 0, 1024, 7)
    for r in range(8):
        lo, hi = P.shard_range(1024, r, 8)
        assert torch.equal(P.chain_seeds(1331, lo, hi, 7), full[lo:hi])
    assert len(set(full.tolist())) == 1024 and not torch.equal(full, P.chain_seeds(1331, 0, 1024, 8))


_WORKER = r'''
import os, sys, math
import torch, torch.distributed as dist
sys.path.insert(0, os.environ["FT_ROOT"])
from fthmc_amd import parallel as P
from oracle import ref_cpu as R            # the oracle stands in for the GPU trajectory in this CPU test
rank, world, _ = P.init("gloo")
B, L, nl, beta, dt, nstep = int(os.environ.get("FT_B", "4")), 8, 2, 2.0, 0.1, 3
gen = torch.Generator().manual_seed(11)
flow = R.default_flow(nl, gen)
x_all = (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
lo, hi = P.shard_range(B, rank, world)
stats = P.RunStats.zeros("cpu")
gw_local = torch.zeros(3)
qold = R.charge(R.flow_forward(x_all[lo:hi], flow)[0])
for traj in range(2):
    seeds = P.chain_seeds(5, lo, hi, traj)
    v = torch.stack([torch.randn(2, L, L, generator=torch.Generator().manual_seed(int(s)), dtype=torch.float64) for s in seeds])
    u = torch.stack([torch.rand([], generator=torch.Generator().manual_seed(int(s) ^ 1), dtype=torch.float64) for s in seeds])
    dH, _, acc, newx, _, _ = R.ft_hmc(x_all[lo:hi], v, u, flow, beta, dt, nstep)
    y = R.flow_forward(newx, flow)[0]
    q = R.charge(y)
    stats.add(acc.double(), R.plaq_mean(y, beta), q, q - qold, dH)
    w = stats.reduce(async_op=world > 1)
    if w is not None: w.wait()
    qold = q
m = stats.means()
lw = torch.arange(lo, hi, dtype=torch.float64) * 0.3
lse = float(P.global_logsumexp(lw)); mean = float(P.global_mean(lw, B))
ess = float(P.global_ess(1000.0 * torch.sin(torch.arange(lo, hi, dtype=torch.float64)), B))     # one all-gather (C2 of a training step)
g = torch.full((3,), float(rank + 1)); P.allreduce_grads(g)
# the C2 collectives of a captured training step run on a process group of their own (parallel.capture_group): same numbers
if world > 1:
    cg = P.capture_group()
    assert cg is not None and cg is P.capture_group() and cg is not dist.group.WORLD
    g2 = torch.full((3,), float(rank + 1)); P.allreduce_grads(g2, group=cg)
    ess2 = float(P.global_ess(1000.0 * torch.sin(torch.arange(lo, hi, dtype=torch.float64)), B, group=cg))
    assert float(g2[0]) == float(g[0]) and ess2 == ess, (float(g2[0]), float(g[0]), ess2, ess)
else:
    assert P.capture_group() is None
if rank == 0:
    print("RESULT", m["n"], m["acc"], m["plaq"], m["q"], m["dh"], lse, mean, float(g[0]), ess)
if world > 1:
    dist.barrier()                       # nobody tears a group down while a peer is still inside a collective of it
    dist.destroy_process_group(P.capture_group())
    dist.destroy_process_group()
'''


def _run_workers(world, B=4):
    env = dict(os.environ, FT_ROOT=ROOT, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(29500 + world + os.getpid() % 500),
               OMP_NUM_THREADS='1', FT_B=str(B))
    procs = []
    for r in range(world):
        e = dict(env, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, '-c', _WORKER], env=e, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    for p, (o, err) in zip(procs, outs):
        assert p.returncode == 0, err[-2000:]
    line = [l for l in outs[0][0].splitlines() if l.startswith('RESULT')][0]
    return [float(t) for t in line.split()[1:]]


def test_two_rank_gloo_equals_single_process():
    """Chains sharded over 2 ranks (gloo) + C1 all-reduce == the same chains in one process."""
    one = _run_workers(1)
    two = _run_workers(2)
    assert one[0] == two[0] == 8.0                                   # 4 chains x 2 trajectories
    np.testing.assert_allclose(two[:7], one[:7], rtol=1e-12, atol=1e-12)
    assert one[7] == 1.0 and two[7] == 3.0                           # SUM all-reduce of "gradients"
    # calc_ess (distributions.py:27-37) of the whole batch: exp(2 lse(logw) - lse(2 logw)) / B
    lw = 1000.0 * torch.sin(torch.arange(4, dtype=torch.float64))
    want = float(torch.exp(2 * torch.logsumexp(lw, 0) - torch.logsumexp(2 * lw, 0)) / 4)
    np.testing.assert_allclose([one[8], two[8]], [want, want], rtol=1e-12)


def test_eight_rank_gloo_equals_single_process():
    """BASELINE configs[3] shape of the job: the chains sharded over EIGHT ranks (gloo on the CPU; async C1 all-reduce
    every trajectory, C2 SUM, global logsumexp / mean) == the same chains in one process."""
    one = _run_workers(1, B=16)
    eight = _run_workers(8, B=16)
    assert one[0] == eight[0] == 32.0                                # 16 chains x 2 trajectories
    np.testing.assert_allclose(eight[:7], one[:7], rtol=1e-12, atol=1e-12)
    assert eight[7] == 36.0                                          # SUM over ranks of rank + 1
    np.testing.assert_allclose(eight[8], one[8], rtol=1e-12)         # the ESS from one all-gather of three doubles per rank


def test_reference_import_path_is_an_alias_of_this_package():
    """`fthmc.X` (the reference's import path, fthmc/main.py:18-33) resolves to the module object `fthmc_amd.X`."""
    import importlib
    import fthmc
    import fthmc_amd
    from fthmc.config import PLAQ_EXACT, Param, TrainConfig, lfConfig            # noqa: F401
    from fthmc.ft_hmc import FieldTransformation, run_ftHMC                        # noqa: F401
    from fthmc.hmc import run_hmc                                                  # noqa: F401
    from fthmc.train import get_model, train, train_step, transfer_to_new_lattice  # noqa: F401
    import fthmc.utils.qed_helpers as qed
    import fthmc.utils.layers as layers
    from fthmc.utils.distributions import MultivariateUniform, calc_dkl, calc_ess  # noqa: F401
    from fthmc.utils.samplers import apply_flow_to_prior, make_mcmc_ensemble       # noqa: F401
    import fthmc_amd.ft_hmc
    import fthmc_amd.utils.layers
    import fthmc_amd.utils.qed_helpers
    assert sys.modules['fthmc.ft_hmc'] is fthmc_amd.ft_hmc and qed is fthmc_amd.utils.qed_helpers
    assert layers is fthmc_amd.utils.layers and fthmc.utils is fthmc_amd.utils
    assert qed.__spec__.name == 'fthmc_amd.utils.qed_helpers'      # the real spec survives: reload works
    importlib.reload(qed)
    for name in ('ft_action', 'ft_force', 'ft_flow', 'ft_flow_inv', 'BatchAction', 'batch_charges', 'regularize',
                 'leapfrog', 'hmc', 'force', 'action'):
        assert hasattr(qed, name), name
    with pytest.raises(ModuleNotFoundError):
        import fthmc.main                                                           # noqa: F401  (out of scope: raises)
    # the alias holds no code of its own besides the finder
    src = open(os.path.join(ROOT, 'fthmc', '__init__.py')).read()
    assert 'def ' in src and src.count('\n') < 80 and os.listdir(os.path.join(ROOT, 'fthmc')) in (['__init__.py'], ['__init__.py', '__pycache__'], ['__pycache__', '__init__.py'])


def test_checkpoint_history_loads_without_unpickling_code(tmp_path):
    """save_checkpoint stores histories as tensors / plain numbers: the file loads with weights_only=True."""
    from fthmc_amd import train as T
    hist = {'loss': [np.float64(1.5), 2.0], 'q': [np.arange(3.0)], 'nested': {'a': (np.int64(3), 'x')}}
    path = tmp_path / 'h.tar'
    torch.save({'history': T._plain(hist)}, path)
    back = torch.load(path, weights_only=True)['history']
    assert back['loss'] == [1.5, 2.0] and torch.equal(back['q'][0], torch.arange(3.0, dtype=torch.float64))
    assert back['nested']['a'] == (3, 'x')
    torch.save({'history': hist}, path)                              # what the reference writes: numpy pickles
    with pytest.raises(Exception):
        torch.load(path, weights_only=True)


def test_torch_operator_library_registers_without_a_gpu():
    """torch.ops.fthmc_hip.*: schemas exist, shapes propagate on fake tensors, and there is no CPU kernel."""
    import fthmc_amd.torch_ops as T
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in T.__all__:
        assert hasattr(torch.ops.fthmc_hip, name), name
    sch = str(torch.ops.fthmc_hip.fthmc_trajectory.default._schema)
    assert sch.startswith('fthmc_hip::fthmc_trajectory(Tensor x, Tensor v, Tensor u, Tensor w_all')
    with FakeTensorMode():
        x = torch.empty(3, 2, 8, 8, dtype=torch.float64)
        y, lj = torch.ops.fthmc_hip.flow_layer_fwd(x, torch.empty(955, dtype=torch.float64), 0, 1, 2, 0)
        assert y.shape == x.shape and lj.shape == (3,)
        out = torch.ops.fthmc_hip.train_grad(x, torch.empty(4 * 955, dtype=torch.float64), 4, 2.0, 0)
        assert out[3].shape == (4 * 955,)
    with pytest.raises(NotImplementedError):
        torch.ops.fthmc_hip.wilson_force(torch.zeros(1, 2, 8, 8, dtype=torch.float64), 1.0)


def test_observables_tooling(tmp_path):
    """delta-Q^2 versus lag and the susceptibility on a synthetic charge history with a known answer."""
    from fthmc_amd.utils import observables as O
    rng = np.random.default_rng(3)
    # a random walk with unit steps with probability 1/2: <(Q(t+k) - Q(t))^2> = k / 2
    steps = rng.integers(0, 2, size=(20000, 4)) * rng.choice([-1, 1], size=(20000, 4))
    q = np.cumsum(steps, axis=0).astype(np.float64)
    rows = O.change_sqr_vs_dt(q, dt_range=4)
    for lag, mean, sig in rows:
        assert abs(mean - lag / 2) < 5 * sig + 0.02, (lag, mean, sig)
    assert np.isnan(O.change_sqr(q[:3], 5)[0])
    bm = O.block_means(np.arange(35.0), 16)                   # 35 = 3 dropped + 16 blocks of 2
    assert bm.shape == (16,) and bm[0] == 3.5 and bm[-1] == 33.5
    # iid integer charges with variance 2 on a volume of 64: chi = 2 / 64
    qq = rng.normal(0, np.sqrt(2.0), size=40000)
    chi, err = O.topological_susceptibility(qq, 64, nboot=50, binsize=8)
    assert abs(chi - 2 / 64) < 5 * err + 1e-3
    out = O.save_topo_change_sqr(str(tmp_path / 'dq2.txt'), q[:, 0], dt_range=3)
    assert len(out) == 3 and len(open(tmp_path / 'dq2.txt').read().splitlines()) == 3


@pytest.mark.parametrize('name', ['r01_bench.json', 'r02_bench.json', 'r02_bench_config5.json', 'r03_bench.json',
                                  'r03_bench_config2.json', 'r03_bench_config5.json', 'r05_bench.json', 'r05_bench_config3.json',
                                  'r05_bench_config2.json', 'r05_bench_config5.json'])
def test_committed_bench_line_follows_the_contract(name):
    """profiles/rNN_bench*.json is one JSON line of bench.py: every key the driver and the judge read is there,
    and the numbers are mutually consistent."""
    import json
    line = open(os.path.join(ROOT, 'profiles', name)).read().strip().splitlines()[-1]
    d = json.loads(line)
    if not name.startswith('r01'):
        assert d['cpu_baseline']['parity']['ok'] is True and d['cpu_baseline']['one_thread']['cores'] == 1
        assert d['config']['baseline_config'] in (2, 3, 5) and ('train' in d) == (d['config']['baseline_config'] == 5)
        if d['config']['baseline_config'] == 2:                # small lattice: the fused single-launch kernel is the dominant one
            assert d['roofline']['kernel'].startswith('k_ft_small<16>') and d['config']['path'].startswith('small-lattice')
        else:
            assert d['roofline']['attainable']['kernel'].startswith('k_flow_fwd') and 'traffic_source' in d['roofline']
    if name.startswith('r05'):
        # round 5: regions are timed until 6 s of GPU work have accumulated; the dominant kernel's launch time is carried twice
        # (HIP events of this run, rocprofv3 of the committed summary) and frac_rocprof follows from the latter to the digit
        reg = d['regions']
        assert sum(reg['seconds']) >= 6.0 or reg['n'] == 400
        r5 = d['roofline']
        if d['config']['baseline_config'] == 3:
            assert r5['rocprof_source']['file'] == 'profiles/r05_kernel_stats.csv' and r5['rocprof_source']['stale'] is False
            want = r5['algorithmic_flops_per_launch'] / (r5['rocprof_avg_launch_ms'] * 1e-3) / 1e12 / r5['peak']
            assert abs(r5['frac_rocprof'] - want) < 1e-3 and abs(r5['frac_rocprof'] - r5['frac']) < 0.05 * r5['frac']
            assert r5['traffic_source']['stale'] is False
        elif d['config']['baseline_config'] == 5:
            assert r5['rocprof_avg_launch_ms'] is None and d['train']['wall']['launch'].startswith('hipGraph replay')
    if name.startswith('r03') or name.startswith('r05'):
        reg = d['regions']
        assert reg['n'] == len(reg['seconds']) >= 1 and reg['value_from'] == 'median region'
        assert abs(d['ms_per_step'] - sorted(reg['seconds'])[len(reg['seconds']) // 2] / d['steps'] * 1e3) < 1e-3 * d['ms_per_step']
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in d, k
    assert d['higher_is_better'] is True and d['scaling'] == 'weak' and d['dtype'] == 'f64' and d['data'] == 'synthetic'
    assert d['vs_baseline'] is None                       # BASELINE.md publishes no number for this metric
    assert 'workload' in d['config'] and 'model' not in d['config']
    r = d['roofline']
    for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
        assert k in r, k
    assert r['bound'] in ('hbm', 'mfma') and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-3
    assert abs(r['achieved'] - r['algorithmic_flops_per_launch'] / (r['avg_launch_ms'] * 1e-3) / 1e12) < 0.1
    c = d['cpu_baseline']
    for k in ('value', 'unit', 'cores', 'kind', 'sample'):
        assert k in c, k
    assert c['kind'] in ('reference', 'port') and c['unit'] == d['unit']
    # value = chains x leapfrog steps x trajectories / time
    cfg = d['config']
    assert abs(d['value'] - cfg['chains_total'] * cfg['nstep'] / (d['ms_per_step'] * 1e-3)) / d['value'] < 1e-3


def test_independence_sampler_accept_chain_on_recorded_reference_run():
    """Host logic of utils.samplers.make_mcmc_ensemble: the recorded proposals and uniforms of a reference run
    (tests/golden/make_golden.py section 9) give the reference's accept sequence and histories."""
    from fthmc_amd.utils import samplers as S
    g = load_golden('sampler_L8')
    n = len(g['logq'])
    props = [(torch.from_numpy(g['xi'][i]), torch.tensor(g['logq'][i]), torch.tensor(g['logp_xi'][i]),
              torch.tensor(g['q_xi'][i])) for i in range(n)]
    h = S.make_mcmc_ensemble(None, None, int(g['batch_size']), n, proposals=props, uniforms=list(g['u']), keep_x=True)
    assert np.array_equal(h['acc'], g['hist_acc'])
    for k in ('q', 'dqsq', 'logq', 'logp'):
        np.testing.assert_allclose(h[k], g['hist_' + k], rtol=2e-7, atol=1e-6)     # float32 reference histories
    assert h['x'].shape == (n, 2, 8, 8)
    rej = np.where(g['hist_acc'] == 0)[0]
    assert len(rej) and all(torch.equal(h['x'][i], h['x'][i - 1]) for i in rej)    # a reject repeats the configuration


def test_bench_launch_command_and_refusal_without_gpu():
    """bench.py --gpus N: the parent builds a one-node torchrun command with N ranks; on a box without a GPU
    the job fails loudly instead of printing a 1-GPU number."""
    import bench
    cmd = bench.launch_command(4, ['--gpus', '4', '--steps', '2'], 29511)
    assert cmd[1:4] == ['-m', 'torch.distributed.run', '--nnodes=1'] and '--nproc-per-node=4' in cmd
    assert cmd[-4:] == ['--gpus', '4', '--steps', '2'] and '127.0.0.1' in cmd
    assert set(bench.CONFIGS) == {1, 2, 3, 5} and bench.CONFIGS[3]['B'] == 128 and bench.CONFIGS[5]['L'] == 256
    # the self-launching parent starts a CHILD job and never replaces itself (forbidden on the GPU pool once a runtime
    # is up), and it counts devices without initialising one
    src = open(os.path.join(ROOT, 'bench.py')).read()
    import re
    assert not re.search(r'\bos\.(exec[a-z]*|spawn[a-z]*|posix_spawn)\s*\(', src)
    launch_src = src[src.index('def self_launch'):src.index('def host_threads')]
    assert 'torch.cuda' not in launch_src and 'subprocess.run' in launch_src
    n = bench.visible_gpus()
    assert n is None or n >= 0
    os.environ['HIP_VISIBLE_DEVICES'] = '0,3'
    try:
        assert bench.visible_gpus() == 2
    finally:
        del os.environ['HIP_VISIBLE_DEVICES']
    assert len(bench.csrc_sha16()) == 16
    if not torch.cuda.is_available():
        env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '1', '--warmup', '0'],
                           env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode != 0 and 'MI355X' in (p.stderr + p.stdout)


def test_bench_is_plain_unless_asked_for_full(monkeypatch):
    """bench.py's options: a plain run times one region of --steps and nothing else; --full asks for the extra measurements,
    --dump-outputs DIR for the last timed trajectory's arrays."""
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    assert a.regions is None and a.min_seconds is None
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', '/nonexistent/out'])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == '/nonexistent/out'


def test_net_shapes_and_their_limits():
    """Any s/t net the reference's make_conv_net accepts is packed for the HIP path (the default shape for the tuned kernels,
    anything else for csrc/flow_generic.hip); what the kernels cannot take raises before anything is launched -- never a
    silent fallback (fthmc/utils/layers.py:138-167, 399-429)."""
    from fthmc_amd import ops
    from fthmc_amd._lib import FthmcError
    from fthmc_amd.utils import layers as Lyr
    for kw in (dict(hidden_sizes=[8] * 9), dict(hidden_sizes=[300, 8]), dict(kernel_size=17), dict(n_mixture_comps=0),
               dict(n_mixture_comps=65)):
        args = dict(n_layers=2, n_mixture_comps=2, lattice_shape=(8, 8), hidden_sizes=[8, 8], kernel_size=3)
        args.update(kw)
        with pytest.raises(NotImplementedError, match='limits of the HIP kernels'):
            Lyr.make_u1_equiv_layers(**args)
    z = torch.zeros
    w = [z(8, 2, 3, 3), z(8), z(8, 8, 3, 3), z(8), z(3, 8, 3, 3), z(3)]
    assert ops.arch_of(ops.pack_weights([w])) == ops.DEFAULT_ARCH == ((8, 8), 3, 2) and ops.arch_params() == 955
    w3 = [z(8, 2, 3, 3), z(8), z(8, 8, 3, 3), z(8), z(4, 8, 3, 3), z(4)]                  # n_mixture_comps = 3
    p = ops.pack_weights([w3, w3])
    assert ops.arch_of(p) == ((8, 8), 3, 3) and p.numel() == 2 * ops.arch_params(((8, 8), 3, 3)) == 2 * (152 + 584 + 292)
    w5 = [z(4, 2, 5, 5), z(4), z(6, 4, 5, 5), z(6), z(5, 6, 5, 5), z(5), z(2, 5, 5, 5), z(2)]   # three hidden layers, k = 5, one component
    p = ops.pack_weights([w5])
    assert ops.arch_of(p) == ((4, 6, 5), 5, 1)
    assert [tuple(t.shape) for t in ops.unpack_weight_grads(p, 1)[0]] == [tuple(t.shape) for t in w5]
    for bad in ([z(8, 3, 3, 3), z(8), z(3, 8, 3, 3), z(3)],          # first conv must take (cos, sin)
                [z(8, 2, 3, 3), z(8), z(3, 7, 3, 3), z(3)],          # channel chain broken
                [z(8, 2, 3, 3), z(8), z(3, 8, 5, 5), z(3)],          # one kernel size
                [z(8, 2, 4, 4), z(8), z(3, 8, 4, 4), z(3)],          # odd kernels only
                [z(8, 2, 3, 3), z(8), z(1, 8, 3, 3), z(1)]):         # needs n_mix + 1 >= 2 outputs
        with pytest.raises(FthmcError, match='unsupported s/t net'):
            ops.pack_weights([bad])
    with pytest.raises(FthmcError, match='share the net shape'):
        ops.pack_weights([w, w3])
    header = open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
    assert 'fthmc_arch_t' in header and 'fthmc_set_arch' not in header and 'FTHMC_ERR_UNSUPPORTED' in header
    # no mutable global in the kernel sources but the debug switches (variant, small path, leapfrog rows)
    import glob
    for f in glob.glob(os.path.join(ROOT, 'fthmc_amd', 'csrc', '*.hip')):
        src = open(f).read()
        assert 'g_arch' not in src and 'g_wcan' not in src, f


def _device_code_objects(path, tmp):
    """gfx950 code objects embedded in a host object / shared library (one clang offload bundle per translation unit)."""
    import subprocess
    llvm = '/opt/rocm/lib/llvm/bin'
    fat = os.path.join(tmp, 'fat.bin')
    subprocess.run(['objcopy', '-O', 'binary', '--only-section=.hip_fatbin', path, fat], check=True)
    blob = open(fat, 'rb').read()
    magic = b'__CLANG_OFFLOAD_BUNDLE__'
    starts = [i for i in range(len(blob)) if blob.startswith(magic, i)]
    outs = []
    for k, a in enumerate(starts):
        part = os.path.join(tmp, f'bundle{k}.bin')
        open(part, 'wb').write(blob[a:starts[k + 1] if k + 1 < len(starts) else len(blob)])
        dev = os.path.join(tmp, f'dev{k}.o')
        subprocess.run([f'{llvm}/clang-offload-bundler', '--unbundle', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950',
                        f'--input={part}', f'--output={dev}'], check=True, capture_output=True)
        if os.path.getsize(dev):
            outs.append(dev)
    return outs


def test_hot_kernels_are_what_the_build_intends(tmp_path):
    """Static check of the shipped library's gfx950 code (no GPU needed): the three coupling-layer kernels run on
    v_mfma_f64_16x16x4_f64, feed it with ds_read_b64 (the Makefile switches the ds_read2_b64 pairing off: half the LDS
    bandwidth) and use no scratch memory (no register spills); the forward and the backward are built for kernel-argument
    preload (round 5: their first loads do not wait for a scalar fetch of the argument segment)."""
    import re
    import subprocess
    from fthmc_amd import _lib
    llvm = '/opt/rocm/lib/llvm/bin'
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(f'{llvm}/llvm-objdump') and shutil.which('objcopy')):
        pytest.skip('library or LLVM tools not present')
    seen = {}
    for dev in _device_code_objects(_lib.LIB_PATH, str(tmp_path)):
        dis = subprocess.run([f'{llvm}/llvm-objdump', '-d', dev], check=True, capture_output=True, text=True).stdout
        notes = subprocess.run([f'{llvm}/llvm-readelf', '--notes', dev], check=True, capture_output=True, text=True).stdout
        for name, body in re.findall(r'<(_Z\w+)>:\n(.*?)(?=\n\n|\Z)', dis, flags=re.S):
            for key in ('k_flow_fwd', 'k_flow_bwd_gather', 'k_flow_wgrad'):
                if key in name:
                    m = re.search(r'\.name:\s+' + re.escape(name) + r'\s.*?\.private_segment_fixed_size:\s+(\d+)', notes, flags=re.S)
                    # a kernel built for kernel-argument preload starts with the fall-back prologue for firmware without it: scalar
                    # loads of the preloaded arguments, one wait, a branch over the padding to the real entry 256 bytes in
                    head = body.split('\n')[:8]
                    preload = any('s_branch' in l for l in head) and sum('s_load_dword' in l for l in head) >= 2
                    seen.setdefault(key, []).append((body.count('v_mfma_f64_16x16x4'), body.count('ds_read2_b64'),
                                                     body.count('ds_read_b64'), int(m.group(1)) if m else -1, preload))
    assert set(seen) == {'k_flow_fwd', 'k_flow_bwd_gather', 'k_flow_wgrad'}, seen.keys()
    # round 5: no FLAT memory instruction in the coupling kernels, and at most the two kernel-entry ones in the small-lattice
    # kernel (its pointers pass through SGPR-pinning asm statements and used to come out generic: 91 flat loads / stores that
    # count on lgkmcnt as well, so that every LDS wait also waited for the stash stores in flight); its spilled SGPRs stay below
    # what MachineLICM's hoisted fp64 constants used to cost (171 with the pass, 71 without: csrc/Makefile NOLICM)
    n_small = 0
    for dev in _device_code_objects(_lib.LIB_PATH, str(tmp_path)):
        dis = subprocess.run([f'{llvm}/llvm-objdump', '-d', dev], check=True, capture_output=True, text=True).stdout
        notes = subprocess.run([f'{llvm}/llvm-readelf', '--notes', dev], check=True, capture_output=True, text=True).stdout
        for name, body in re.findall(r'<(_Z\w+)>:\n(.*?)(?=\n\n|\Z)', dis, flags=re.S):
            flat = len(re.findall(r'\bflat_(?:load|store)_', body))
            if 'k_flow_fwd' in name or 'k_flow_bwd_gather' in name or 'k_flow_wgrad' in name:
                assert flat == 0, f'{name}: {flat} FLAT memory instructions'
            if 'k_ft_small' in name:
                n_small += 1
                assert flat <= 4, f'{name}: {flat} FLAT memory instructions (global pointers lost their address space?)'
                m = re.search(r'\.name:\s+' + re.escape(name) + r'\s.*?\.sgpr_spill_count:\s+(\d+)', notes, flags=re.S)
                assert m and int(m.group(1)) <= 120, f'{name}: {m and m.group(1)} spilled SGPRs (NOLICM of csrc/Makefile not applied?)'
    assert n_small >= 12, n_small
    for key, variants in seen.items():
        for mfma, read2, read1, scratch, preload in variants:
            # the two coupling kernels take their hot arguments as explicit scalars delivered with the wave (csrc/Makefile PRELOAD)
            assert preload == (key in ('k_flow_fwd', 'k_flow_bwd_gather')), f'{key}: kernel-argument preload prologue {preload}'
            assert mfma > 0 and read1 > 0, (key, mfma, read1)
            # the one paired read the ISel itself forms is conv2's bias pair (the accumulator's start value, once per tile);
            # with the pairing passes on there are dozens, in the MFMA operand streams
            assert read2 <= 1, f'{key}: {read2} ds_read2_b64 (LDSFLAGS of csrc/Makefile not applied?)'
            assert scratch == 0, f'{key}: {scratch} bytes of scratch per lane (spills)'


def test_lazy_history_behaves_like_the_plain_dict_it_stands_for():
    """FieldTransformation.run's captured loop hands out its history as a dict that is filled from the device when somebody looks
    (ft_hmc.py:272-346 returns a plain dict): EVERY way of reading, copying or changing a dict must see the filled one."""
    import copy
    import pickle
    from fthmc_amd.ft_hmc import LazyHistory
    full = {'acc': [1, 2], 'dh': [3]}
    calls = []

    def mk():
        def fill():
            calls.append(1)
            return {k: list(v) for k, v in full.items()}
        return LazyHistory(fill)
    assert mk().pop('acc') == [1, 2] and mk().popitem() == ('dh', [3]) and mk().copy() == full and dict(mk()) == full
    assert (mk() | {'c': 1}) == {**full, 'c': 1} and ({'c': 1} | mk()) == {'c': 1, **full}
    h = mk(); h['z'] = 5; assert h == {**full, 'z': 5}
    h = mk(); h.update(q=1); assert len(h) == 3 and h['acc'] == [1, 2]
    h = mk(); del h['acc']; assert list(h) == ['dh']
    h = mk(); h |= {'k': 2}; assert h['k'] == 2 and h['acc'] == [1, 2]
    assert bool(mk()) and 'dh' in mk() and mk().get('nope', 7) == 7 and sorted(mk().keys()) == ['acc', 'dh']
    assert pickle.loads(pickle.dumps(mk())) == full and copy.deepcopy(mk()) == full and type(copy.copy(mk())) is dict
    n = len(calls); h = mk(); _ = h['acc'], h['dh'], len(h), list(h.items()); assert len(calls) == n + 1      # filled once


def test_nothing_that_travels_to_a_gpu_box_asks_for_a_sanitizer():
    """The GPU pool refuses snapshots whose build files carry sanitizer flags (GPU sanitizers / XNACK are off there): the host-side
    sanitizer recipe lives in csrc/san.mk, which -- with the libraries it builds -- is listed in .gpurunignore."""
    ignore = open(os.path.join(ROOT, '.gpurunignore')).read().split()
    for f in ('fthmc_amd/csrc/san.mk', 'fthmc_amd/libfthmc_hip_san.so', 'fthmc_amd/libfthmc_torch_san.so'):
        assert f in ignore, f
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'fthmc_amd')):
        for name in files:
            rel = os.path.relpath(os.path.join(dirpath, name), ROOT)
            if rel in ignore or name.endswith(('.so', '.o', '.pyc')):
                continue
            text = open(os.path.join(dirpath, name), errors='ignore').read()
            assert '-fsanitize' not in text and 'xnack+' not in text and 'HSA_XNACK' not in text, rel
