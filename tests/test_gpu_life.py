"""GPU parity tests of cd_life_kernel (csrc/cd_life.hip, round 5) -- improve_coord_descent (qcqp.py:181-192: phase 1 qcqp.py:101-149,
gate :189, phase 2 :152-178) for a queue of restarts inside ONE persistent launch, for every problem class the kernel takes:
the Boolean family at any n (also n not a multiple of 16), box / disc families (one interval per coordinate), MAXCUT (zero
diagonal: the scalar objective is linear) up to BASELINE.json configs[2]'s n = 2000.  Every case goes against
  * the ORACLE (oracle/: the C restatement of the reference, keyed Philox stream), >= 8 trajectories per family, 16 at the headline size,
  * the serial path (qcqpmi_pop_randn + qcqpmi_cd_run per population: other kernels, same draws),
  * where it applies, the round-4 lifecycle kernel (cd_phase2_qs_kernel<lifecycle>).
Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

from conftest import oracle_map

pytestmark = pytest.mark.gpu

COUNTERS = ('sweeps1', 'sweeps2', 'visits2', 'accepted2', 'ran_phase2', 'status1', 'status2')


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def make(eng_mod, funcs):
    from qcqp_amd.form import QCQPForm
    return eng_mod.Engine(QCQPForm.from_arrays(funcs))


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b)) / (1.0 + np.abs(np.asarray(b))))


def family(name, n):
    from qcqp_amd import problems
    if name == 'bls':
        return problems.boolean_least_squares(n, max(4, n // 4), seed=1)[0]
    if name == 'box':
        return problems.box_least_squares(n, max(4, n // 2), bound=1.0, seed=1)[0]
    if name == 'disc':          # x_i^2 <= 0.49 around an objective whose unconstrained minimiser lies outside: active bounds
        return problems.box_least_squares(n, max(4, n // 3), bound=0.7, seed=5)[0]
    if name == 'maxcutw':       # weighted edges: no exact ties between cuts (see test_maxcut_unweighted_* for the tied case)
        return problems.maxcut(n, 0.5, seed=1, weighted=True)[0]
    raise KeyError(name)


def oracle_restarts(orc, funcs, eng_mod, seed, first, R, picks, iters):
    """improve_coord_descent of the oracle on the keyed normals of restarts `picks` of the population (seed, first)."""
    e = make(eng_mod, funcs)
    e.randn(R, seed=seed, first_index=first)
    X0 = e.download()
    prob = orc.Problem(funcs)

    def run(r):
        rng = orc.Rng(orc.RNG_KEYED, seed)
        rng.set_restart(first + r)
        x, s1, s2 = prob.improve_cd(X0[:, r], num_iters=iters, rng=rng)
        return r, x, s1, s2, prob.eval(0, x), prob.max_violation(x)
    return oracle_map(run, picks)


CASES = [
    # family, n, R, K, num_iters, oracle restarts per population, kernel name
    ('bls', 128, 100, 3, 1000, 8, 'cd_life_kernel<3,band>'),
    ('bls', 1000, 200, 2, 3, 4, 'cd_life_kernel<3,band>'),             # n not a multiple of 16; 8 oracle trajectories of three sweeps + the frozen one
                                                                       # (to convergence at this size: the factored case bls-1000-r250 below, ~35 s of oracle per trajectory)
    ('bls', 1024, 4096, 2, 4, 4, 'cd_life_kernel<3,band>'),            # BASELINE.json configs[1]'s size: 8 oracle trajectories of four sweeps (to convergence:
                                                                       # test_gpu_stream.py's 1024 case with this kernel, bls-1024-r256 below with the factored one)
    ('bls', 50, 40, 2, 1000, 8, 'cd_life_kernel<3,band>'),             # NB = 4: no chain share
    ('bls', 1040, 32, 1, 3, 8, 'cd_life_kernel<7,band>'),              # just past 1024: eight waves, seven multiplying (three sweeps:
                                                                        # the serial path's kernel for n > 1024 takes minutes to converge)
    ('box', 128, 100, 2, 1000, 8, 'cd_life_kernel<3,gen>'),
    ('box', 1000, 128, 2, 4, 4, 'cd_life_kernel<3,gen>'),             # (the box family takes ~170 sweeps: four of them here, then the frozen sweep)
    ('disc', 200, 64, 2, 1000, 8, 'cd_life_kernel<3,gen>'),
    ('maxcutw', 200, 64, 2, 1000, 8, 'cd_life_kernel<3,lin>'),
    ('maxcutw', 2000, 64, 1, 1, 8, 'cd_life_kernel<7,lin>'),           # configs[2]'s size; ONE sweep (17 s of oracle per sweep and trajectory): the frozen
                                                                        # sweeps before and after it evaluate the objective
]


@pytest.mark.parametrize('fam,n,R,K,iters,norc,kname', CASES)
def test_life_kernel_vs_oracle_and_serial(eng_mod, orc, fam, n, R, K, iters, norc, kname):
    """Every restart of the launch is the restart the reference computes: `norc` restarts per population through the oracle
    (points 1e-9, every counter, objective and max violation against the oracle's evaluation of its own point), ALL restarts
    against the serial path (points 1e-12: the same arithmetic per column in another kernel), the reported objective / max
    violation against a fresh evaluation of the returned points, the per-population winner against select_best."""
    funcs = family(fam, n)
    es = make(eng_mod, funcs)
    seed0, sstride, first0, fstride = 500, 3, 11, 70000
    o = es.cd_stream_run(K, R, num_iters=iters, seed=seed0, seed_stride=sstride, first_index=first0, first_stride=fstride)
    assert es.last_cd_kernel() == kname
    assert es.pop_size == K * R
    X = es.download()
    f0e, mve = es.eval()
    assert rel(o['f0'], f0e) < 1e-11 and np.max(np.abs(o['maxviol'] - mve)) < 1e-12
    e = make(eng_mod, funcs)
    for p in range(K):
        sd, fi = seed0 + p * sstride, first0 + p * fstride
        sl = slice(p * R, (p + 1) * R)
        # ---- the oracle
        picks = sorted(set(np.linspace(0, R - 1, norc).astype(int).tolist()))
        for r, x, s1, s2, f_or, v_or in oracle_restarts(orc, funcs, eng_mod, sd, fi, R, picks, iters):
            k = p * R + r
            assert rel(X[:, k], x) < 1e-9, (fam, n, p, r, np.max(np.abs(X[:, k] - x)))
            # (a restart that phase 1 cannot improve any further stops after its first sweep without an update; the reference burns
            #  all num_iters sweeps on the same point: documented deviation 4)
            assert o['sweeps1'][k] == s1[0] or (s1[0] == iters and not o['ran_phase2'][k])
            assert o['visits2'][k] == s2[1] and o['accepted2'][k] == s2[2], (fam, n, p, r)
            assert abs(o['f0'][k] - f_or) <= 1e-9 * (1 + abs(f_or)) and abs(o['maxviol'][k] - v_or) <= 1e-12
        # ---- the serial path
        e.randn(R, seed=sd, first_index=fi)
        outr = e.cd_run(phase1=True, num_iters=iters, seed=sd, first_index=fi)
        Xr = e.download()
        assert rel(X[:, sl], Xr) < 1e-12, (fam, n, p, np.max(np.abs(X[:, sl] - Xr)))
        for key in COUNTERS:
            assert np.array_equal(o[key][sl], outr[key]), (fam, n, p, key)
        assert rel(o['f0'][sl], outr['f0']) < 1e-11
        idx, fb, vb, xb = e.select_best(1e-4)
        assert o['best_index'][p] == idx and o['best_f0'][p] == o['f0'][sl][idx] and o['best_maxviol'][p] == o['maxviol'][sl][idx]
        assert np.array_equal(o['best_x'][p], X[:, p * R + idx])


def test_life_kernel_equals_round4_lifecycle_kernel(eng_mod):
    """Where both apply (Boolean family, n a multiple of 16, n <= 1024) the two lifecycle kernels produce the same restarts:
    points to rounding of nothing, all counters equal -- four waves and a global tile against eight waves and an LDS tile."""
    from qcqp_amd import problems
    for n, R, K in ((256, 600, 3), (1024, 1024, 2)):
        funcs, _, _ = problems.boolean_least_squares(n, n // 4, seed=2)
        e2, e1 = make(eng_mod, funcs), make(eng_mod, funcs)
        e2.cd_life_version(2)
        e1.cd_life_version(1)
        o2 = e2.cd_stream_run(K, R, seed=9, seed_stride=2, first_index=100, first_stride=5000)
        o1 = e1.cd_stream_run(K, R, seed=9, seed_stride=2, first_index=100, first_stride=5000)
        assert e2.last_cd_kernel() == 'cd_life_kernel<3,band>' and e1.last_cd_kernel() == 'cd_phase2_qs_kernel<lifecycle>'
        assert np.max(np.abs(e2.download() - e1.download())) < 1e-12
        for key in COUNTERS:
            assert np.array_equal(o2[key], o1[key]), key
        assert rel(o2['f0'], o1['f0']) < 1e-11 and np.array_equal(o2['best_index'], o1['best_index'])


def test_life_kernel_scheduling_invariance(eng_mod):
    """A restart's result does not depend on the slot, the workgroup, the episode boundaries or the number of populations in the
    launch: the same 96 restarts as one population, as three populations of 32 and with the launch confined to 3 workgroups are
    bit-identical (every product is summed in one association wherever an episode begins)."""
    from qcqp_amd import problems
    funcs = family('box', 176)
    ref = None
    for K, R, dbg in ((1, 96, 0), (3, 32, 0), (1, 96, 1024 | (3 << 12))):
        e = make(eng_mod, funcs)
        if dbg:
            e.L.qcqpmi_debug_profile(e.h, dbg << 4, None)
        o = e.cd_stream_run(K, R, num_iters=400, seed=77, seed_stride=0, first_index=5, first_stride=R)
        got = (e.download(), o['f0'].copy(), o['visits2'].copy(), o['accepted2'].copy())
        if ref is None:
            ref = got
        else:
            for a, b in zip(ref, got):
                assert np.array_equal(a, b)


def test_life_kernel_uploaded_starts_and_gate(eng_mod, orc):
    """generate = 0: improve() on resident points (the reference's improve after the user set the variables), with and without
    phase 1; restarts that do not pass the gate (qcqp.py:189) keep their point and report its objective (one frozen sweep)."""
    funcs = family('box', 100)
    n, R = 100, 48
    rs = np.random.RandomState(4)
    X0 = rs.randn(n, R) * 1.5
    X0[:, ::3] = np.clip(X0[:, ::3], -0.99, 0.99)          # a third of the starts is feasible already
    prob = orc.Problem(funcs)
    for phase1 in (True, False):
        e = make(eng_mod, funcs)
        e.upload(X0)
        o = e.cd_stream_run(1, R, generate=False, phase1=phase1, num_iters=500, seed=3, first_index=40)
        assert e.last_cd_kernel() == 'cd_life_kernel<3,gen>'
        X = e.download()
        ran = o['ran_phase2'].astype(bool)
        assert ran.any() and (phase1 or (~ran).any())
        for r in range(0, R, 5):
            rng = orc.Rng(orc.RNG_KEYED, 3)
            rng.set_restart(40 + r)
            x, s1, s2 = prob.improve_cd(X0[:, r], num_iters=500, phase1=phase1, rng=rng)
            assert rel(X[:, r], x) < 1e-9, (phase1, r)
            assert abs(o['f0'][r] - prob.eval(0, x)) <= 1e-9 * (1 + abs(prob.eval(0, x)))
        if not phase1:
            assert np.array_equal(X[:, ~ran], X0[:, ~ran])


def test_maxcut_unweighted_ties_are_the_references(eng_mod, orc):
    """Unweighted MAXCUT (examples/maxcut.py: W in {0, 1}) is full of EXACT ties: once every |x_j| sits at the same end point, a
    vertex with as many neighbours on either side has t1 = 0 up to the rounding of the row sum -- and the reference's onevar_qcqp
    then either draws a uniform point (t1 == 0 exactly, utilities.py:266-267) or picks one of four end points at random (t1 = +-1e-16,
    utilities.py:275-288): WHICH depends on the summation order of the row, i.e. on the BLAS / CSR layout.  No arithmetic other
    than SciPy's can follow such a restart (the weighted family above is followed to 1e-9).  What is asserted instead: restarts
    whose oracle trajectory never met a tie are reproduced exactly; all restarts end feasible with the objective a fresh
    evaluation of the returned point; the population's cut values have the oracle's distribution."""
    from qcqp_amd import problems
    n, R = 200, 96
    funcs, _, _ = problems.maxcut(n, 0.5, seed=1)
    e = make(eng_mod, funcs)
    o = e.cd_stream_run(1, R, num_iters=300, seed=21, first_index=0)
    assert e.last_cd_kernel() == 'cd_life_kernel<3,lin>'
    X = e.download()
    f0e, mve = e.eval()
    ran = o['ran_phase2'].astype(bool)
    assert rel(o['f0'], f0e) < 1e-11 and ran.sum() >= R - 2 and np.all(o['maxviol'][ran] <= 1e-2)
    res = oracle_restarts(orc, funcs, eng_mod, 21, 0, R, list(range(R)), 300)
    f_or = np.array([t[4] for t in res])
    same = np.array([rel(X[:, r], x) < 1e-9 for r, x, *_ in res])
    print('unweighted MAXCUT n = %d: %d of %d restarts identical to the oracle; median cut value engine %.1f / oracle %.1f'
          % (n, int(same.sum()), R, -np.median(o['f0']), -np.median(f_or)))
    assert same.sum() >= R // 8
    # same distribution of local optima: medians within 1 % of the spread-normalised cut value, best within 1 %
    assert abs(np.median(o['f0']) - np.median(f_or)) < 0.01 * abs(np.median(f_or))
    assert abs(o['f0'].min() - f_or.min()) < 0.01 * abs(f_or.min())


def test_stream_run_refusal_leaves_population(eng_mod):
    """A problem the lifecycle kernel does not take (six constraint classes: since round 6 it takes up to four) is refused BEFORE the
    resident population is touched: the points uploaded before the call are still there and still evaluate."""
    from qcqp_amd import problems
    funcs, _, _ = problems.boolean_least_squares(64, 16, seed=1)
    funcs = [funcs[0]] + [(P * (1.0 + (i % 6)), q, r * (1.0 + (i % 6)), rel_) for i, (P, q, r, rel_) in enumerate(funcs[1:])]
    e = make(eng_mod, funcs)
    X0 = np.random.RandomState(0).randn(64, 24)
    e.upload(X0)
    with pytest.raises(eng_mod.EngineError) as ei:
        e.cd_stream_run(2, 50, seed=1)
    assert ei.value.code == eng_mod.E_UNSUPPORTED
    assert e.pop_size == 24 and np.array_equal(e.download(), X0)
    f0, mv = e.eval()
    assert np.all(np.isfinite(f0))


def test_comm_allgather_over_rccl_one_rank(eng_mod):
    """qcqpmi_comm_allgather (round 5: the 32-byte keys of a streamed run's exchange travel through ONE ncclAllGather, integers as
    integers) on the library's communicator: with one rank the gathered table is the contribution itself, for byte counts that
    are not multiples of 8 and for int64 fields beyond 2^53."""
    from qcqp_amd import dist, problems
    funcs, _, _ = problems.boolean_least_squares(64, 16, seed=7)
    e = make(eng_mod, funcs)
    dist.init_rccl(e, 0, 1)
    rec = np.array([[3, np.float64(1.25).view(np.int64), (1 << 62) + 12345, -7]] * 5, dtype=np.int64)
    out = e.comm_allgather(rec)
    assert out.shape == (1, 5, 4) and out.dtype == np.int64 and np.array_equal(out[0], rec)
    odd = np.arange(13, dtype=np.uint8)
    assert np.array_equal(e.comm_allgather(odd)[0], odd)
    o = e.cd_stream_run(4, 40, seed=3, seed_stride=1)
    ks, X = dist.global_best_of_populations(lambda a: e.comm_allreduce(a, 'sum'), 0, 1, o['best_f0'], o['best_maxviol'], o['best_index'],
                                            o['best_x'], allgather=e.comm_allgather)
    assert [k[0] for k in ks] == list(o['best_index']) and np.array_equal(X, o['best_x'])


@pytest.mark.parametrize('launch', ['torch_distributed_run', 'visible_devices'])
def test_bench_under_the_drivers_launcher_on_one_gpu(tmp_path, launch):
    """bench.py the way the driver starts it for N > 1 -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr
    127.0.0.1 --master-port P bench.py --gpus N ...` -- with the one GPU this box has (N = 1): RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* come from the launcher, the RCCL communicator is created on the real device, comm_barrier and the max / sum
    all-reduces of the timing run through RCCL, one JSON line comes out.  And under HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES
    = 0, the isolation a launcher may set per rank: Engine(device=LOCAL_RANK) must still find its device."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # (no --n / --m-rows here: torch.distributed.run's own parser rejects `--n` as an ambiguous abbreviation of its options)
    args = ['bench.py', '--gpus', '1', '--steps', '2', '--warmup', '1', '--restarts', '256', '--no-secondary', '--no-cpu-baseline']
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'QCQP_AMD_RDZV')}
    if launch == 'torch_distributed_run' and os.environ.get('QCQP_TEST_TORCHRUN') == '1':
        # the real launcher: its `import torch` alone takes 1-2 minutes on a fresh box (95 s of round 5's 928 s GPU suite), so it is
        # opt-in; the default below gives bench.py exactly the environment the launcher gives it
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr', '127.0.0.1',
               '--master-port', str(29400 + os.getpid() % 500)] + args
    elif launch == 'torch_distributed_run':
        port = str(29400 + os.getpid() % 500)
        cmd = [sys.executable] + args
        env.update(RANK='0', LOCAL_RANK='0', WORLD_SIZE='1', LOCAL_WORLD_SIZE='1', GROUP_RANK='0', ROLE_RANK='0', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=port, TORCHELASTIC_RUN_ID='none', TORCHELASTIC_RESTART_COUNT='0', TORCHELASTIC_MAX_RESTARTS='0', OMP_NUM_THREADS='1')
    else:
        cmd = [sys.executable] + args
        env.update(HIP_VISIBLE_DEVICES='0', ROCR_VISIBLE_DEVICES='0')
    pr = subprocess.run(cmd, cwd=repo, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert pr.returncode == 0, pr.stderr.decode()[-3000:]
    lines = [l for l in pr.stdout.decode().splitlines() if l.startswith('{')]
    assert len(lines) == 1, pr.stdout.decode()[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 1 and d['steps'] == 2 and d['config']['scheme'] == 'stream' and d['value'] > 0
    assert d['roofline']['kernel'].startswith('cd_life_kernel')


def test_two_real_engines_two_processes_share_one_gpu(tmp_path):
    """SURVEY.md section 8e with what a one-GPU box can offer (no multi-GPU node exists for the builder or the driver): `bench.py
    --gpus 2 --scaling strong` -- rank 0 plus the rank 1 it spawns itself, TWO real engines in two processes, both on device 0,
    the exchange of the streamed run (all-gather of the 32-byte keys, all-reduce of the winners' points, the max / sum reductions
    of the timing) over the job's file rendezvous (RCCL refuses a communicator whose ranks share a device; its one-rank path has
    its own tests) -- against `--gpus 1` on the same 8192 GLOBAL restart indices per step: the global best of every step is the
    same restart, objective and point bit for bit, each rank ran only its shard (4096 restarts per step), and the shards together
    did exactly the sweeps of the whole (the same restarts, wherever they ran)."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'QCQP_AMD_RDZV')}
    out = {}
    for gpus in (1, 2):
        best = str(tmp_path / ('best%d.npy' % gpus))
        cmd = [sys.executable, 'bench.py', '--gpus', str(gpus), '--scaling', 'strong', '--restarts', '8192', '--steps', '2', '--warmup', '1',
               '--n', '512', '--m-rows', '128', '--comm', 'file', '--device', '0', '--no-cpu-baseline', '--best-out', best]
        pr = subprocess.run(cmd, cwd=repo, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert pr.returncode == 0, pr.stderr.decode()[-3000:]
        lines = [l for l in pr.stdout.decode().splitlines() if l.startswith('{')]
        assert len(lines) == 1, pr.stdout.decode()[-2000:]
        out[gpus] = (json.loads(lines[0]), np.load(best))
    (d1, x1), (d2, x2) = out[1], out[2]
    assert d1['n_gpus'] == 1 and d2['n_gpus'] == 2 and d1['scaling'] == d2['scaling'] == 'strong'
    assert d1['config']['restarts_per_gpu'] == 8192 and d2['config']['restarts_per_gpu'] == 4096      # each rank: its shard only
    # (the two runs may dispatch to different lifecycle kernels -- 8192 restarts per launch against 4096 --: same restarts either way)
    for key in ('objective', 'max_violation', 'global_restart_index', 'step'):
        assert d1['best'][key] == d2['best'][key], (key, d1['best'], d2['best'])
    assert x1.shape == x2.shape == (2, 512) and np.array_equal(x1, x2)                                # every step's winner, bit for bit
    # the same restarts did the same sweeps wherever they ran: value x time = phase-2 sweeps of the job
    s1, s2 = d1['value'] * d1['timed_region_s'], d2['value'] * d2['timed_region_s']
    assert abs(s1 - s2) <= 1e-6 * s1, (s1, s2)
    assert d1['phase2_sweeps_per_restart'] == pytest.approx(d2['phase2_sweeps_per_restart'], rel=1e-12)


FACTORED = [
    # family, n, rows of A, R, K, num_iters, oracle restarts per population
    ('bls', 128, 32, 4000, 2, 1000, 4),            # 8000 restarts on 8192 slots... and back: refills, episodes that begin and end mid-run
    ('bls', 1000, 250, 150, 2, 1000, 2),           # n not a multiple of 16 (63 blocks), rank 250 (16 blocks of Y, the last one partly zero)
    ('bls', 1024, 256, 4096, 2, 1000, 2),          # BASELINE.json configs[1]
    ('box', 320, 96, 700, 2, 60, 2),               # the `gen` step kind (box |x_i| <= 1) on a rank-96 objective
    ('bls', 2320, 200, 40, 1, 2, 0),               # past 2304: ONLY the factored instantiation goes there (Y, not X, lives in registers); all restarts
                                                   # against the serial path (oracle-checked up to n = 1040; an oracle sweep costs ~40 s here: the full
                                                   # suite ran 589 s with one trajectory -- QCQP_ORACLE_2320=1 adds it back)
    ('bls', 4096, 256, 32, 2, 2, 0),               # n = 4096 (256 blocks of 16 coordinates), two populations
]


@pytest.mark.parametrize('fam,n,rows,R,K,iters,norc', FACTORED, ids=['%s-%d-r%d' % (c[0], c[1], c[2]) for c in FACTORED])
def test_factored_objective_kernel_vs_serial_oracle_and_itself(eng_mod, orc, fam, n, rows, R, K, iters, norc):
    """qcqpmi_cd_set_objective_factor (round 6): with P0 = L L^T handed over (qcqp_amd.lowrank.objective_factor finds L from P0 alone
    and verifies it entry by entry) the lifecycle kernel carries Y = L^T X per tile and never multiplies with P0.  What must hold:
      * every restart is the serial path's restart (which multiplies with P0): all counters equal, points 1e-9 (the two sum (P0 x)_i
        in different orders: measured 6e-14), objective 1e-9, the same best restart per population;
      * sampled restarts follow the ORACLE's trajectory (1e-9, every counter);
      * the reported objective and max violation are those of the final point (fresh evaluation by the evaluation kernel);
      * results do not depend on the scheduling: one population of K R restarts and K populations of R restarts with matching
        keys give the same bits, twice in a row (Y rests between episodes in exactly the state the first product of the next
        episode wants; a restart's column is loaded by the products' own updates)."""
    from qcqp_amd import lowrank, problems
    if fam == 'bls':
        funcs = problems.boolean_least_squares(n, rows, seed=1)[0]
    else:
        funcs = problems.box_least_squares(n, rows, bound=1.0, seed=1, ridge=0.0)[0]      # (no ridge: P0 = A^T A of rank rows)
    P0 = funcs[0][0]
    P0 = P0.toarray() if hasattr(P0, 'toarray') else np.asarray(P0)
    L = lowrank.objective_factor(P0, max_rank=288)
    assert L is not None and L.shape == (n, rows)
    es, e = make(eng_mod, funcs), make(eng_mod, funcs)
    es.cd_set_objective_factor(L)
    seed0, first0, fstride = 700, 3, 50000
    o = es.cd_stream_run(K, R, num_iters=iters, seed=seed0, seed_stride=1, first_index=first0, first_stride=fstride)
    assert 'factored' in es.last_cd_kernel(), es.last_cd_kernel()
    X = es.download()
    f0e, mve = es.eval()
    # (the evaluation kernel multiplies with P0, the factored kernel's window sum uses L (L^T x): 1e-13 of the objective's TERMS apart --
    #  the box family's optimum nearly cancels them, f0 ~ 1e-3 there)
    assert rel(o['f0'], f0e) < 1e-9 and np.max(np.abs(o['maxviol'] - mve)) < 1e-12
    prob = orc.Problem(funcs)
    jobs = []
    for p in range(K):
        sd, fi = seed0 + p, first0 + p * fstride
        e.randn(R, seed=sd, first_index=fi)
        X0 = e.download()
        outr = e.cd_run(phase1=True, num_iters=iters, seed=sd, first_index=fi)
        assert 'factored' not in e.last_cd_kernel()
        Xr = e.download()
        sl = slice(p * R, (p + 1) * R)
        assert rel(X[:, sl], Xr) < 1e-9, (p, np.max(np.abs(X[:, sl] - Xr)))
        for key in ('sweeps1', 'sweeps2', 'visits2', 'accepted2', 'ran_phase2', 'status1', 'status2'):
            assert np.array_equal(o[key][sl], outr[key]), (p, key)
        assert rel(o['f0'][sl], outr['f0']) < 1e-9 and np.max(np.abs(o['maxviol'][sl] - outr['maxviol'])) < 1e-9
        assert o['best_index'][p] == e.select_best(1e-4)[0]
        jobs += [(p, r, sd, fi, X0[:, r].copy()) for r in list(range(R))[:(1 if (n == 2320 and __import__('os').environ.get('QCQP_ORACLE_2320') == '1') else norc)]]

    def oracle_restart(job):
        p, r, sd, fi, x0 = job
        rng = orc.Rng(orc.RNG_KEYED, sd)
        rng.set_restart(fi + r)
        return prob.improve_cd(x0, num_iters=iters, rng=rng)
    for (p, r, sd, fi, x0), (x, s1, s2) in zip(jobs, oracle_map(oracle_restart, jobs)):
        k = p * R + r
        assert rel(X[:, k], x) < 1e-9, (p, r)
        assert o['visits2'][k] == s2[1] and o['accepted2'][k] == s2[2]
        assert abs(o['f0'][k] - prob.eval(0, x)) <= 1e-9 * (1 + abs(prob.eval(0, x)))
    # scheduling invariance, bit for bit: the same restarts as ONE population (other slots, other episode boundaries), and again
    o1 = es.cd_stream_run(1, K * R, num_iters=iters, seed=seed0, seed_stride=0, first_index=first0, first_stride=0)
    X1 = es.download()
    o2 = es.cd_stream_run(1, K * R, num_iters=iters, seed=seed0, seed_stride=0, first_index=first0, first_stride=0)
    assert np.array_equal(X1, es.download()) and np.array_equal(o1['f0'], o2['f0'])
    assert np.array_equal(X1[:, :R], X[:, :R]) and np.array_equal(o1['f0'][:R], o['f0'][:R])      # population 0 has the same keys in both runs
    # without the factor the same call runs the kernel that multiplies with P0 -- where that one exists (n <= 2304: its B operands are
    # the X tile, register-resident); beyond, the call is refused
    es.cd_set_objective_factor(None)
    if n <= 2304:
        es.cd_stream_run(K, R, num_iters=iters, seed=seed0, seed_stride=1, first_index=first0, first_stride=fstride)
        assert 'factored' not in es.last_cd_kernel()
    else:
        with pytest.raises(eng_mod.EngineError) as ei:
            es.cd_stream_run(K, R, num_iters=iters, seed=seed0, seed_stride=1, first_index=first0, first_stride=fstride)
        assert ei.value.code == eng_mod.E_UNSUPPORTED


MULTI = [
    # family, n, R, K, num_iters, oracle restarts per population, kernel name
    ('box3', 100, 70, 2, 1000, 4, 'cd_life_kernel<3,gen,classes>'),      # three classes, n not a multiple of 16
    ('box3', 256, 40, 2, 30, 4, 'cd_life_kernel<3,gen,classes>'),
    ('ann2', 96, 70, 2, 1000, 4, 'cd_life_kernel<3,gen,classes>'),       # two constraints per coordinate (two intervals) beside an equality class
    ('lin2', 130, 50, 2, 60, 4, 'cd_life_kernel<3,gen,classes>'),        # two LINEAR constraints per coordinate, bounds by class
    ('cut2', 100, 70, 2, 1000, 4, 'cd_life_kernel<3,lin,classes>'),      # zero diagonal (linear scalar objective), two classes
    ('box3', 1100, 32, 1, 3, 2, 'cd_life_kernel<7,gen,classes>'),        # past 1024: eight waves
]


@pytest.mark.parametrize('fam,n,R,K,iters,norc,kname', MULTI)
def test_life_kernel_several_classes_vs_oracle_and_serial(eng_mod, orc, fam, n, R, K, iters, norc, kname):
    """Round 6: the lifecycle launch for separable problems with SEVERAL constraint classes and up to two constraints per coordinate
    (kinds GENK / LINK: a feasible set per (class, slot), the chain looks its columns' classes up per block; qcqp.py:113-141, 160-176
    treat every coordinate's list on its own).  `norc` restarts per population through the oracle (points 1e-9, every counter,
    objective, max violation), ALL restarts against the serial path -- qcqpmi_cd_run: the general phase-2 kernel, which follows the
    reference's one-variable arithmetic visit by visit where this kernel projects the vertex (1e-9, counters equal) --, the
    reported values against a fresh evaluation, the per-population winner against select_best."""
    from qcqp_amd import problems
    funcs = problems.multi_class(fam, n)
    es = make(eng_mod, funcs)
    seed0, sstride, first0, fstride = 900, 2, 5, 30000
    o = es.cd_stream_run(K, R, num_iters=iters, seed=seed0, seed_stride=sstride, first_index=first0, first_stride=fstride)
    assert es.last_cd_kernel() == kname
    X = es.download()
    f0e, mve = es.eval()
    assert rel(o['f0'], f0e) < 1e-10 and np.max(np.abs(o['maxviol'] - mve)) < 1e-12
    e = make(eng_mod, funcs)
    for p in range(K):
        sd, fi = seed0 + p * sstride, first0 + p * fstride
        sl = slice(p * R, (p + 1) * R)
        picks = sorted(set(np.linspace(0, R - 1, norc).astype(int).tolist()))
        for r, x, s1, s2, f_or, v_or in oracle_restarts(orc, funcs, eng_mod, sd, fi, R, picks, iters):
            k = p * R + r
            assert rel(X[:, k], x) < 1e-9, (fam, n, p, r, np.max(np.abs(X[:, k] - x)))
            assert o['sweeps1'][k] == s1[0] or (s1[0] == iters and not o['ran_phase2'][k])
            assert o['visits2'][k] == s2[1] and o['accepted2'][k] == s2[2], (fam, n, p, r)
            assert abs(o['f0'][k] - f_or) <= 1e-9 * (1 + abs(f_or)) and abs(o['maxviol'][k] - v_or) <= 1e-12
        e.randn(R, seed=sd, first_index=fi)
        outr = e.cd_run(phase1=True, num_iters=iters, seed=sd, first_index=fi)
        Xr = e.download()
        assert rel(X[:, sl], Xr) < 1e-9, (fam, n, p, np.max(np.abs(X[:, sl] - Xr)))
        for key in COUNTERS:
            assert np.array_equal(o[key][sl], outr[key]), (fam, n, p, key)
        assert rel(o['f0'][sl], outr['f0']) < 1e-9
        idx = e.select_best(1e-4)[0]
        assert o['best_index'][p] == idx and np.array_equal(o['best_x'][p], X[:, p * R + idx])
    # scheduling invariance, bit for bit: the same restarts as ONE population
    o1 = es.cd_stream_run(1, R, num_iters=iters, seed=seed0, seed_stride=0, first_index=first0, first_stride=0)
    assert np.array_equal(es.download(), X[:, :R]) and np.array_equal(o1['f0'], o['f0'][:R])


def test_stream_run_refuses_what_the_kinds_do_not_cover(eng_mod):
    """More than four classes (every coordinate its own bounds) is refused with E_UNSUPPORTED, not misrouted."""
    from qcqp_amd import problems
    n = 64
    funcs = [problems.multi_class('box3', n)[0]]
    rs = np.random.RandomState(1)
    import scipy.sparse as sp
    for i in range(n):
        funcs.append((sp.csr_matrix(([1.0], ([i], [i])), shape=(n, n)), np.zeros(n), -1.0 - rs.rand(), '<='))
    e = make(eng_mod, funcs)
    with pytest.raises(eng_mod.EngineError) as ei:
        e.cd_stream_run(2, 32, seed=1)
    assert ei.value.code == eng_mod.E_UNSUPPORTED


def _fuzz_shape(rs):
    fam = str(rs.choice(['bls', 'bls', 'box', 'maxcutw']))
    n = int(rs.choice([48, 50, 64, 77, 96, 100, 128, 130, 176, 200, 256, 300, 320]))
    R = int(rs.choice([1, 2, 15, 16, 17, 100, 257, 600]))
    K = int(rs.choice([1, 2, 3, 5]))
    iters = int(rs.choice([0, 1, 2, 5, 40, 1000])) if fam != 'box' else int(rs.choice([0, 1, 3, 25]))
    return fam, n, R, K, iters, bool(rs.rand() < 0.7), bool(rs.rand() < 0.6)


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_life_kernel_fuzz_shapes(eng_mod, orc, seed):
    """Ten random shapes per seed (40 in all; tools/fuzz_stream.py promoted to a test, with the ORACLE in it): family (Boolean / box /
    weighted MAXCUT), n = 48 .. 320 incl. sizes that are not multiples of 16, 1 .. 600 restarts, 1 .. 5 populations, sweep limits
    0 .. 1000, with and without phase 1, generated and uploaded starts (a share of the uploaded ones fails the gate).  Every
    population against the serial path (points 1e-12, all counters, objective, winner), two restarts per shape against the oracle."""
    rs = np.random.RandomState(1000 + seed)
    rf = np.random.RandomState(5000 + seed)          # (its own stream: the shapes of rounds 5 stay what they were)
    for case in range(10):
        fam, n, R, K, iters, phase1, generate = _fuzz_shape(rs)
        funcs = family(fam, n)
        es, e = make(eng_mod, funcs), make(eng_mod, funcs)
        # round 6: half of the Boolean shapes run the FACTORED instantiation (P0 = A^T A = L L^T of rank n / 4; 1e-9 against the serial
        # path, which multiplies with P0 -- another summation order --, the counters still equal)
        factored = False
        if fam == 'bls' and n >= 128 and rf.rand() < 0.5:
            from qcqp_amd import lowrank
            P0 = funcs[0][0]
            Lf = lowrank.objective_factor(P0.toarray() if hasattr(P0, 'toarray') else np.asarray(P0), max_rank=288)
            assert Lf is not None and Lf.shape[1] == max(4, n // 4)
            es.cd_set_objective_factor(Lf)
            factored = True
        xtol = 1e-9 if factored else 1e-12
        seed0, sstride, first0, fstride = int(rs.randint(1 << 20)), int(rs.randint(0, 4)), int(rs.randint(100)), int(rs.choice([0, R, 100000]))
        tag = (seed, case, fam, n, R, K, iters, phase1, generate)
        X0 = None
        if generate:
            o = es.cd_stream_run(K, R, generate=True, phase1=phase1, num_iters=iters, seed=seed0, seed_stride=sstride, first_index=first0, first_stride=fstride)
        else:
            X0 = np.sign(rs.randn(n, K * R)) * (1.0 - 2e-3 * rs.rand(n, K * R))     # feasible for the box, near-feasible for x^2 == 1
            far = rs.rand(K * R) < 0.3
            X0[:, far] *= 1.0 + rs.rand(int(far.sum()))
            es.upload(X0)
            o = es.cd_stream_run(K, R, generate=False, phase1=phase1, num_iters=iters, seed=seed0, seed_stride=sstride, first_index=first0, first_stride=fstride)
        assert es.last_cd_kernel().startswith('cd_life_kernel<3,') and ('factored' in es.last_cd_kernel()) == factored, (tag, es.last_cd_kernel())
        X = es.download()
        prob = orc.Problem(funcs)
        for p in range(K):
            sd, fi = seed0 + p * sstride, first0 + p * fstride
            sl = slice(p * R, (p + 1) * R)
            if generate:
                e.randn(R, seed=sd, first_index=fi)
            else:
                e.upload(X0[:, sl])
            Xs = e.download()
            outr = e.cd_run(phase1=phase1, num_iters=iters, seed=sd, first_index=fi)
            Xr = e.download()
            assert rel(X[:, sl], Xr) < xtol, (tag, p, factored)
            for key in COUNTERS:
                assert np.array_equal(o[key][sl], outr[key]), (tag, p, key)
            assert rel(o['f0'][sl], outr['f0']) < (1e-9 if factored else 1e-10) and np.max(np.abs(o['maxviol'][sl] - outr['maxviol'])) < (1e-9 if factored else 1e-12), (tag, p)
            assert o['best_index'][p] == e.select_best(1e-4)[0], (tag, p)
            if p == 0:
                for r in sorted({0, R - 1}):
                    rng = orc.Rng(orc.RNG_KEYED, sd)
                    rng.set_restart(fi + r)
                    x, s1, s2 = prob.improve_cd(Xs[:, r], num_iters=iters, phase1=phase1, rng=rng)
                    assert rel(X[:, r], x) < 1e-9, (tag, r)
                    assert o['visits2'][r] == s2[1] and o['accepted2'][r] == s2[2], (tag, r)
        es.close()
        e.close()


@pytest.mark.parametrize('seed', list(range(int(__import__('os').environ.get('QCQP_FUZZ_SEEDS', '2')))))     # (QCQP_FUZZ_SEEDS=N: a longer shake-out)
def test_life_kernel_fuzz_several_classes(eng_mod, orc, seed):
    """Eight random shapes per seed of the multi-class kinds (problems.multi_class: three classes of boxes, an annulus class beside an
    equality class, two linear constraints per coordinate, MAXCUT with a relaxed class): n = 48 .. 300 incl. sizes that are not
    multiples of 16, 1 .. 300 restarts, 1 .. 3 populations, sweep limits 0 .. 1000, with and without phase 1, generated and uploaded
    starts.  Every population against the serial path (points 1e-9, all counters, objective, winner), two restarts per shape
    against the oracle."""
    from qcqp_amd import problems
    rs = np.random.RandomState(2000 + seed)
    for case in range(8):
        fam = str(rs.choice(['box3', 'ann2', 'lin2', 'cut2']))
        big = __import__('os').environ.get('QCQP_FUZZ_BIG') == '1'        # a shake-out of the larger instantiations (the fast separable oracle there)
        n = int(rs.choice([500, 777, 1024, 1040, 1100, 1500, 2000] if big else [48, 50, 64, 77, 100, 128, 130, 200, 256, 300]))
        R = int(rs.choice([1, 15, 16, 17, 100, 300]))
        K = int(rs.choice([1, 2, 3]))
        iters = int(rs.choice([0, 1, 2, 3])) if big else (int(rs.choice([0, 1, 2, 5, 40, 1000])) if fam in ('ann2', 'cut2') else int(rs.choice([0, 1, 3, 25])))
        phase1, generate = bool(rs.rand() < 0.7), bool(rs.rand() < 0.6)
        funcs = problems.multi_class(fam, n, seed=int(rs.randint(1, 50)))
        es, e = make(eng_mod, funcs), make(eng_mod, funcs)
        seed0, sstride, first0, fstride = int(rs.randint(1 << 20)), int(rs.randint(0, 4)), int(rs.randint(100)), int(rs.choice([0, R, 100000]))
        tag = (seed, case, fam, n, R, K, iters, phase1, generate)
        X0 = None
        if generate:
            o = es.cd_stream_run(K, R, generate=True, phase1=phase1, num_iters=iters, seed=seed0, seed_stride=sstride, first_index=first0, first_stride=fstride)
        else:
            X0 = np.sign(rs.randn(n, K * R)) * (0.6 + 0.4 * rs.rand(n, K * R))       # inside some classes' sets, outside others'
            es.upload(X0)
            o = es.cd_stream_run(K, R, generate=False, phase1=phase1, num_iters=iters, seed=seed0, seed_stride=sstride, first_index=first0, first_stride=fstride)
        assert 'classes' in es.last_cd_kernel(), tag
        X = es.download()
        prob = orc.Problem(funcs)
        for p in range(K):
            sd, fi = seed0 + p * sstride, first0 + p * fstride
            sl = slice(p * R, (p + 1) * R)
            if generate:
                e.randn(R, seed=sd, first_index=fi)
            else:
                e.upload(X0[:, sl])
            Xs = e.download()
            outr = e.cd_run(phase1=phase1, num_iters=iters, seed=sd, first_index=fi)
            Xr = e.download()
            assert rel(X[:, sl], Xr) < 1e-9, (tag, p)
            for key in COUNTERS:
                assert np.array_equal(o[key][sl], outr[key]), (tag, p, key)
            assert rel(o['f0'][sl], outr['f0']) < 1e-9 and np.max(np.abs(o['maxviol'][sl] - outr['maxviol'])) < 1e-12, (tag, p)
            assert o['best_index'][p] == e.select_best(1e-4)[0], (tag, p)
            if p == 0:
                for r in sorted({0, R - 1}):
                    rng = orc.Rng(orc.RNG_KEYED, sd)
                    rng.set_restart(fi + r)
                    x, s1, s2 = (prob.improve_cd_sep if big else prob.improve_cd)(Xs[:, r], num_iters=iters, phase1=phase1, rng=rng)
                    assert rel(X[:, r], x) < 1e-9, (tag, r)
                    assert o['visits2'][r] == s2[1] and o['accepted2'][r] == s2[2], (tag, r)
        es.close()
        e.close()


def test_lifecycle_dispatch_is_one_kernel(eng_mod):
    """Round 6: qcqpmi_cd_stream_run launches cd_life_kernel for every shape it takes (the round-5 rule that sent the Boolean family at
    n >= 960 with more than 8192 restarts to the round-4 kernel is gone); qcqpmi_cd_life_version(1) -- a debug switch -- still reaches
    the round-4 kernel, and the restarts are the same either way."""
    from qcqp_amd import problems
    funcs, _, _ = problems.boolean_least_squares(1024, 256, seed=1)
    e = make(eng_mod, funcs)
    o3 = e.cd_stream_run(3, 4096, seed=7, seed_stride=1)
    assert e.last_cd_kernel() == 'cd_life_kernel<3,band>'
    X3 = e.download()
    e.cd_life_version(1)
    o3b = e.cd_stream_run(3, 4096, seed=7, seed_stride=1)
    assert e.last_cd_kernel() == 'cd_phase2_qs_kernel<lifecycle>'
    assert np.max(np.abs(e.download() - X3)) < 1e-12 and np.array_equal(o3['visits2'], o3b['visits2']) and np.array_equal(o3['best_index'], o3b['best_index'])
    e.cd_life_version(0)
    e.cd_stream_run(1, 4096, seed=7)
    assert e.last_cd_kernel() == 'cd_life_kernel<3,band>'
    # a problem the round-4 kernel never took (n not a multiple of 16) is refused under the debug switch instead of silently rerouted
    funcs, _, _ = problems.boolean_least_squares(100, 25, seed=1)
    e = make(eng_mod, funcs)
    e.cd_stream_run(2, 64, seed=7, seed_stride=1)
    assert e.last_cd_kernel() == 'cd_life_kernel<3,band>'
    e.cd_life_version(1)
    with pytest.raises(eng_mod.EngineError):
        e.cd_stream_run(2, 64, seed=7, seed_stride=1)
