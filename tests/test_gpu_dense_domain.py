"""The coupled-constraint (dense) coordinate-descent path over its dispatch domain: MFMA block products followed by
dense_chain_mw_kernel (csrc/cd_dense_mw.h) or dense_chain_kernel (csrc/cd_dense.h), against the oracle.

A  dense_chain_mw_kernel at every slot count, template instantiation and placement of the serial thread of mw_geometry,
   teacher-forced along the oracle's trajectories, '==' among the coupled constraints;
B  dense_chain_kernel against dense_chain_mw_kernel bit for bit up to m = 3584 (with and without G staged in LDS, at and
   beyond 32 function slots per lane);
C  dense_chain_kernel beyond eight slots (m = 3585 .. 5055, up to 79 slots per lane) against the oracle, block by block;
D  the gap list (64) and the segment list (32) at and beyond capacity, the LDS refusal;
E  the full driver: status words, tracked values against fresh evaluations, both chain kernels, forced K-splits.

Cases, families, the walker and its yardstick: tests/dense_domain_cases.py (checked on the host by
tests/test_dense_domain_cpu.py).  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

import dense_domain_cases as dc

pytestmark = pytest.mark.gpu

MW, ONE = 'dense_chain_mw_kernel', 'dense_chain_kernel'
KEYS = ('f0', 'maxviol', 'sweeps1', 'sweeps2', 'visits2', 'accepted2', 'ran_phase2', 'status1', 'status2')


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def make(eng_mod, funcs, forced=True, mode=0):
    from qcqp_amd.form import QCQPForm
    e = eng_mod.Engine(QCQPForm.from_arrays(funcs))
    if forced:
        e.L.qcqpmi_debug_profile(e.h, dc.DENSE_PATH, None)      # the dense path also for n <= 64
    e.dense_chain_mode(mode)
    return e


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b)) / (1.0 + np.abs(np.asarray(b))))


def walk_and_judge(e, orc, case, kernel, widths, blocks, label, strict_first=False):
    """Both phases, every width: no visit of the walked blocks is left out; the figures are printed before anything about
    them is asserted."""
    moved, total = dc.moved_visits(case, blocks)
    assert 4 * moved >= total, (moved, total)              # not a walk over fixed points
    slack_all = None
    if len(case.restarts) < case.R:                        # restarts nobody compares: the slack of their own start
        slack_all = e.eval_batch(case.X[2])[1]
    nvis = sum(min(16, case.n - 16 * b) for b in blocks)
    for phase in (1, 2):
        for width in widths:
            steps = dc.walk(e, case, phase, width, blocks, slack_all)
            assert e.last_cd_kernel() == kernel
            assert sum(len(s.dev) for s in steps) == nvis * len(case.restarts)
            devs = np.concatenate([s.dev for s in steps])
            firsts = np.array([s.dev[0] for s in steps])
            print('\n%s phase %d, steps of %d: %d visits (%d of %d moved over both phases), max deviation %.2e (first visit of a step '
                  '%.2e), median %.1e, beyond 1e-8: %d, beyond 1e-6: %d' % (label, phase, width, len(devs), moved, total, devs.max(),
                                                                             firsts.max(), np.median(devs), int((devs > 1e-8).sum()),
                                                                             int((devs > 1e-6).sum())))
            worst, worst_first, judged = dc.judge(orc, case, steps, width, strict_first)
            if judged:
                print('%s phase %d, steps of %d: %d steps within 10 x the oracle\'s own deviation + 1e-6' % (label, phase, width, judged))


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize('m', dc.A_GRID)
def test_multi_wave_kernel_follows_the_oracle(eng_mod, orc, m):
    """dense_chain_mw_kernel at n = 40 through the forced dense path, R = 8, phase 1 from random points and phase 2 from points
    that satisfy the '<=' constraints (slack = the violation of the equalities): blocks 0 and 2 (the ragged one) of the
    oracle's first sweep, visit by visit and block by block.  Every visit within 1e-8 of the oracle (relative to 1 + max|x|),
    every block within 1e-6 -- or within 10 x the oracle's own deviation under 1, 32 and 1024 ulps + 1e-6.
    Measured on the MI355X, visit by visit: at most 6.3e-12 over the whole grid; seven blocks of phase 1 beyond 1e-6 (up to 2.4e-5),
    all within the yardstick (profiles/r13_dense_domain.md)."""
    case = dc.walk_case(orc, m)
    e = make(eng_mod, case.funcs)
    assert dc.geometry(e.L, m) == dc.GEOMETRY[m]
    walk_and_judge(e, orc, case, MW, (1, 16), (0, 2), 'A m=%d %s' % (m, dc.GEOMETRY[m]))


def test_multi_wave_kernel_follows_the_oracle_with_forty_restarts(eng_mod, orc):
    """m = 600 with 40 restarts (three tiles, another K-split of the products): restarts 15, 16, 17 (the tile boundary) and 39
    against the oracle."""
    m, R, restarts = dc.A_EXTRA
    case = dc.walk_case(orc, m, R=R, restarts=restarts)
    e = make(eng_mod, case.funcs)
    walk_and_judge(e, orc, case, MW, (1, 16), (0, 2), 'A m=%d R=%d' % (m, R))


# ------------------------------------------------------------------------------------------------ B
def both_phases(e, X1, X2, vt2, iters, kernel):
    """Phase 1 from X1 (the equalities keep the gate shut for most restarts), then phase 2 alone from X2 with the gate opened
    to the violation of the starts: (points, outputs) of each run."""
    runs = []
    for X0, p1, vt in ((X1, True, 1e-2), (X2, False, vt2)):
        e.upload(X0)
        out = e.cd_run(phase1=p1, num_iters=iters, viol_tol=vt, seed=dc.SEED, first_index=dc.FIRST)
        assert e.last_cd_kernel() == kernel
        runs.append((e.download(), out, vt))
    return runs


def assert_identical(runs0, runs1):
    for (Xa, oa, _), (Xb, ob, _) in zip(runs0, runs1):
        assert np.array_equal(Xa, Xb)
        for key in KEYS:
            assert np.array_equal(oa[key], ob[key]), key
        assert not oa['status1'].any() and not oa['status2'].any()
    assert runs0[0][1]['sweeps1'].sum() > 0
    assert runs0[1][1]['ran_phase2'].all() and runs0[1][1]['accepted2'].sum() > 0


@pytest.mark.parametrize('m,n,R', dc.B_CASES)
def test_one_wave_kernel_agrees_with_multi_wave_bit_for_bit(eng_mod, orc, m, n, R):
    """dense_chain_kernel (forced) against dense_chain_mw_kernel on dense_mixed, three sweeps of phase 1 and three of phase 2:
    points, objective, max violation and every counter identical, both status words zero.  m = 33 with 1040 restarts: G not
    staged in LDS at small m; 600: staged; 2047 / 2048: 32 / 33 function slots per lane; 2689, 3584: equalities and
    two-interval constraints in slots >= 32 -- where the kernel used to pack relops and two-interval flags into words
    narrower than the slot count (an '==' in slot j >= 32 was read as '<=')."""
    funcs = dc.dense_mixed(n, m)
    prob = orc.Problem(funcs)
    X1, X2 = dc.starts(prob, funcs, n, R)
    vt2 = 1.05 * float(prob.eval_batch(X2)[1].max())
    res = [both_phases(make(eng_mod, funcs, mode=mode), X1, X2, vt2, 3, name) for mode, name in ((0, MW), (1, ONE))]
    assert_identical(res[0], res[1])


# ------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize('m,R,restarts', [(m, dc.C_R, None) for m in dc.C_GRID] + [dc.C_EXTRA])
def test_one_wave_kernel_beyond_eight_slots_follows_the_oracle(eng_mod, orc, m, R, restarts):
    """m > 3584 takes dense_chain_kernel without being asked (57 to 79 function slots per lane, equalities in slots >= 32).  It
    refuses a coordinate range, so the walk is block by block over all three blocks: the first coordinate of every block
    step has seen exactly the oracle's state -- within 1e-8 for every restart and both phases; the block as a whole within
    1e-6 or the oracle's own deviation.  The run with 1040 restarts compares three of them.  Measured: first visits at most
    1.6e-12, blocks at most 1.1e-7."""
    case = dc.walk_case(orc, m, R=R, restarts=restarts)
    e = make(eng_mod, case.funcs)
    assert dc.geometry(e.L, m)[0] > 8
    with pytest.raises(eng_mod.EngineError, match='coordinate range'):
        e.upload(case.X[1])
        e.cd_dense_block_step(1, 0, 0, seed=dc.SEED, first_index=dc.FIRST, coords=(0, 1))
    walk_and_judge(e, orc, case, ONE, (16,), (0, 1, 2), 'C m=%d R=%d' % (m, R), strict_first=True)


# ------------------------------------------------------------------------------------------------ D
GAP_R, GAP_ITERS = 12, 6


def cd_status(e):
    import ctypes as C
    R = e.pop_size
    st1, st2 = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
    e._chk(e.L.qcqpmi_cd_status(e.h, st1.ctypes.data_as(C.POINTER(C.c_int)), st2.ctypes.data_as(C.POINTER(C.c_int))))
    return st1, st2


@pytest.mark.parametrize('mode', (0, 1))
@pytest.mark.parametrize('name,phase1', [('g31', False), ('g64', False), ('g31', True)])
def test_lists_at_capacity_follow_the_oracle(eng_mod, orc, name, phase1, mode):
    """32 segments (the segment list exactly full) from 31 disjoint gaps, and from 64 gaps (the gap list exactly full) that
    merge into 31 islands, in both chain kernels: every restart follows orc.improve_cd -- same visits and accepted moves,
    points within 1e-6, status 0, no point inside a gap.  phase1: from starts inside the gaps, the bisection on the slack
    builds the 32 segments at every step."""
    funcs = dc.gap_problem(name)
    prob = orc.Problem(funcs)
    X0 = dc.gap_starts(name, GAP_R, feasible=not phase1)
    e = make(eng_mod, funcs, mode=mode)
    e.upload(X0)
    out = e.cd_run(phase1=phase1, num_iters=GAP_ITERS, seed=dc.SEED, first_index=dc.FIRST)
    assert e.last_cd_kernel() == (MW, ONE)[mode]
    X = e.download()
    assert not out['status1'].any() and not out['status2'].any()
    worst = 0.0
    for r in range(GAP_R):
        rng = orc.Rng(orc.RNG_KEYED, dc.SEED)
        rng.set_restart(dc.FIRST + r)
        x, s1, s2 = prob.improve_cd(X0[:, r], num_iters=GAP_ITERS, phase1=phase1, rng=rng)
        worst = max(worst, rel(X[:, r], x))
        assert out['visits2'][r] == s2[1] and out['accepted2'][r] == s2[2], (r, out['visits2'][r], s2)
        assert not phase1 or out['sweeps1'][r] == s1[0], r
        assert not dc.in_a_gap(name, X[0, r]), (r, X[0, r])
    print('\nD %s phase1=%s mode %d: worst restart %.2e off the oracle, %d moves accepted' % (name, phase1, mode, worst, out['accepted2'].sum()))
    assert worst < 1e-6
    assert out['accepted2'].sum() > 0 and (X[0] != X0[0]).any()


@pytest.mark.parametrize('mode', (0, 1))
@pytest.mark.parametrize('name', ('g32', 'g65'))
def test_lists_beyond_capacity_are_reported(eng_mod, name, mode):
    """33 segments, or 65 gaps in [L, H]: the run reports it -- the call fails with the 'more than 32 segments' message when
    no restart survives, else the restarts concerned carry status -4 -- and with 33 segments (a list cut short is still a
    subset of the feasible set) no point lands inside a gap."""
    X0 = dc.gap_starts(name, GAP_R)
    e = make(eng_mod, dc.gap_problem(name), mode=mode)
    e.upload(X0)
    try:
        out = e.cd_run(phase1=False, num_iters=GAP_ITERS, seed=dc.SEED, first_index=dc.FIRST)
    except eng_mod.EngineError as err:
        assert err.code == -4 and 'more than 32 segments' in str(err), str(err)      # QCQPMI_EUNSUPPORTED
        st1, st2 = cd_status(e)
        assert not st1.any() and (st2 == -4).all()
    else:
        st2 = out['status2']
        assert (st2 == -4).any() and set(st2.tolist()) <= {0, -4} and not out['status1'].any()
        assert np.all(np.isinf(out['f0'][st2 == -4])) and np.all(np.isfinite(out['f0'][st2 == 0]))
    assert e.last_cd_kernel() == (MW, ONE)[mode]
    if name == 'g32':
        X = e.download()
        for r in range(GAP_R):
            assert not dc.in_a_gap(name, X[0, r]), (r, X[0, r])


def test_lds_limit_runs_and_one_more_constraint_is_refused(eng_mod):
    """dense_le at n = 16: m = 5055 is the largest problem whose per-restart tables fit 160 KB of LDS (one wave per
    workgroup) -- it runs and returns status 0, values that a fresh evaluation confirms; m = 5056 is refused with
    QCQPMI_EUNSUPPORTED and the population is left as it was."""
    n, R = 16, 4
    m = dc.largest_m_one_wave()
    X0 = 0.5 * np.random.RandomState(2).randn(n, R)
    e = make(eng_mod, dc.dense_le(n, m))
    e.upload(X0)
    out = e.cd_run(phase1=True, num_iters=1, seed=dc.SEED, first_index=dc.FIRST)
    assert e.last_cd_kernel() == ONE
    assert not out['status1'].any() and not out['status2'].any()
    assert out['sweeps1'].sum() > 0 and (e.download() != X0).any()
    f0, mv = e.eval()
    assert rel(out['f0'], f0) < 1e-9 and np.max(np.abs(out['maxviol'] - mv)) < 1e-9
    e = make(eng_mod, dc.dense_le(n, m + 1))
    e.upload(X0)
    with pytest.raises(eng_mod.EngineError, match='too large for the per-restart LDS tables') as ei:
        e.cd_run(phase1=True, num_iters=1, seed=dc.SEED, first_index=dc.FIRST)
    assert ei.value.code == -4      # QCQPMI_EUNSUPPORTED
    assert np.array_equal(e.download(), X0)


# ------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize('zs', dc.E_ZS)
@pytest.mark.parametrize('m', dc.E_MS)
def test_full_driver_invariants(eng_mod, orc, monkeypatch, m, zs):
    """cd_run on dense_mixed at n = 72 through the default dispatch, 24 restarts, the K-split of the products left to the
    dispatch or forced: status words zero; the reported objective and max violation -- the values tracked through every
    accepted move, the fix-up plane of blocks >= 1 included -- within 1e-9 of a fresh oracle evaluation of the returned
    points; ran_phase2 consistent with the max violation against viol_tol; dense_chain_kernel identical to
    dense_chain_mw_kernel."""
    n, R = dc.N_DEFAULT, dc.E_R
    if zs is None:
        monkeypatch.delenv('QCQPMI_DENSE_ZS', raising=False)
    else:
        monkeypatch.setenv('QCQPMI_DENSE_ZS', str(zs))
    funcs = dc.dense_mixed(n, m)
    prob = orc.Problem(funcs)
    X1, X2 = dc.starts(prob, funcs, n, R)
    vt2 = 1.05 * float(prob.eval_batch(X2)[1].max())
    res = [both_phases(make(eng_mod, funcs, forced=False, mode=mode), X1, X2, vt2, 4, name) for mode, name in ((0, MW), (1, ONE))]
    for X, out, vt in res[0]:
        g0, gv = prob.eval_batch(X)
        print('\nE m=%d zs=%s viol_tol=%.3g: tracked f0 %.2e, max violation %.2e off a fresh evaluation; phase 2 ran for %d of %d'
              % (m, zs, vt, rel(out['f0'], g0), np.max(np.abs(out['maxviol'] - gv)), int(out['ran_phase2'].sum()), R))
        assert rel(out['f0'], g0) < 1e-9 and np.max(np.abs(out['maxviol'] - gv)) < 1e-9
        assert np.array_equal(out['ran_phase2'] != 0, out['maxviol'] < vt)
    assert_identical(res[0], res[1])
