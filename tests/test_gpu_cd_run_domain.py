"""qcqpmi_cd_run on the resident population of a separable problem over the whole dispatch domain of launch_cd (csrc/capi_cd.hip):
every case uploads or generates R starts, calls Engine.cd_run, runs the fast separable oracle (Problem.improve_cd_sep, keyed
generator, pinned to the restatement by tests/test_oracle_golden.py and tests/test_cd_run_domain_cpu.py) on the same starts and
checks EVERY restart with life_oracle.check_restart: point 1e-9 relative, phase-1 sweeps, ran_phase2, phase-2 visits and accepted
moves, both status words zero, f0 within 1e-9 (1 + |f0|), max violation within 1e-12.  last_cd_kernel() names the kernel but not
its template arguments, so every case also asserts the instantiation from the lines QCQPMI_CD_DEBUG=1 makes launch_cd print
(`launch_cd: <kernel> <template arguments>`; one line for phase 1, one for phase 2).

The expected instantiation is typed in per case (CASES[..]['want']) AND computed by dispatch() below, which restates the
conditions of launch_cd -- n mod 16, NB, the LDS bounds rs_common / common / RQ_LDS_COMMON, RQ_NSIMD * RQ_MAXU, objclass, the
number of classes, symcls, MAXC, the chain share -- from the problem's arrays.  tests/test_cd_run_domain_cpu.py checks both
against each other without a GPU, and that the sizes of the XL = 0 cells ARE the first ones past their bound (the same family
one block of 16 smaller still prints XL 1).

Reached (R = 21 .. 40 restarts: two or three tiles, the last one partial, first_index nonzero):
  cd_phase2_q_kernel<CS>     CS 0 (NB 3, 4, forced at NB 60), 2 (forced), 4 (NB 5, 64), 6 (forced; at NB 66, its largest)
  cd_phase2_qs_kernel<CS>    CS 0 (NB 3), 4 (NB 64; R = 5; R = 37; a second run on the same context)
  cd_phase2_rs_kernel        FULL 1: XL x FA {1, 2} x SYM, all eight; n = 16, 32; the Boolean fallback at n = 1040
  cd_phase2_kernel<1,...>    XL x FA {0, 1, 2} at CL 1; CL 0 at XL 1 and 0; UN 1 for FA 1 and 2; n = 1, 15, 17
  cd_phase2_kernel<4,...>    box4, cut4 (CL 1), mixed_separable with two and three constraints per coordinate (CL 0), each at
                             n = 100, n = 96 and the first XL = 0 size
  cd_phase1_sep_kernel<1>, <4>
and across kernels: phase1 = False from feasible and infeasible uploaded points, num_iters = 0, 1, 2, the staged run
(cd_begin / cd_phase2 / cd_fetch) against the whole one bit for bit, independence of the population's size, exact ties.

NOT reachable from launch_cd (read off the code, not run):
  * cd_phase2_rs_kernel<.., FULL = false, ..>: the kernel needs K == 1; finalize counts classes over all n16 coordinates and the
    padded ones carry no constraint, so n % 16 != 0 gives K >= 2 as soon as ONE coordinate carries a constraint.  Only a problem
    without any constraint (m = 0, n % 16 != 0, a one-signed diagonal) would select FULL = false, SYM = false -- not a QCQP: phase 1
    of the reference raises there (max() of an empty list), its phase 2 alone takes all num_iters sweeps (the max violation of
    no constraint is -inf), and the kernel's closing max-violation pass reads the first constraint of the class, which does not
    exist.  No cell: nothing to compare.  FULL = false, SYM = true cannot be selected at all (symcls needs a constraint).
  * cd_phase2_kernel<1, XL, CL = true, FA = 0, UN = true> does not exist: UN is only instantiated with FA 1 / 2 (a mixed
    diagonal with K == 1 runs UN = false).  cd_phase2_kernel<4, ...> always runs FA = 0, UN = false.
  * cd_phase2_q_kernel / cd_phase2_qs_kernel with CS = 2 or 6 without the debug knob (bit 128 and bits 8..10 of dbg).

Size: 50 grid cases and 23 more, n <= 1057, R <= 40; the oracle's share is 9.6 s of CPU wall time for the whole file, 2.1 s for the
largest case (profiles/r09_cd_run_domain.md).  The file's time on an MI355X has NOT been measured yet: it was written and
checked on the CPU side while no device could be had, so its first run on one is its first run.  Run with `-m gpu`."""
import re
import struct

import numpy as np
import pytest

from life_oracle import ExactObjective, check_restart, make, oracle_runs

pytestmark = pytest.mark.gpu

LINE = re.compile(r'launch_cd: (cd_phase\w+ [^\n]*)')
COUNTERS = ('sweeps1', 'sweeps2', 'visits2', 'accepted2', 'ran_phase2', 'status1', 'status2')

# ---- launch_cd's thresholds (csrc/capi_cd.hip, csrc/cd_roles.h), in doubles unless said
LDS_BYTES = 160 * 1024
RQ_NSIMD, RQ_MAXU, RQ_CSMAX = 3, 20, 6
RQ_LDS_COMMON = 2 * RQ_NSIMD * 256 + 256 + 2 * 256 + 2 * 16 + 2 * 16 + 2 * 16 + 16 + 4 * 16 + 8 + 8 + 8
RS_COMMON = 2 * 6 * 256 + 256 + 2 * 256 + 2 * 16 + 2 * 16 + 16 + 4 * 16 + 8 + 8 + 8
QS_EXTRA = 8 + 16 * 5 + 8 * 6 + 64 * 10 + 32 + 16 + 8 * 5          # cd_queue_lds_bytes (csrc/cd_queue.hip)
DBG_NO_Q, DBG_CS = 64, 128                                          # bits of qcqpmi_debug_profile(enable >> 4)


def generic_common_bytes(maxc4, K):
    """`common` of launch_cd<MAXC>: partial tiles, G, diagonal block, slack, the block table and the class table (K <= 16)."""
    MAXC = 4 if maxc4 else 1
    slots = K * 16 if K <= 16 else 0
    return (4 * 256 + 256 + 256 + 3 * 16 + 512) * 8 + (2 * (MAXC + 1) * 256 + 256) * 8 + \
        (2 * (MAXC + 1) * slots + ((slots + 1) // 2) * 2) * 8 + 64


def shape(funcs):
    """What qcqpmi_finalize derives from a separable problem: n, K (classes of bit-identical constraint lists over all n16
    coordinates, the padded ones included), Kreal, maxc, objclass, symcls."""
    import scipy.sparse as sp
    n = int(np.asarray(funcs[0][1]).size)
    n16 = (n + 15) // 16 * 16
    lists = [[] for _ in range(n16)]
    for P, q, r, relop in funcs[1:]:
        Pc = sp.coo_matrix(P)
        q = np.asarray(q, dtype=np.float64).ravel()
        coords = set(int(i) for i in Pc.row[Pc.data != 0]) | set(int(i) for i in np.nonzero(q)[0])
        assert len(coords) == 1 and (Pc.row == Pc.col).all(), 'not separable'
        i = coords.pop()
        lists[i].append(struct.pack('ddd', float(Pc.data.sum()), float(q[i]), float(r)) + relop.encode())
    keys = [b'|'.join(l) + b'#%d' % len(l) for l in lists]
    P0 = funcs[0][0]
    d = np.asarray(P0.diagonal() if hasattr(P0, 'diagonal') else np.diag(P0), dtype=np.float64)
    oc = 1 if (d > 0).all() else (2 if (d == 0).all() else 0)
    K, Kreal, maxc = len(set(keys)), len(set(keys[:n])), max(len(l) for l in lists)
    sym = False
    if Kreal == 1 and maxc == 1:
        p, q, r = struct.unpack('ddd', lists[0][0][:24])
        sym = q == 0.0 and lists[0][0][24:] == b'==' and p != 0.0
    return dict(n=n, n16=n16, NB=n16 // 16, K=K, Kreal=Kreal, maxc=maxc, objclass=oc, symcls=sym)


def dispatch(s, queue=0, dbg=0, generic=False):
    """The phase-2 line launch_cd prints for a problem of shape s (queue: qcqpmi_cd_queue mode 0 / 1; dbg: the debug word;
    generic: force_generic)."""
    n, n16, NB, K, oc = s['n'], s['n16'], s['NB'], s['K'], s['objclass']
    maxc4 = s['maxc'] > 1
    if not maxc4 and K == 1 and oc == 1 and s['symcls'] and n % 16 == 0 and not generic and not dbg & DBG_NO_Q:
        cs = (dbg >> 8) & 7 if dbg & DBG_CS else 4
        cs = min(cs, RQ_CSMAX)
        if cs >= NB:
            cs = 0
        cs &= ~1
        in_range = NB - cs <= RQ_NSIMD * RQ_MAXU and NB >= 3
        if queue == 1 and in_range and (RQ_LDS_COMMON + QS_EXTRA + n16 * 16) * 8 <= LDS_BYTES:
            return 'cd_phase2_qs_kernel CS %d' % cs
        if in_range and (RQ_LDS_COMMON + n16 * 16) * 8 <= LDS_BYTES:
            return 'cd_phase2_q_kernel CS %d' % cs
    if not maxc4 and K == 1 and oc in (1, 2) and not generic:
        xl = (RS_COMMON + n16 * 16) * 8 <= LDS_BYTES
        return 'cd_phase2_rs_kernel XL %d FA %d FULL %d SYM %d' % (xl, oc, n % 16 == 0, s['symcls'])
    xl = generic_common_bytes(maxc4, K) + n16 * 16 * 8 <= LDS_BYTES
    cl = K <= 16
    fa = 0 if maxc4 else oc
    un = cl and K == 1 and fa in (1, 2)
    return 'cd_phase2_kernel MAXC %d XL %d CL %d FA %d UN %d' % (4 if maxc4 else 1, xl, cl, fa, un)


# ---- families
def _classes23(n):
    """Least squares + ridge with per-coordinate bounds x_i^2 <= b_i^2, 23 different b: more classes than the class table holds."""
    from qcqp_amd import problems
    funcs = problems.box_least_squares(n, max(4, n // 2), bound=1.0, seed=2)[0]
    return [funcs[0]] + [(P, q, -(0.5 + (i % 23) / 23.0) ** 2, relop) for i, (P, q, r, relop) in enumerate(funcs[1:])]


def family(fam, n):
    from qcqp_amd import problems
    if fam == 'bls':            # a third of n rows: rank-deficient, many sweeps
        return problems.boolean_least_squares(n, max(4, n // 3), seed=1)[0]
    if fam == 'maxcutw':        # zero diagonal, x_i^2 == 1; weighted edges: no exact ties between cuts
        return problems.maxcut(n, 0.5, seed=1, weighted=True)[0]
    if fam == 'box':            # positive diagonal, one inequality class
        return problems.box_least_squares(n, max(4, n // 2), bound=1.0, seed=1)[0]
    if fam == 'boxz':           # zero diagonal, one inequality class: the indefinite box QP with its diagonal removed
        return problems.box_qp(n, seed=3, zero_every=1)[0]
    if fam == 'boxmix':         # a diagonal of all three signs, one inequality class
        return problems.box_qp(n, seed=3, zero_every=3)[0]
    if fam == 'classes23':
        return _classes23(n)
    if fam in ('mixed2', 'mixed3'):     # two / three constraints per coordinate, a class per coordinate
        from test_gpu_parity import mixed_separable
        return mixed_separable(n, int(fam[-1]), seed=5 + int(fam[-1]), objective='indef')
    if fam in ('ties_bls', 'ties_ann'):
        from test_gpu_life_domain import _diagonal_ties
        return _diagonal_ties(n, fam[5:])
    return problems.multi_class(fam, n, seed=1)


def case(fam, n, want, R=21, queue=0, dbg=0, generic=False, iters=1000, first=3, **kw):
    return dict(fam=fam, n=n, want=want, R=R, queue=queue, dbg=dbg, generic=generic, iters=iters, first=first, **kw)


def forced_cs(cs):
    return DBG_CS | (cs << 8)


Q, QS, RS, GEN = 'cd_phase2_q_kernel CS %d', 'cd_phase2_qs_kernel CS %d', 'cd_phase2_rs_kernel XL %d FA %d FULL %d SYM %d', \
    'cd_phase2_kernel MAXC %d XL %d CL %d FA %d UN %d'

CASES = {
    # ---- cd_phase2_q_kernel: Boolean least squares, n a multiple of 16, cd_queue(0)
    'q-cs0-nb3': case('bls', 48, Q % 0, R=21),
    'q-cs0-nb4': case('bls', 64, Q % 0, R=37),
    'q-cs4-nb5': case('bls', 80, Q % 4, R=40),
    'q-cs4-nb64': case('bls', 1024, Q % 4, R=21),
    'q-cs2-forced': case('bls', 256, Q % 2, R=21, dbg=forced_cs(2)),
    'q-cs6-forced': case('bls', 256, Q % 6, R=21, dbg=forced_cs(6)),
    'q-cs6-nb66': case('bls', 1056, Q % 6, R=21, dbg=forced_cs(6)),       # NB - 6 = 60: the largest it admits
    'q-cs0-nb60': case('bls', 960, Q % 0, R=21, dbg=forced_cs(0)),        # NB = 60: the largest without a share
    # ---- cd_phase2_qs_kernel: cd_queue(1)
    'qs-nb3': case('bls', 48, QS % 0, R=21, queue=1),
    'qs-nb64': case('bls', 1024, QS % 4, R=21, queue=1),
    'qs-r5': case('bls', 128, QS % 4, R=5, queue=1),                      # fewer restarts than slots
    'qs-r37': case('bls', 128, QS % 4, R=37, queue=1),
    # ---- cd_phase2_rs_kernel, FULL = 1: SYM x FA x XL
    'rs-sym-fa1-n16': case('bls', 16, RS % (1, 1, 1, 1), R=21),           # NB < 3
    'rs-sym-fa1-n32': case('bls', 32, RS % (1, 1, 1, 1), R=37),
    'rs-sym-fa1-xl0': case('bls', 1040, RS % (0, 1, 1, 1), R=21),         # the Boolean fallback: the first n cd_phase2_q_kernel refuses
    'rs-sym-fa2-xl1': case('maxcutw', 256, RS % (1, 2, 1, 1), R=37),      # FA = 2 past n = 128
    'rs-sym-fa2-xl0': case('maxcutw', 1040, RS % (0, 2, 1, 1), R=21),
    'rs-box-fa1-xl1': case('box', 112, RS % (1, 1, 1, 0), R=37),
    'rs-box-fa1-xl0': case('box', 1040, RS % (0, 1, 1, 0), R=21),
    'rs-box-fa2-xl1': case('boxz', 112, RS % (1, 2, 1, 0), R=37),
    'rs-box-fa2-xl0': case('boxz', 1040, RS % (0, 2, 1, 0), R=21),
    'rs-box-fa1-n16': case('box', 16, RS % (1, 1, 1, 0), R=21),
    'rs-box-fa2-n32': case('boxz', 32, RS % (1, 2, 1, 0), R=21),
    # ---- cd_phase2_kernel<1, ...>: n not a multiple of 16 (K = 2 with the padding class)
    'g1-fa1-xl1': case('box', 100, GEN % (1, 1, 1, 1, 0), R=37),
    'g1-fa2-xl1': case('boxz', 100, GEN % (1, 1, 1, 2, 0), R=37),
    'g1-fa0-xl1': case('boxmix', 100, GEN % (1, 1, 1, 0, 0), R=37),
    'g1-fa1-xl0': case('box', 1057, GEN % (1, 0, 1, 1, 0), R=21),
    'g1-fa2-xl0': case('boxz', 1057, GEN % (1, 0, 1, 2, 0), R=21),
    'g1-fa0-xl0': case('boxmix', 1057, GEN % (1, 0, 1, 0, 0), R=21),
    'g1-fa0-mult16': case('boxmix', 256, GEN % (1, 1, 1, 0, 0), R=21),    # a mixed diagonal with K = 1: still UN = 0
    'g1-cl0-xl1': case('classes23', 100, GEN % (1, 1, 0, 1, 0), R=37),
    'g1-cl0-xl0': case('classes23', 1057, GEN % (1, 0, 0, 1, 0), R=21),
    'g1-un-fa1': case('bls', 96, GEN % (1, 1, 1, 1, 1), R=21, generic=True),
    'g1-un-fa2': case('maxcutw', 96, GEN % (1, 1, 1, 2, 1), R=21, generic=True),
    'g1-n1': case('box', 1, GEN % (1, 1, 1, 1, 0), R=21),
    'g1-n15': case('bls', 15, GEN % (1, 1, 1, 1, 0), R=21),
    'g1-n17': case('maxcutw', 17, GEN % (1, 1, 1, 2, 0), R=21),
    # ---- cd_phase2_kernel<4, ...> and cd_phase1_sep_kernel<4>
    'g4-box4-100': case('box4', 100, GEN % (4, 1, 1, 0, 0), R=37),
    'g4-box4-96': case('box4', 96, GEN % (4, 1, 1, 0, 0), R=21),
    'g4-box4-xl0': case('box4', 913, GEN % (4, 0, 1, 0, 0), R=21),
    'g4-cut4-100': case('cut4', 100, GEN % (4, 1, 1, 0, 0), R=37),
    'g4-cut4-96': case('cut4', 96, GEN % (4, 1, 1, 0, 0), R=21),
    'g4-cut4-xl0': case('cut4', 944, GEN % (4, 0, 1, 0, 0), R=21),        # K = 4 at a multiple of 16: the bound is one block higher
    'g4-mixed2-100': case('mixed2', 100, GEN % (4, 1, 0, 0, 0), R=37),
    'g4-mixed2-96': case('mixed2', 96, GEN % (4, 1, 0, 0, 0), R=21),
    'g4-mixed2-xl0': case('mixed2', 961, GEN % (4, 0, 0, 0, 0), R=21),
    'g4-mixed3-100': case('mixed3', 100, GEN % (4, 1, 0, 0, 0), R=37),
    'g4-mixed3-96': case('mixed3', 96, GEN % (4, 1, 0, 0, 0), R=21),
    'g4-mixed3-xl0': case('mixed3', 961, GEN % (4, 0, 0, 0, 0), R=21),
    # ---- exact ties (a diagonal objective: every phase-2 visit draws); four sweeps, a walk among equal candidates never converges
    'ties-rs-xl0': case('ties_bls', 1040, RS % (0, 1, 1, 1), R=21, iters=4, converges=False),
    'ties-g4': case('ties_ann', 100, GEN % (4, 1, 1, 0, 0), R=37, iters=4, converges=False),
}

# the cells of CASES that sit at the first size past a bound of the dispatch: one block of 16 below, the line still says `below`
# (the Boolean family below n = 1040 runs cd_phase2_q_kernel: its fallback is the first size that kernel refuses, and the LDS
# bound of cd_phase2_rs_kernel is read off its siblings at the same size)
FIRST_PAST = [(name, 'XL 1') for name in sorted(CASES) if name.endswith('-xl0') and name not in ('ties-rs-xl0', 'rs-sym-fa1-xl0')] + \
    [('rs-sym-fa1-xl0', 'cd_phase2_q_kernel CS 4')]
# ... and the last size inside one: one block of 16 above, the line no longer says `inside`
LAST_INSIDE = [('q-cs4-nb64', 'cd_phase2_q_kernel'), ('q-cs6-nb66', 'cd_phase2_q_kernel'), ('q-cs0-nb60', 'cd_phase2_q_kernel'),
               ('qs-nb64', 'cd_phase2_qs_kernel')]


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


@pytest.fixture(autouse=True)
def cd_debug(monkeypatch):
    monkeypatch.setenv('QCQPMI_CD_DEBUG', '1')      # launch_cd prints the instantiation it launches on stderr


def engine_for(eng_mod, funcs, queue=0, dbg=0, generic=False):
    e = make(eng_mod, funcs)
    assert e.separable
    e.cd_queue(queue)
    e.L.qcqpmi_debug_profile(e.h, (dbg << 4) | (2 if generic else 0), None)
    return e


def run(e, capfd, R, seed, first, iters=1000, phase1=True, X0=None, staged=False):
    """One cd_run on engine e from keyed normals (or the uploaded X0): (starts, outputs, points, lines of launch_cd)."""
    if X0 is None:
        e.randn(R, seed=seed, first_index=first)
        X0 = e.download()
    else:
        e.upload(X0)
    capfd.readouterr()
    if staged:
        e.cd_begin(phase1=phase1, num_iters=iters, seed=seed, first_index=first)
        e.cd_phase2()
        o = e.cd_fetch()
    else:
        o = e.cd_run(phase1=phase1, num_iters=iters, seed=seed, first_index=first)
    lines = LINE.findall(capfd.readouterr().err)
    return X0, o, e.download(), lines


def check_lines(lines, want, maxc4, phase1=True):
    p1 = ['cd_phase1_sep_kernel MAXC %d' % (4 if maxc4 else 1)] if phase1 else []
    assert lines == p1 + [want], (lines, want)


def check_all(orc, funcs, X0, o, X, seed, first, iters, tag, phase1=True, converges=True):
    """Every restart against the oracle; returns the oracle's results."""
    prob, exact = orc.Problem(funcs), ExactObjective(funcs)
    R = X0.shape[1]
    res = oracle_runs(orc, prob, [(X0[:, r], seed, first + r) for r in range(R)], iters, phase1=phase1)
    for r in range(R):
        if converges:
            assert res[r][1][0] < iters and res[r][2][0] < iters, (tag, r, 'the oracle did not converge', res[r][1], res[r][2])
        check_restart(o, X, r, res[r], iters, tag, exact)
    return res


@pytest.mark.parametrize('name', sorted(CASES))
def test_cd_run_domain_vs_oracle(eng_mod, orc, capfd, name):
    c = CASES[name]
    funcs = family(c['fam'], c['n'])
    s = shape(funcs)
    assert dispatch(s, c['queue'], c['dbg'], c['generic']) == c['want'], (name, s)
    seed = 300 + c['n']
    e = engine_for(eng_mod, funcs, c['queue'], c['dbg'], c['generic'])
    X0, o, X, lines = run(e, capfd, c['R'], seed, c['first'], c['iters'])
    assert e.last_cd_kernel() == c['want'].split()[0], (name, e.last_cd_kernel())
    e.close()
    check_lines(lines, c['want'], s['maxc'] > 1)
    assert o['ran_phase2'].any(), 'no restart reached phase 2'
    check_all(orc, funcs, X0, o, X, seed, c['first'], c['iters'], (name,), converges=c.get('converges', True))


def test_queue_is_reset_between_two_runs_on_one_context(eng_mod, orc, capfd):
    """cd_phase2_qs_kernel twice on the same context, another population and another first_index the second time: the device-side
    queue and the per-restart outputs start from zero again."""
    funcs = family('bls', 128)
    e = engine_for(eng_mod, funcs, queue=1)
    for R, first in ((37, 3), (21, 1000)):
        X0, o, X, lines = run(e, capfd, R, 17, first)
        check_lines(lines, QS % 4, False)
        check_all(orc, funcs, X0, o, X, 17, first, 1000, ('qs twice', first))
    e.close()


def gate_starts(n, R, fam=None):
    """Points just inside |x_i| = 1 (box4: just inside each class's own bound, 0.7 and [-1/2, 1] for classes 1 and 2), about a third
    of them scaled by 1 .. 2 afterwards: those fail the gate."""
    rs = np.random.RandomState(17)
    X0 = np.sign(rs.randn(n, R)) * (1.0 - 1e-3 * rs.rand(n, R))
    if fam == 'box4':
        X0[1::4] *= 0.7
        X0[2::4] *= 0.5
    far = rs.rand(R) < 0.3
    X0[:, far] *= 1.0 + rs.rand(int(far.sum()))
    return X0


GATE = [('q', 'bls', 80, 0, Q % 4), ('rs-xl0', 'box', 1040, 0, RS % (0, 1, 1, 0)), ('g1-fa0', 'boxmix', 100, 0, GEN % (1, 1, 1, 0, 0)),
        ('g4', 'box4', 100, 0, GEN % (4, 1, 1, 0, 0)), ('qs', 'bls', 80, 1, QS % 4)]


@pytest.mark.parametrize('tag,fam,n,queue,want', GATE, ids=[g[0] for g in GATE])
def test_without_phase1_from_feasible_and_infeasible_points(eng_mod, orc, capfd, tag, fam, n, queue, want):
    """phase1 = False on uploaded points: near-feasible ones (gate_starts) pass the gate;
    the ones scaled by 1 .. 2 do not, stay as uploaded and report the objective of the uploaded point."""
    R = 37
    funcs = family(fam, n)
    X0 = gate_starts(n, R, fam)
    e = engine_for(eng_mod, funcs, queue)
    _, o, X, lines = run(e, capfd, R, 29, 11, phase1=False, X0=X0)
    e.close()
    check_lines(lines, want, shape(funcs)['maxc'] > 1, phase1=False)
    ran = o['ran_phase2'].astype(bool)
    assert ran.any() and (~ran).any()
    assert np.array_equal(X[:, ~ran], X0[:, ~ran])
    check_all(orc, funcs, X0, o, X, 29, 11, 1000, ('gate', tag), phase1=False)


LIMITS = [('q', 'bls', 80, Q % 4), ('rs-xl0', 'maxcutw', 1040, RS % (0, 2, 1, 1)), ('g1-xl0', 'boxmix', 1057, GEN % (1, 0, 1, 0, 0)),
          ('g4', 'cut4', 100, GEN % (4, 1, 1, 0, 0))]


@pytest.mark.parametrize('iters', [0, 1, 2])
@pytest.mark.parametrize('tag,fam,n,want', LIMITS, ids=[g[0] for g in LIMITS])
def test_sweep_limits(eng_mod, orc, capfd, tag, fam, n, want, iters):
    """num_iters = 0, 1, 2: restarts stop at the limit in both phases."""
    funcs = family(fam, n)
    e = engine_for(eng_mod, funcs)
    X0, o, X, lines = run(e, capfd, 21, 71 + iters, 5, iters=iters)
    e.close()
    check_lines(lines, want, shape(funcs)['maxc'] > 1)
    check_all(orc, funcs, X0, o, X, 71 + iters, 5, iters, ('limit', tag, iters), converges=False)


STAGED = [('q', 'bls', 80, 0, Q % 4), ('qs', 'bls', 80, 1, QS % 4), ('rs-xl0', 'box', 1040, 0, RS % (0, 1, 1, 0)),
          ('g1', 'boxmix', 100, 0, GEN % (1, 1, 1, 0, 0)), ('g4-xl0', 'box4', 913, 0, GEN % (4, 0, 1, 0, 0))]


@pytest.mark.parametrize('tag,fam,n,queue,want', STAGED, ids=[g[0] for g in STAGED])
def test_staged_run_equals_whole_run_and_population_size_does_not_matter(eng_mod, capfd, tag, fam, n, queue, want):
    """qcqpmi_cd_run_stage 1 -> 2 -> 3 against stage 0 on the same starts: bit-identical points, objectives, violations and
    counters.  And the same global restart indices in a population of 21 and in one of 40: bit-identical again (a restart's
    result depends on its global index, not on its tile or on who shares it)."""
    funcs = family(fam, n)
    e = engine_for(eng_mod, funcs, queue)
    X0, o0, Xa, la = run(e, capfd, 40, 13, 7)
    _, o1, Xb, lb = run(e, capfd, 40, 13, 7, staged=True)
    _, o2, Xc, lc = run(e, capfd, 21, 13, 7)
    e.close()
    for lines in (la, lb, lc):
        check_lines(lines, want, shape(funcs)['maxc'] > 1)
    assert np.array_equal(Xa, Xb) and np.array_equal(Xa[:, :21], Xc)
    for key in COUNTERS + ('f0', 'maxviol'):
        assert np.array_equal(o0[key], o1[key]) and np.array_equal(o0[key][:21], o2[key]), key


def workloads():
    """Every oracle workload of this file: (tag, family, n, R, seed, first_index, num_iters, phase1, uploaded starts or None,
    converges).  tests/test_cd_run_domain_cpu.py runs them without a GPU (keyed normals from the oracle's own generator)."""
    for name in sorted(CASES):
        c = CASES[name]
        yield (name, c['fam'], c['n'], c['R'], 300 + c['n'], c['first'], c['iters'], True, None, c.get('converges', True))
    for R, first in ((37, 3), (21, 1000)):
        yield ('qs twice %d' % first, 'bls', 128, R, 17, first, 1000, True, None, True)
    for tag, fam, n, _, _ in GATE:
        yield ('gate ' + tag, fam, n, 37, 29, 11, 1000, False, gate_starts(n, 37, fam), True)
    for tag, fam, n, _ in LIMITS:
        for iters in (0, 1, 2):
            yield ('limit %s %d' % (tag, iters), fam, n, 21, 71 + iters, 5, iters, True, None, False)
