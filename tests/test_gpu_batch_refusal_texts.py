"""The refusals of the six small-problem batch drivers (csrc/capi_small.hip: cd_small_batch, admm_small_batch, chain_small_batch,
sdr_small_batch, spectral_small_batch, admm_setup_batch) and of the checks they share, each provoked once: the code AND the full
message, against the literal text.  The other GPU files assert the code (and here and there a word); the drivers word their refusals
through shared helpers, which is where a text drifts.  Every refusal that arguments can reach is here -- not the occupancy and
HIP-error returns.  Shapes: n = 4, B = 2, R = 2; n = 65 and n = 129 for the two size limits; one P0 that is not symmetric per driver
(the only calls that launch: a few sweeps).  Run with `-m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from life_oracle import make

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
N, B, R = 4, 2, 2
NOT_SEPARABLE = '%s: the constraints are not separable (a constraint couples coordinates, or a coordinate carries more than 4)'
COUNT = '%s: B R = 2147483648 restarts, at most 2^30 - 1 per call'
CONS_NOT_FINITE = '%s: constraint 2 of problem 1 holds a coefficient that is not finite'
CONS_NO_COORDINATE = '%s: constraint 3 of problem 0 has p == 0 and q == 0: it touches no coordinate'
RHO = '%s: rho of problem 1 is not positive and finite'


@pytest.fixture(scope='module')
def ctx():
    """The contexts the refusals need, made once: name -> Engine."""
    from qcqp_amd import engine, problems
    assert engine.device_count() >= 1, 'no HIP device visible'
    bls = problems.boolean_least_squares(N, N + 2, seed=1)[0]
    P = np.zeros((N, N))
    P[0, 1] = P[1, 0] = 0.5
    funcs = dict(bls=bls, box=problems.box_qp(N, seed=1)[0], coupled=bls + [(P, np.zeros(N), -1.0, '<=')], free=bls[:1],
                 n65=problems.boolean_least_squares(65, 70, seed=1)[0], n129=problems.boolean_least_squares(129, 132, seed=1)[0])
    engines = {k: make(engine, f) for k, f in funcs.items()}
    engines['error'] = engine.EngineError
    yield engines
    for k, e in engines.items():
        if k != 'error':
            e.close()


def obj(n=N, b=B):
    """B objectives: symmetric P0s, q0s, r0s."""
    return np.stack([np.eye(n)] * b) if b else np.zeros((0, n, n)), np.zeros((b, n)), np.zeros(b)


def asymmetric(n=N):
    P0s = np.stack([np.eye(n)] * B)
    P0s[1, 1, 2] = 0.25
    return P0s


def cons_of(e, bad):
    """(B, m, 3) per-problem coefficients of x_i^2 == 1 with one bad entry: 'nan' or 'zero'."""
    c = np.tile(np.array([1.0, 0.0, -1.0]), (B, e.m, 1))
    if bad == 'nan':
        c[1, 1, 2] = np.nan
    else:
        c[0, 2, :2] = 0.0
    return c


def refused(ctx, code, text, call):
    """call() raises the EngineError of that code with exactly that text."""
    with pytest.raises(ctx['error']) as ex:
        call()
    assert ex.value.code == code and str(ex.value) == text, (ex.value.code, str(ex.value))


def refused_raw(e, code, text, rc):
    msg = e.L.qcqpmi_last_error(e.h).decode()
    assert rc == code and msg == text, (rc, msg)


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_coordinate_descent(ctx):
    name, e = 'cd_small_batch_run', ctx['bls']
    P0s, q0s, r0s = obj()
    refused(ctx, EUNSUPPORTED, NOT_SEPARABLE % name, lambda: ctx['coupled'].cd_small_batch_run(P0s, q0s, r0s, R))
    refused(ctx, EUNSUPPORTED, 'cd_small_batch_run: n = 65, the small-problem kernel takes n <= 64 (one lane per coordinate)',
            lambda: ctx['n65'].cd_small_batch_run(*obj(65), R))
    refused(ctx, EUNSUPPORTED, 'cd_small_batch_run: n = 129, the small-problem kernel takes n <= 128 (two coordinates per lane)',
            lambda: ctx['n129'].cd_batch_run(*obj(129), R))
    bad = 'cd_small_batch_run: bad B / R / num_iters / tol, or a missing input array'
    refused(ctx, EINVAL, bad, lambda: e.cd_small_batch_run(*obj(b=0), R))
    refused(ctx, EINVAL, bad, lambda: e.cd_small_batch_run(P0s, q0s, r0s, R, tol=0.0))
    tail = (1, None, 1, 3, 1e-2, 1e-4, 0, 1, 0, 1e-4) + (None,) * 14      # generated starts, no output wanted
    refused_raw(e, EINVAL, COUNT % name, e.L.qcqpmi_cd_small_batch_run(e.h, B, dp(P0s), dp(q0s), dp(r0s), 1 << 30, *tail))
    refused_raw(e, EINVAL, 'cd_small_batch_run_pc: missing cons (B x m x 3 coefficients)',
                e.L.qcqpmi_cd_small_batch_run_pc(e.h, B, dp(P0s), dp(q0s), dp(r0s), None, R, *tail))
    refused(ctx, EINVAL, CONS_NOT_FINITE % 'cd_small_batch_run_pc', lambda: e.cd_small_batch_run(P0s, q0s, r0s, R, cons=cons_of(e, 'nan')))
    refused(ctx, EINVAL, CONS_NO_COORDINATE % 'cd_small_batch_run_pc', lambda: e.cd_batch_run(P0s, q0s, r0s, R, cons=cons_of(e, 'zero')))
    refused(ctx, EINVAL, 'cd_small_batch_run: an objective matrix P0_b is not symmetric (or holds a NaN)',
            lambda: e.cd_small_batch_run(asymmetric(), q0s, r0s, R, num_iters=3))


def test_admm(ctx):
    name, e = 'admm_small_batch_run', ctx['bls']
    P0s, q0s, r0s = obj()
    rhos, Minvs = np.ones(B), np.stack([np.eye(N)] * B)
    refused(ctx, EUNSUPPORTED, NOT_SEPARABLE % name, lambda: ctx['coupled'].admm_small_batch_run(P0s, q0s, r0s, R, rhos, Minvs))
    refused(ctx, EUNSUPPORTED, 'admm_small_batch_run: n = 65, the small-problem kernel takes n <= 64 (one lane per coordinate)',
            lambda: ctx['n65'].admm_small_batch_run(*obj(65), R, rhos, np.stack([np.eye(65)] * B)))
    refused(ctx, EUNSUPPORTED, 'admm_small_batch_run: n = 129, the small-problem kernel takes n <= 128 (two coordinates per lane)',
            lambda: ctx['n129'].admm_batch_run(*obj(129), R, rhos, np.stack([np.eye(129)] * B)))
    refused(ctx, EINVAL, 'admm_small_batch_run: bad B / R / num_iters, or a missing input array',
            lambda: e.admm_small_batch_run(*obj(b=0), R, np.ones(0), np.zeros((0, N, N))))
    refused_raw(e, EINVAL, COUNT % name,
                e.L.qcqpmi_admm_small_batch_run(e.h, B, dp(P0s), dp(q0s), dp(r0s), None, dp(rhos), dp(Minvs), 1 << 30, 1, None, 1, 3, 1e-2, 1e4,
                                                0, 1, 0, 1e-4, *(None,) * 9))
    refused(ctx, EINVAL, 'admm_small_batch_run: the context has no constraint (the consensus average divides by m)',
            lambda: ctx['free'].admm_small_batch_run(P0s, q0s, r0s, R, rhos, Minvs))
    refused(ctx, EINVAL, RHO % name, lambda: e.admm_small_batch_run(P0s, q0s, r0s, R, np.array([1.0, 0.0]), Minvs))
    refused(ctx, EINVAL, CONS_NOT_FINITE % name, lambda: e.admm_small_batch_run(P0s, q0s, r0s, R, rhos, Minvs, cons=cons_of(e, 'nan')))
    refused(ctx, EINVAL, CONS_NO_COORDINATE % name, lambda: e.admm_batch_run(P0s, q0s, r0s, R, rhos, Minvs, cons=cons_of(e, 'zero')))
    asym = 'admm_small_batch_run: a matrix P0_b or Minv_b is not symmetric (or holds a NaN)'
    refused(ctx, EINVAL, asym, lambda: e.admm_small_batch_run(asymmetric(), q0s, r0s, R, rhos, Minvs, num_iters=3))
    refused(ctx, EINVAL, asym, lambda: e.admm_small_batch_run(P0s, q0s, r0s, R, rhos, asymmetric(), num_iters=3))


def test_chain(ctx):
    name, e = 'chain_small_batch_run', ctx['bls']
    P0s, q0s, r0s = obj()
    rhos, Minvs = np.ones(B), np.stack([np.eye(N)] * B)
    cd = dict(method=0, phase1=True, num_iters=3, tol=1e-4, viol_tol=1e-2)
    admm = dict(method=1, phase1=True, num_iters=3, tol=1e-2, viol_lim=1e4)
    both = dict(rhos=rhos, Minvs=Minvs)
    refused(ctx, EUNSUPPORTED, NOT_SEPARABLE % name, lambda: ctx['coupled'].chain_small_batch_run(P0s, q0s, r0s, R, [cd]))
    refused(ctx, EUNSUPPORTED, 'chain_small_batch_run: n = 65, the chain kernel takes n <= 64 (one lane per coordinate)',
            lambda: ctx['n65'].chain_small_batch_run(*obj(65), R, [cd]))
    refused(ctx, EINVAL, 'chain_small_batch_run: nstages = 0, 1 to 4 stages per launch (and their descriptors)',
            lambda: e.chain_small_batch_run(P0s, q0s, r0s, R, []))
    refused(ctx, EINVAL, 'chain_small_batch_run: nstages = 5, 1 to 4 stages per launch (and their descriptors)',
            lambda: e.chain_small_batch_run(P0s, q0s, r0s, R, [cd] * 5))
    refused(ctx, EINVAL, 'chain_small_batch_run: bad B / R, or a missing input array', lambda: e.chain_small_batch_run(*obj(b=0), R, [cd]))
    refused(ctx, EINVAL, 'chain_small_batch_run: stage 1 has method 2 (0: COORD_DESCENT, 1: ADMM)',
            lambda: e.chain_small_batch_run(P0s, q0s, r0s, R, [cd, dict(cd, method=2)]))
    refused(ctx, EINVAL, 'chain_small_batch_run: stage 1 has a bad num_iters / tol',
            lambda: e.chain_small_batch_run(P0s, q0s, r0s, R, [admm, dict(cd, tol=0.0)], **both))
    from qcqp_amd import _ffi
    desc = (_ffi.ChainStage * 1)(_ffi.ChainStage(0, 1, 3, 1e-4, 1e-2, 1e4))
    refused_raw(e, EINVAL, COUNT % name,
                e.L.qcqpmi_chain_small_batch_run(e.h, B, dp(P0s), dp(q0s), dp(r0s), None, None, None, 1 << 30, 1, None, 1, C.cast(desc, C.c_void_p),
                                                 0, 1, 0, 1e-4, *(None,) * 18))
    refused(ctx, EINVAL, 'chain_small_batch_run: an ADMM stage needs rhos and Minvs', lambda: e.chain_small_batch_run(P0s, q0s, r0s, R, [cd, admm]))
    refused(ctx, EINVAL, 'chain_small_batch_run: the context has no constraint (the consensus average of an ADMM stage divides by m)',
            lambda: ctx['free'].chain_small_batch_run(P0s, q0s, r0s, R, [admm], **both))
    refused(ctx, EINVAL, RHO % name, lambda: e.chain_small_batch_run(P0s, q0s, r0s, R, [admm], rhos=np.array([1.0, np.inf]), Minvs=Minvs))
    refused(ctx, EINVAL, CONS_NOT_FINITE % name, lambda: e.chain_small_batch_run(P0s, q0s, r0s, R, [cd], cons=cons_of(e, 'nan')))
    refused(ctx, EINVAL, CONS_NO_COORDINATE % name, lambda: e.chain_small_batch_run(P0s, q0s, r0s, R, [cd], cons=cons_of(e, 'zero')))
    refused(ctx, EINVAL, 'chain_small_batch_run: a matrix P0_b or Minv_b is not symmetric (or holds a NaN)',
            lambda: e.chain_small_batch_run(asymmetric(), q0s, r0s, R, [cd, admm], **both))


def test_sdr(ctx):
    e = ctx['bls']
    P0s, q0s, r0s = obj()
    refused(ctx, EUNSUPPORTED, 'sdr_small_batch: n = 65, the small-problem kernel takes n <= 64 (the full C_b in LDS)',
            lambda: ctx['n65'].sdr_small_batch(*obj(65), 1))
    refused(ctx, EUNSUPPORTED, 'sdr_small_batch: n = 129, the small-problem kernel takes n <= 128 (C_b packed, two coordinates per lane in the samples)',
            lambda: ctx['n129'].sdr_batch(*obj(129), 1))
    family = ('sdr_small_batch: the constraints are not of the unit-diagonal family (every coordinate exactly one constraint p x_i^2 + r == 0 '
              'with -r / p > 0)')
    refused(ctx, EUNSUPPORTED, family, lambda: ctx['box'].sdr_small_batch(P0s, q0s, r0s, 1))
    refused(ctx, EUNSUPPORTED, family, lambda: ctx['coupled'].sdr_small_batch(P0s, q0s, r0s, 1))
    refused(ctx, EINVAL, 'sdr_small_batch: bad B / S / max_sweeps / tol, or a missing input array', lambda: e.sdr_small_batch(*obj(b=0), 1))
    tail = (3, 1e-11, 0, 1, 0) + (None,) * 6      # keyed start, no output wanted
    refused_raw(e, EINVAL, 'sdr_small_batch: B = 2 problems with S = 1073741824 samples, at most 2^30 - 1 per call',
                e.L.qcqpmi_sdr_small_batch(e.h, B, dp(P0s), dp(q0s), dp(r0s), 1 << 30, *tail))
    refused_raw(e, EINVAL, 'sdr_small_batch_pc: missing ds (B x n)', e.L.qcqpmi_sdr_small_batch_pc(e.h, B, dp(P0s), dp(q0s), dp(r0s), None, 1, *tail))
    ds = np.ones((B, N))
    ds[1, 2] = 0.0
    refused(ctx, EINVAL, 'sdr_small_batch_pc: d of coordinate 2 of problem 1 is not a positive finite number',
            lambda: e.sdr_batch(P0s, q0s, r0s, 1, ds=ds))
    refused(ctx, EINVAL, 'sdr_small_batch: an objective matrix P0_b is not symmetric (or holds a NaN)',
            lambda: e.sdr_small_batch(asymmetric(), q0s, r0s, 1, max_sweeps=3))


def test_spectral(ctx):
    e = ctx['bls']
    P0s, q0s, r0s = obj()
    sphere = np.concatenate([np.ones(N), np.zeros(N), [-1.0]])      # sum x_i^2 - 1
    refused(ctx, EUNSUPPORTED, 'spectral_small_batch: n = 65, the small-problem kernel takes n <= 64 (A_b and Q_b in LDS, one lane per eigenvalue)',
            lambda: ctx['n65'].spectral_small_batch(*obj(65), np.concatenate([np.ones(65), np.zeros(65), [-1.0]]), '=='))
    refused(ctx, EUNSUPPORTED, 'spectral_small_batch: n = 129, the small-problem kernel takes n <= 128 (one array G_b in LDS, two eigenvalues per lane)',
            lambda: ctx['n129'].spectral_batch(*obj(129), np.concatenate([np.ones(129), np.zeros(129), [-1.0]]), '=='))
    bad = 'spectral_small_batch: bad B / max_sweeps / tol / agg_stride (0 or 2 n + 1), or a missing input array'
    refused(ctx, EINVAL, bad, lambda: e.spectral_small_batch(*obj(b=0), sphere, '=='))
    refused(ctx, EINVAL, bad, lambda: e.spectral_small_batch(P0s, q0s, r0s, sphere, '==', max_sweeps=-1))
    agg = sphere.copy()
    agg[1] = -1.0
    refused(ctx, EINVAL, 'spectral_small_batch: a = -1, beta = 0 of coordinate 1 of problem 0: a must be positive, both finite',
            lambda: e.spectral_small_batch(P0s, q0s, r0s, agg, '=='))
    agg = np.stack([sphere, sphere])
    agg[1, 2 * N] = 1.0
    refused(ctx, EINVAL, 'spectral_small_batch: rho^2 = sum beta^2 / (4 a) - gamma = -1 of problem 1 is not positive and finite',
            lambda: e.spectral_batch(P0s, q0s, r0s, agg, '<='))
    refused(ctx, EINVAL, 'spectral_small_batch: an objective matrix P0_b is not symmetric (or holds a NaN)',
            lambda: e.spectral_small_batch(asymmetric(), q0s, r0s, sphere, '==', max_sweeps=3))


def test_admm_setup(ctx):
    name, e = 'admm_batch_setup', ctx['bls']
    P0s = obj()[0]
    refused(ctx, EUNSUPPORTED, NOT_SEPARABLE % name, lambda: ctx['coupled'].admm_batch_setup(P0s))
    refused(ctx, EUNSUPPORTED, 'admm_batch_setup: n = 129, the setup kernels take n <= 128 (one array G_b in LDS, two eigenvalues per lane)',
            lambda: ctx['n129'].admm_batch_setup(obj(129)[0]))
    refused(ctx, EINVAL, 'admm_batch_setup: B = 0 problems, 1 to 2^30 - 1 per call', lambda: e.admm_batch_setup(obj(b=0)[0]))
    refused_raw(e, EINVAL, 'admm_batch_setup: the objective matrices P0s are missing',
                e.L.qcqpmi_admm_batch_setup(e.h, B, None, None, 30, 1e-15, None, None, None, None, None))
    refused(ctx, EINVAL, 'admm_batch_setup: max_sweeps = 0, at least one sweep', lambda: e.admm_batch_setup(P0s, max_sweeps=0))
    refused(ctx, EINVAL, 'admm_batch_setup: tol = 0 is not positive and finite', lambda: e.admm_batch_setup(P0s, tol=0.0))
    refused(ctx, EINVAL, 'admm_batch_setup: rho = -2 is not positive and finite', lambda: e.admm_batch_setup(P0s, rho=-2.0))
    refused(ctx, EINVAL, 'admm_batch_setup: the context has no constraint (the rule divides by m)', lambda: ctx['free'].admm_batch_setup(P0s))
    refused(ctx, EINVAL, 'admm_batch_setup: an objective matrix P0_b is not symmetric (or holds a NaN)', lambda: e.admm_batch_setup(asymmetric(), max_sweeps=3))
