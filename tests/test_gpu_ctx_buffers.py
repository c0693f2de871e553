"""The context's buffers (csrc/dev_buf.h) through growth and reuse: one context is driven small -> large -> small along every path
whose buffers grow on demand, and the last step must equal, bit for bit, what a FRESH context gives for that step alone.  Restarts
and samples are functions of (seed, index) only, so a buffer that is stale, too small, laid out for another size or not cleared where
a kernel expects zeros shows as a difference.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CD_KEYS = ('sweeps1', 'sweeps2', 'visits2', 'accepted2', 'ran_phase2', 'status1', 'status2', 'f0', 'maxviol')
STREAM_KEYS = CD_KEYS + ('best_index', 'best_f0', 'best_maxviol', 'best_x')


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def make(eng_mod, funcs):
    from qcqp_amd.form import QCQPForm
    return eng_mod.Engine(QCQPForm.from_arrays(funcs))


def same(a, b, keys):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def last_equals_fresh(eng_mod, funcs, sizes, step, keys, prepare=None):
    """step(engine, size) -> dict of arrays.  One context takes every size in turn; a fresh one takes the last size only."""
    e = make(eng_mod, funcs)
    if prepare:
        prepare(e)
    for size in sizes:
        grown = step(e, size)
    e.close()
    f = make(eng_mod, funcs)
    if prepare:
        prepare(f)
    fresh = step(f, sizes[-1])
    f.close()
    same(grown, fresh, keys)
    return grown


def test_sdr_sample_after_the_population_grew(eng_mod):
    """pop_sdr_sample keeps its standard normals in a buffer of its own, which goes when the population group is reallocated: S = 48
    samples, then a larger population (randn, 200 points), then S = 20 samples must find a buffer again.  n = 24 is not a multiple of
    16 and has two blocks: every call takes the affine_tiles_kernel branch."""
    from qcqp_amd import problems
    n = 24
    funcs = problems.boolean_least_squares(n, 8, seed=1)[0]
    rs = np.random.RandomState(3)
    F = rs.randn(n, n) / np.sqrt(n)
    mu = rs.randn(n)
    e = make(eng_mod, funcs)
    e.sdr_sample(mu, F, 48, seed=5, first_index=0)
    e.randn(200, seed=1)
    e.sdr_sample(mu, F, 20, seed=5, first_index=7)
    X = e.download()
    e.close()
    f = make(eng_mod, funcs)
    f.sdr_sample(mu, F, 20, seed=5, first_index=7)
    Xf = f.download()
    f.close()
    assert X.shape == (n, 20) and np.all(np.isfinite(X))
    assert np.array_equal(X, Xf)


def test_resident_cd_run_grow_shrink(eng_mod):
    """randn + cd_run, Boolean least squares, n = 48 (three blocks: the least the pipelined kernels take), R 20 -> 100 -> 20: the
    population group, the packed outputs and their pinned mirror."""
    from qcqp_amd import problems
    funcs = problems.boolean_least_squares(48, 24, seed=1)[0]

    def step(e, R):
        e.randn(R, seed=3, first_index=5)
        o = e.cd_run(num_iters=100, seed=7, first_index=5)
        o['X'] = e.download()
        return o

    o = last_equals_fresh(eng_mod, funcs, (20, 100, 20), step, CD_KEYS + ('X',))
    assert o['ran_phase2'].any()


def test_eval_and_weighted_product_grow_shrink(eng_mod):
    """eval(want_F=True) (d_F) and weighted_product (its work buffers and the pinned bounce buffer) on the problem and the sizes of
    the cd_run case."""
    from qcqp_amd import problems
    funcs = problems.boolean_least_squares(48, 24, seed=1)[0]
    w = np.zeros(len(funcs))
    w[0] = 1.5

    def step(e, R):
        e.randn(R, seed=3, first_index=5)
        f0, mv, F = e.eval(want_F=True)
        return dict(f0=f0, mv=mv, F=F, Y=e.weighted_product(w), X=e.download())

    o = last_equals_fresh(eng_mod, funcs, (20, 100, 20), step, ('f0', 'mv', 'F', 'Y', 'X'))
    P0 = funcs[0][0]
    P0 = P0.toarray() if hasattr(P0, 'toarray') else np.asarray(P0)
    assert np.max(np.abs(o['Y'] - 1.5 * P0.dot(o['X']))) <= 1e-12 * np.max(np.abs(o['Y']))


def test_factored_stream_run_grow_shrink(eng_mod):
    """cd_stream_reserve + cd_stream_run with an objective factor, n = 128 and rank 16 (eight blocks: the least the factored kernel
    takes), (K, R) (1, 20) -> (3, 40) -> (1, 20): the tiles' scratch, the prebuilt slacks, Y0, the packed outputs, the winners of the
    K populations.  The evaluation afterwards (128 points in the middle step: eight tiles of eight blocks) goes through the partial
    planes of the GEMM evaluation."""
    from qcqp_amd import lowrank, problems
    funcs = problems.boolean_least_squares(128, 16, seed=1)[0]
    P0 = funcs[0][0]
    P0 = P0.toarray() if hasattr(P0, 'toarray') else np.asarray(P0)
    L = lowrank.objective_factor(P0, max_rank=288)
    assert L is not None and L.shape[1] == 16

    def step(e, KR):
        K, R = KR
        e.cd_stream_reserve(K, R)
        o = e.cd_stream_run(K, R, num_iters=200, seed=900, first_index=11, first_stride=50000)
        assert 'factored' in e.last_cd_kernel(), e.last_cd_kernel()
        o['X'] = e.download()
        o['ef0'], o['emv'], o['eF'] = e.eval(want_F=True)
        return o

    o = last_equals_fresh(eng_mod, funcs, ((1, 20), (3, 40), (1, 20)), step, STREAM_KEYS + ('X', 'ef0', 'emv', 'eF'),
                          prepare=lambda e: e.cd_set_objective_factor(L))
    assert o['ran_phase2'].any()


def test_small_batch_grow_shrink(eng_mod):
    """cd_small_batch_run, B 2 -> 8 -> 2 problems of 24 variables: the call's own work buffer."""
    from qcqp_amd import problems
    fl = problems.boolean_least_squares_batch(8, 24, 36, seed=2)

    def step(e, B):
        P0s = np.stack([np.asarray(f[0][0]) for f in fl[:B]])
        q0s = np.stack([np.asarray(f[0][1]) for f in fl[:B]])
        r0s = np.array([f[0][2] for f in fl[:B]])
        return e.cd_small_batch_run(P0s, q0s, r0s, 16, num_iters=100, seed=5, first_index=3)

    o = last_equals_fresh(eng_mod, fl[0], (2, 8, 2), step, STREAM_KEYS + ('X',))
    assert o['X'].shape == (2, 16, 24) and o['ran_phase2'].any()


def test_dense_path_cd_run_grow_shrink(eng_mod):
    """Coupled constraints on the dense path (forced at n = 32 by the debug switch the API tests use), R 20 -> 40 -> 20: the product
    planes, the tracked function values, the per-restart state of a phase (laid out for the current population) and d_F."""
    from qcqp_amd import problems
    funcs = problems.dense_indefinite(32, 3)[0]

    def step(e, R):
        e.randn(R, seed=3, first_index=5)
        o = e.cd_run(num_iters=6, seed=7, first_index=5)
        assert e.last_cd_kernel().startswith('dense_chain'), e.last_cd_kernel()
        o['X'] = e.download()
        o['ef0'], o['emv'], o['eF'] = e.eval(want_F=True)
        return o

    last_equals_fresh(eng_mod, funcs, (20, 40, 20), step, CD_KEYS + ('X', 'ef0', 'emv', 'eF'),
                      prepare=lambda e: e.L.qcqpmi_debug_profile(e.h, 32 << 4, None))


def test_streaming_upload_twice_in_a_row(eng_mod, monkeypatch):
    """The streamed problem of test_streaming_upload_with_single_coordinate_constraints_mixed_in (n = 100: nine coupled constraints, a
    box constraint, a one-coordinate linear one and a constant one beyond the streaming limit) created, evaluated, run and closed
    twice: the staging buffer and the pre-packed matrices change owner at finalize and go with the context; the second context gives
    what the first gave."""
    import scipy.sparse as sp
    from qcqp_amd import problems
    n, R = 100, 24
    funcs, _, _ = problems.dense_indefinite(n, 9, seed=5)
    box = sp.csr_matrix(([1.0], ([17], [17])), shape=(n, n))
    qlin = np.zeros(n)
    qlin[40] = 2.0
    funcs = funcs[:4] + [(box, np.zeros(n), -9.0, '<=')] + funcs[4:7] + [(np.zeros((n, n)), qlin, -7.0, '<=')] + funcs[7:] + \
        [(np.zeros((n, n)), np.zeros(n), -1.0, '<=')]
    X0 = 1.5 * np.random.RandomState(2).randn(n, R)
    monkeypatch.setenv('QCQPMI_STREAM_LIMIT', '100000')
    res = []
    for _ in range(2):
        e = make(eng_mod, funcs)
        f0, mv, F = e.eval_batch(X0, want_F=True)
        o = e.cd_run(phase1=True, num_iters=4, seed=7, first_index=3)
        assert e.last_cd_kernel() == 'dense_chain_mw_kernel'
        o.update(ef0=f0, emv=mv, eF=F, X=e.download())
        res.append(o)
        e.close()
    same(res[0], res[1], CD_KEYS + ('ef0', 'emv', 'eF', 'X'))
