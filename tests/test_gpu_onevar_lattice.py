"""The one-variable solver's device restatements on the degenerate-case lattice of tests/onevar_cases.py, compiled for gfx950:
every instantiation the coordinate-descent kernels run (qcqpmi_onevar_variant_batch: the end-point sweep and the closed form for
one constraint at 1, 2 and 4 slots; qcqpmi_p1_visit_batch: the generic phase-1 visit at 1 and 4 slots, the band visit, the fused
band visits with and without the fast first phase) against the oracle in keyed mode, bit for bit -- status, every piece of the
feasible set, the point, keyed draws included; x_i, moved, vafter and status for the visits -- with the comparison functions the
host build is held to in tests/test_onevar_lattice_cpu.py.  No tolerance anywhere: the same IEEE operations in the same order,
-ffp-contract=off on both sides.

The last part hands degenerate coordinate lists to the real kernels: the separable families of onevar_cases (a touching pair widened
to [-eps, eps], x^2 == 1 as two inequalities, equal linear bounds, (x - 1/2)^2 == 1/4, a leading coefficient of exactly 1e-4 and one
of 1.5e-4, a disc with two holes; a least-squares + ridge objective and one with a zero diagonal) through Engine.cd_run -- 7 classes:
cd_phase2_kernel<4> with the class table (compute_set / SetTable) and cd_phase1_sep_kernel<4>; 23 classes: without the table; one
constraint per coordinate: cd_phase2_kernel<1> and cd_phase1_sep_kernel<1>, each asserted from the QCQPMI_CD_DEBUG lines -- and
through Engine.cd_batch_run (cd_small_kernel<4>, <4,w2>, <1,w2>; B = 3, R = 8), n = 48 / 96 / 112, 21 restarts from first_index 3,
num_iters = 40, every restart checked by life_oracle.check_restart against Problem.improve_cd_sep in keyed mode at the tolerances
that function carries.  tests/test_onevar_lattice_cpu.py asserts that none of these workloads degenerates under the oracle.
The one-constraint family also runs through Engine.cd_stream_run (qcqpmi_cd_stream_run, one population of 21 restarts): the stream
plan (cd_life2_config, csrc/cd_life_plan.h) takes it -- one constraint per coordinate, four classes -- as the multi-class kinds of
cd_life_kernel, GENK on the ridge objective and LINK on the zero diagonal, at n = 48 (<3, cs 0>), 96 and 112 (<3, cs 2>); the
(nmw, cs, kind) triple is asserted from the QCQPMI_L2_DEBUG line.  The plan refuses mix7 and mix23 (three constraints on a
coordinate; 7 and more classes against its four): they are not forced through it (tests/test_onevar_lattice_cpu.py asserts both answers)."""
import ctypes as C

import numpy as np
import pytest

import onevar_cases as oc
import test_gpu_cd_run_domain as dom
import test_gpu_life_curvature as lc
import test_gpu_small_batch as sb
import test_gpu_wide_batch as wb

pytestmark = pytest.mark.gpu

SEED, SWEEP = 123, 3
IP = C.POINTER(C.c_int)


@pytest.fixture(scope='module')
def L():
    from qcqp_amd import _ffi
    return _ffi.lib()


def dp(a):
    from qcqp_amd import _ffi
    return a.ctypes.data_as(_ffi.c_dp)


@pytest.fixture(scope='module')
def lattice():
    return oc.onevar_arrays()


def device_onevar(L, lattice, idx, variant=None):
    f0, fs, nf, s = (np.ascontiguousarray(a[idx]) for a in lattice)
    N = len(idx)
    x, st, Cs, nC = np.zeros(N), np.zeros(N, dtype=np.int32), np.zeros((N, 5, 2)), np.zeros(N, dtype=np.int32)
    if variant is None:
        rc = L.qcqpmi_onevar_qcqp_batch(0, N, dp(f0), dp(fs), nf.ctypes.data_as(IP), dp(s), SEED, dp(x), st.ctypes.data_as(IP), dp(Cs),
                                        nC.ctypes.data_as(IP))
    else:
        rc = L.qcqpmi_onevar_variant_batch(0, variant, N, dp(f0), dp(fs), nf.ctypes.data_as(IP), dp(s), SEED, dp(x), st.ctypes.data_as(IP),
                                           dp(Cs), nC.ctypes.data_as(IP))
    assert rc == 0, L.qcqpmi_last_error(None)
    return dict(status=st, x=x, nC=nC, C=Cs)


@pytest.mark.parametrize('name', sorted(oc.ONEVAR_VARIANTS))
def test_set_builder_and_minimiser_on_device_equal_the_oracle(orc, L, lattice, name):
    f0, fs, nf, s = lattice
    idx = oc.onevar_subset(name, nf)
    assert len(idx) >= 1000
    got = device_onevar(L, lattice, idx, oc.ONEVAR_VARIANTS[name])
    ref = oc.oracle_onevar(orc, f0[idx], fs[idx], nf[idx], s[idx], mode=orc.RNG_KEYED, seed=SEED)
    bad = oc.compare_onevar(got, ref, np.arange(len(idx)), oc.ONEVAR_MAXC[name])
    print(name, len(idx), 'cases,', len(bad), 'mismatches')
    assert len(bad) == 0, [(oc.describe_onevar(idx[b], f0, fs, nf, s), {k: v[b] for k, v in got.items()}, {k: v[b] for k, v in ref.items()}) for b in bad[:3]]


def test_existing_entry_equals_sweep4_byte_for_byte(orc, L, lattice):
    """qcqpmi_onevar_qcqp_batch on the whole lattice: equal to the oracle including C_out / nC_out and the drawn points, and to
    variant sweep4 in every byte of every output."""
    f0, fs, nf, s = lattice
    idx = np.arange(len(nf))
    old = device_onevar(L, lattice, idx)
    new = device_onevar(L, lattice, idx, oc.ONEVAR_VARIANTS['sweep4'])
    ref = oc.oracle_onevar(orc, f0, fs, nf, s, mode=orc.RNG_KEYED, seed=SEED)
    assert len(oc.compare_onevar(old, ref, idx, 4)) == 0
    for k in old:
        assert old[k].tobytes() == new[k].tobytes(), k


def test_feasible_intervals_on_every_atom_and_slack(orc, L):
    """qcqpmi_feasible_intervals_batch on every (atom, slack) pair of the lattice against the oracle's feasible_intervals, as G3:
    the count and every end point, ==."""
    pairs = [(a, sl) for a in oc.ATOMS for sl in oc.SLACKS]
    N = len(pairs)
    pqrs = np.ascontiguousarray([[a[0], a[1], a[2], sl] for a, sl in pairs], dtype=np.float64)
    relop = np.ascontiguousarray([oc.RELCODE[a[3]] for a, _ in pairs], dtype=np.int32)
    res = np.zeros((N, 5))
    assert L.qcqpmi_feasible_intervals_batch(0, N, dp(pqrs), relop.ctypes.data_as(IP), dp(res)) == 0
    for i, (a, sl) in enumerate(pairs):
        iv = orc.feasible_intervals(a[0], a[1], a[2], a[3], sl)
        assert len(iv) <= 2, (a, sl, iv)        # one of the two halves of an equality is convex: at most two intersections
        assert int(res[i, 0]) == len(iv), (a, sl, res[i], iv)
        for j, (lo, hi) in enumerate(iv):
            assert res[i, 1 + 2 * j] == lo and res[i, 2 + 2 * j] == hi, (a, sl, res[i], iv)
    print(N, '(atom, slack) pairs')


def device_visits(L, vl, idx, variant):
    cons, nf, xi = np.ascontiguousarray(vl['cons'][idx]), np.ascontiguousarray(vl['nf'][idx].astype(np.int32)), np.ascontiguousarray(vl['xi'][idx])
    N = len(idx)
    x, mv, va, st = np.zeros(N), np.zeros(N, dtype=np.int32), np.zeros(N), np.zeros(N, dtype=np.int32)
    rc = L.qcqpmi_p1_visit_batch(0, variant, N, dp(cons), nf.ctypes.data_as(IP), dp(xi), oc.TOL, oc.VIOL_TOL, SEED, SWEEP, dp(x),
                                 mv.ctypes.data_as(IP), dp(va), st.ctypes.data_as(IP))
    assert rc == 0, L.qcqpmi_last_error(None)
    return dict(x=x, moved=mv, vafter=va, status=st)


@pytest.mark.parametrize('name', sorted(oc.VISIT_VARIANTS))
def test_phase1_visit_on_device_equals_the_oracle(orc, L, name):
    vl = oc.visit_lattice()
    idx = oc.visit_subset(name, vl)
    assert len(idx) >= 300
    got = device_visits(L, vl, idx, oc.VISIT_VARIANTS[name])
    ref = oc.oracle_visits(orc, vl['cons'][idx], vl['nf'][idx], vl['xi'][idx], SEED, SWEEP)
    bad = oc.compare_visits(got, ref, np.arange(len(idx)))
    print(name, len(idx), 'visits,', len(bad), 'mismatches')
    assert len(bad) == 0, [(int(idx[b]), vl['cons'][idx[b], :vl['nf'][idx[b]]].tolist(), vl['xi'][idx[b]], {k: v[b] for k, v in got.items()},
                            {k: v[b] for k, v in ref.items()}) for b in bad[:3]]


def test_variants_that_should_agree_do(L, lattice):
    """Two variants handed the same case give the same bytes: the closed form against the sweep on lists of one (at 1, 2 and 4
    slots), the band visit against the generic visit on band inputs, the fused visits against the band visit."""
    f0, fs, nf, s = lattice
    idx = np.nonzero(nf == 1)[0]
    base = device_onevar(L, lattice, idx, oc.ONEVAR_VARIANTS['sweep1'])
    for name in ('single1', 'single2', 'single4', 'sweep2', 'sweep4'):
        other = device_onevar(L, lattice, idx, oc.ONEVAR_VARIANTS[name])
        for k in ('status', 'x', 'nC'):
            assert base[k].tobytes() == other[k].tobytes(), (name, k)
        assert base['C'][:, :2].tobytes() == other['C'][:, :2].tobytes(), name
    vl = oc.visit_lattice()
    idx = oc.visit_subset('band', vl)
    base = device_visits(L, vl, idx, oc.VISIT_VARIANTS['band'])
    for name in ('core1', 'core4'):
        other = device_visits(L, vl, idx, oc.VISIT_VARIANTS[name])
        for k in base:
            assert base[k].tobytes() == other[k].tobytes(), (name, k)
    idx = oc.visit_subset('band_n2', vl)
    base = device_visits(L, vl, idx, oc.VISIT_VARIANTS['band'])
    for name in ('band_n2', 'band_n2_fasta'):
        other = device_visits(L, vl, idx, oc.VISIT_VARIANTS[name])
        for k in base:
            assert base[k].tobytes() == other[k].tobytes(), (name, k)


# ---------------------------------------------------------------- degenerate coordinate lists through the real kernels
@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


@pytest.mark.parametrize('tag,fam,obj,n', oc.FAMILY_RUNS, ids=[f[0] for f in oc.FAMILY_RUNS])
def test_degenerate_families_through_cd_run(eng_mod, orc, capfd, monkeypatch, tag, fam, obj, n):
    monkeypatch.setenv('QCQPMI_CD_DEBUG', '1')
    funcs = oc.family(fam, n, obj)
    s = dom.shape(funcs)
    want = dom.dispatch(s)
    maxc4 = fam != 'one4'
    assert want.startswith('cd_phase2_kernel MAXC %d XL 1 CL %d ' % (4 if maxc4 else 1, fam != 'mix23')), (tag, want, s)
    seed = 300 + n
    e = dom.engine_for(eng_mod, funcs)
    X0, o, X, lines = dom.run(e, capfd, oc.FAMILY_R, seed, oc.FAMILY_FIRST, oc.FAMILY_ITERS)
    assert e.last_cd_kernel() == 'cd_phase2_kernel', (tag, e.last_cd_kernel())
    e.close()
    dom.check_lines(lines, want, maxc4)
    assert 4 * int(o['ran_phase2'].sum()) >= oc.FAMILY_R
    dom.check_all(orc, funcs, X0, o, X, seed, oc.FAMILY_FIRST, oc.FAMILY_ITERS, (tag,), converges=False)


@pytest.mark.parametrize('tag,fam,n', oc.FAMILY_BATCH, ids=[f[0] for f in oc.FAMILY_BATCH])
def test_degenerate_families_through_cd_batch_run(eng_mod, orc, tag, fam, n):
    fl = oc.batch_family(fam, n)
    o = wb.run(eng_mod, fl, oc.BATCH_R, seed=7, stride=1, fi=oc.BATCH_FIRST, num_iters=oc.FAMILY_ITERS)
    maxc = 1 if fam == 'one4' else 4
    assert o['kernel'] == ('cd_small_kernel<%d,w2>' % maxc if n > 64 else 'cd_small_kernel<%d>' % maxc), (tag, o['kernel'])
    assert 4 * int(o['ran_phase2'].sum()) >= 3 * oc.BATCH_R
    sb.check_vs_oracle(eng_mod, orc, fl, o, oc.BATCH_R, 7, 1, oc.BATCH_FIRST, (tag,), iters=oc.FAMILY_ITERS)



@pytest.mark.parametrize('tag,obj,n,want', oc.FAMILY_STREAM, ids=[s[0] for s in oc.FAMILY_STREAM])
def test_one_constraint_family_through_cd_stream_run(eng_mod, orc, capfd, monkeypatch, tag, obj, n, want):
    monkeypatch.setenv('QCQPMI_L2_DEBUG', '1')
    funcs = oc.family('one4', n, obj)
    assert oc.stream_geometry(dom.shape(funcs)) == want
    seed = 300 + n
    o, X, name, trip = lc.launch(eng_mod, capfd, funcs, 1, oc.FAMILY_R, seed, oc.FAMILY_FIRST, 0, iters=oc.FAMILY_ITERS)
    assert trip == want and name == 'cd_life_kernel<3,%s,classes>' % ('gen' if obj == 'ridge' else 'lin'), (tag, name, trip)
    assert 4 * int(o['ran_phase2'].sum()) >= oc.FAMILY_R
    lc.check_vs_oracle(eng_mod, orc, funcs, o, X, 1, oc.FAMILY_R, seed, oc.FAMILY_FIRST, 0, (tag,), iters=oc.FAMILY_ITERS)
