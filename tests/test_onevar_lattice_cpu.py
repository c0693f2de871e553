"""The one-variable solver on degenerate cases, without a device (tests/onevar_cases.py holds the lattice and says what is in it):
the lattice has the stated shape, judged from the oracle's answers alone; the oracle equals the reference on it (golden g12, MT
draws mirrored); the device headers csrc/onevar.h and csrc/cd_phase1_sep.h, built for the host by tests/host/onevar_selftest.cpp
(-ffp-contract=off, tests/host/hip_stub in place of the HIP runtime header), equal the oracle in keyed mode bit for bit in every
instantiation the kernels run -- status, every piece of the feasible set, the point, keyed draws included; x_i, moved, vafter and
status for the phase-1 visits.  tests/test_gpu_onevar_lattice.py repeats the last part on the device."""
import collections
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import load_golden
import onevar_cases as oc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, SWEEP = 123, 3


@pytest.fixture(scope='module')
def lattice():
    return oc.onevar_arrays()


@pytest.fixture(scope='module')
def mt(orc, lattice):
    return oc.oracle_onevar(orc, *lattice, mode=orc.RNG_MT)


def test_lattice_has_its_stated_shape(orc, lattice, mt):
    """Cell counts from the oracle's answers alone (a draw is told by the MT stream's position): every cell below holds >= 30 cases
    at each list length at which it can occur."""
    f0, fs, nf, s = lattice
    N = len(nf)
    assert 8000 <= N <= 16000
    zero = (f0[:, 0] == 0.) & (f0[:, 1] == 0.)
    st = mt['status']
    kind = np.where(st == 0, 'none', np.where(st == -1, 'raise-1', np.where(st < 0, 'other', np.where(zero, 'zero', np.where(mt['draws'] > 0, 'tie', 'point')))))
    cells = collections.Counter(zip(kind.tolist(), nf.tolist()))
    pieces = collections.Counter(zip(mt['nC'].tolist(), nf.tolist()))
    print('cases', N, 'cells', sorted(cells.items()), 'pieces', sorted(pieces.items()))
    for k in ('none', 'raise-1', 'point', 'tie', 'zero'):
        for length in (1, 2, 3, 4):
            assert cells[(k, length)] >= 30, (k, length, cells[(k, length)])
    # status -2 is unreachable through onevar_qcqp (see onevar_cases): the oracle never returns it, nor anything else
    assert not np.any(kind == 'other')
    for length in (1, 2, 3, 4):
        for npieces in range(1, min(length, 4) + 1):
            assert pieces[(npieces, length)] >= 30, (npieces, length, pieces[(npieces, length)])
    assert np.sum(st == 0) <= N // 2
    # two different constraints of the list contribute an equal finite end point
    ends = {}
    for a in range(len(oc.ATOMS)):
        for k, sl in enumerate(oc.SLACKS):
            iv = orc.feasible_intervals(*oc.ATOMS[a], s=sl)
            ends[(a, k)] = frozenset(v for pair in iv for v in pair if np.isfinite(v))
    lat = oc.onevar_lattice()
    shared = 0
    for i in range(N):
        sets = [ends[(int(a), int(lat['slack'][i]))] for a in lat['atom'][i, :nf[i]]]
        shared += any(sets[a] & sets[b] for a in range(len(sets)) for b in range(a))
    print('cases with an end point shared by two constraints:', shared)
    assert shared >= 1000


def test_oracle_equals_reference(lattice, mt):
    """Golden g12: the reference's onevar_qcqp on the lattice, numpy seeded with the case index.  The oracle in MT mode gives the
    same answer in every case -- None / raise / the point itself, drawn points included, and the number of words drawn -- and the
    tables of onevar_cases reproduce the inputs the golden was recorded on (indices, length and checksum of the coefficients)."""
    z = load_golden('g12_onevar_lattice')
    lat = oc.onevar_lattice()
    for k in ('obj', 'atom', 'slack'):
        assert z[k].dtype == np.int16 and np.array_equal(z[k], lat[k]), k
    assert oc.checksum(*lattice) == (int(z['nbytes']), int(z['crc']))
    err, isnone = z['err'].astype(bool), z['isnone'].astype(bool)
    assert np.array_equal(mt['status'] < 0, err)
    assert np.array_equal(mt['status'] == 0, isnone)
    pt = ~err & ~isnone
    assert np.array_equal(mt['x'][pt], z['x'][pt])
    assert np.array_equal(mt['draws'][~err], z['draws'][~err].astype(np.int64))
    assert np.sum(pt & (z['draws'] > 0)) >= 1000          # drawn points are compared, not only classified


# ---------------------------------------------------------------- the headers on the host
@pytest.fixture(scope='module')
def cxx():
    c = os.environ.get('CXX') or shutil.which('g++') or shutil.which('clang++')
    if not c:
        pytest.skip('no host compiler')
    return c


def build(cxx, tmp, extra=(), name='onevar_selftest'):
    exe = str(tmp / name)
    p = subprocess.run([cxx, '-std=c++17', '-O2', '-ffp-contract=off', '-I' + os.path.join(REPO, 'tests', 'host', 'hip_stub'),
                        '-I' + os.path.join(REPO, 'qcqp_amd', 'csrc'), '-o', exe, os.path.join(REPO, 'tests', 'host', 'onevar_selftest.cpp')]
                       + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return exe if p.returncode == 0 else None, p.stdout.decode()


def run_onevar(exe, tmp, name, lattice, idx, env=None):
    f0, fs, nf, s = lattice
    fin, fout = str(tmp / (name + '.in')), str(tmp / (name + '.out'))
    with open(fin, 'wb') as f:
        f.write(np.int64(len(idx)).tobytes())
        for a in (f0[idx], fs[idx], s[idx], nf[idx].astype(np.int32)):
            f.write(np.ascontiguousarray(a).tobytes())
        f.write(np.uint64(SEED).tobytes())
    r = subprocess.run([exe, 'onevar', str(oc.ONEVAR_VARIANTS[name]), fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
    assert r.returncode == 0, r.stdout.decode()
    out = np.fromfile(fout).reshape(len(idx), 13)
    return dict(status=out[:, 0].astype(np.int32), x=out[:, 1], nC=out[:, 2].astype(np.int32), C=out[:, 3:].reshape(-1, 5, 2))


def run_visits(exe, tmp, name, vl, idx, env=None):
    fin, fout = str(tmp / (name + '.in')), str(tmp / (name + '.out'))
    with open(fin, 'wb') as f:
        f.write(np.int64(len(idx)).tobytes())
        for a in (vl['cons'][idx], vl['xi'][idx], vl['nf'][idx].astype(np.int32)):
            f.write(np.ascontiguousarray(a).tobytes())
        f.write(np.float64(oc.TOL).tobytes() + np.float64(oc.VIOL_TOL).tobytes() + np.uint64(SEED).tobytes() + np.int64(SWEEP).tobytes())
    r = subprocess.run([exe, 'visit', str(oc.VISIT_VARIANTS[name]), fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
    assert r.returncode == 0, r.stdout.decode()
    out = np.fromfile(fout).reshape(len(idx), 4)
    return dict(x=out[:, 0], moved=out[:, 1].astype(np.int32), vafter=out[:, 2], status=out[:, 3].astype(np.int32))


@pytest.fixture(scope='module')
def exe(cxx, tmp_path_factory):
    e, log = build(cxx, tmp_path_factory.mktemp('onevar_host'))
    assert e, log
    return e


def keyed_subset(orc, lattice, idx):
    """The oracle in keyed mode on a subset: the unit operators key a draw by the case's position in the call."""
    f0, fs, nf, s = lattice
    return oc.oracle_onevar(orc, f0[idx], fs[idx], nf[idx], s[idx], mode=orc.RNG_KEYED, seed=SEED)


@pytest.mark.parametrize('name', sorted(oc.ONEVAR_VARIANTS))
def test_host_build_of_the_set_builder_and_minimiser_equals_the_oracle(orc, exe, tmp_path, lattice, name):
    f0, fs, nf, s = lattice
    idx = oc.onevar_subset(name, nf)
    assert len(idx) >= 1000
    got = run_onevar(exe, tmp_path, name, lattice, idx)
    ref = keyed_subset(orc, lattice, idx)
    bad = oc.compare_onevar(got, ref, np.arange(len(idx)), oc.ONEVAR_MAXC[name])
    print(name, len(idx), 'cases,', len(bad), 'mismatches')
    assert len(bad) == 0, [(oc.describe_onevar(idx[b], f0, fs, nf, s), {k: v[b] for k, v in got.items()}, {k: v[b] for k, v in ref.items()}) for b in bad[:3]]


@pytest.fixture(scope='module')
def visit_ref(orc):
    vl = oc.visit_lattice()
    return {name: (idx, oc.oracle_visits(orc, vl['cons'][idx], vl['nf'][idx], vl['xi'][idx], SEED, SWEEP))
            for name, idx in ((n, oc.visit_subset(n, vl)) for n in oc.VISIT_VARIANTS)}


def test_visit_lattice_has_its_stated_shape(visit_ref):
    vl = oc.visit_lattice()
    idx, ref = visit_ref['core4']
    assert not np.any((vl['cons'][:, :, 0] == 0.) & (vl['cons'][:, :, 1] == 0.) & (np.arange(4)[None, :] < vl['nf'][:, None]))
    band = np.arange(len(idx)) < vl['nband']
    print('visits', len(idx), 'band', vl['nband'], 'moved', int(ref['moved'].sum()), 'raise', int(np.sum(ref['status'] < 0)))
    assert vl['nband'] >= 700 and len(idx) - vl['nband'] == 2400
    assert np.sum(ref['moved'][band] == 1) >= 200 and np.sum(ref['moved'][band] == 0) >= 200
    for k in (1, 2, 3, 4):
        sel = ~band & (vl['nf'] == k)
        assert np.sum(ref['moved'][sel] == 1) >= 30 and np.sum((ref['status'][sel] == 0) & (ref['moved'][sel] == 0)) >= 30, k
    assert np.sum(ref['status'] < 0) >= 40        # the unbounded-set status (a list whose first atom is unbounded, where it is violated)
    assert len(visit_ref['band_n2'][0]) >= 300 and len(visit_ref['band_n2'][0]) < len(visit_ref['band'][0])
    # the targeted x_i do what the docstring of onevar_cases says: the bisection (qcqp.py:122-131 for the band class: slack s is
    # achievable iff the discriminant test holds, replayed here) takes a midpoint within the fused visits' guard 1e-9 (1 - r) of 0,
    # for r = -1 and for the two values of r just below -1e-3 -- the branch of p1_band_visit / p1_band_visit_n that forms the
    # reference's discriminants
    hits = collections.Counter()
    for i in range(vl['nband']):
        p, _, r, _ = vl['cons'][i, 0]
        if not r < -1e-3:
            continue
        x = vl['xi'][i]
        ss, es, guard = -oc.TOL, abs(x * (p * x + 0.) + r) - oc.VIOL_TOL, 1e-9 * (1. - r)
        near = False
        while es - ss > oc.TOL:
            s = (ss + es) / 2.
            near = near or not abs(s) > guard
            D1, D2 = 0. - 4. * p * (r - s), 0. - 4. * (-p) * (-r - s)
            if D1 > 0. and (D2 < 0. or D2 < D1):
                es = s
            else:
                ss = s
        hits[float(r)] += near
    print('visits with a midpoint inside the guard, by r:', sorted(hits.items()))
    for r in (-1., -2e-3, float(np.nextafter(-1e-3, -1.))):
        assert hits[r] >= 10, (r, hits)


@pytest.mark.parametrize('name', sorted(oc.VISIT_VARIANTS))
def test_host_build_of_the_phase1_visit_equals_the_oracle(exe, tmp_path, visit_ref, name):
    vl = oc.visit_lattice()
    idx, ref = visit_ref[name]
    got = run_visits(exe, tmp_path, name, vl, idx)
    bad = oc.compare_visits(got, ref, np.arange(len(idx)))
    print(name, len(idx), 'visits,', len(bad), 'mismatches')
    assert len(bad) == 0, [(int(idx[b]), vl['cons'][idx[b], :vl['nf'][idx[b]]].tolist(), vl['xi'][idx[b]], {k: v[b] for k, v in got.items()},
                            {k: v[b] for k, v in ref.items()}) for b in bad[:3]]


def test_host_variants_that_should_agree_do(exe, tmp_path):
    """The band visit against the generic visit on band inputs, and the fused visits against the band visit: the same bytes in
    every output, the same cases at the same positions."""
    vl = oc.visit_lattice()
    for names in (('band', 'core1', 'core4'), ('band', 'band_n2', 'band_n2_fasta')):
        idx = oc.visit_subset(names[-1] if 'band_n2' in names else 'band', vl)
        base = run_visits(exe, tmp_path, names[0], vl, idx)
        for name in names[1:]:
            other = run_visits(exe, tmp_path, name, vl, idx)
            for k in base:
                assert base[k].tobytes() == other[k].tobytes(), (name, k)


def test_host_build_under_sanitizers(orc, cxx, tmp_path, lattice, visit_ref):
    """The same stand-alone program with -fsanitize=address,undefined (where the host compiler has the runtimes): every variant
    runs clean over the whole lattice and still equals the oracle."""
    e, log = build(cxx, tmp_path, ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], name='onevar_selftest_san')
    if not e:
        pytest.skip('host compiler without the sanitizer runtimes: ' + log[-200:])
    f0, fs, nf, s = lattice
    for name in sorted(oc.ONEVAR_VARIANTS):
        idx = oc.onevar_subset(name, nf)
        got = run_onevar(e, tmp_path, name, lattice, idx)
        assert len(oc.compare_onevar(got, keyed_subset(orc, lattice, idx), np.arange(len(idx)), oc.ONEVAR_MAXC[name])) == 0, name
    vl = oc.visit_lattice()
    for name in sorted(oc.VISIT_VARIANTS):
        idx, ref = visit_ref[name]
        assert len(oc.compare_visits(run_visits(e, tmp_path, name, vl, idx), ref, np.arange(len(idx)))) == 0, name


# ---------------------------------------------------------------- the degenerate families under the oracle alone
def _family_jobs():
    for tag, fam, obj, n in oc.FAMILY_RUNS:
        yield tag, (lambda fam=fam, obj=obj, n=n: oc.family(fam, n, obj)), 300 + n, oc.FAMILY_R, oc.FAMILY_FIRST
    for tag, obj, n, _ in oc.FAMILY_STREAM:
        yield tag + '-stream', (lambda obj=obj, n=n: oc.family('one4', n, obj)), 300 + n, oc.FAMILY_R, oc.FAMILY_FIRST
    for tag, fam, n in oc.FAMILY_BATCH:
        for b in range(3):
            yield '%s-batch-%d' % (tag, b), (lambda fam=fam, n=n, b=b: oc.batch_family(fam, n)[b]), 7 + b, oc.BATCH_R, oc.BATCH_FIRST


JOBS = list(_family_jobs())


@pytest.mark.parametrize('job', JOBS, ids=[j[0] for j in JOBS])
def test_family_does_not_degenerate_into_nothing_happened(orc, job):
    """Every workload of part 6 of tests/test_gpu_onevar_lattice.py under the oracle alone (keyed draws, num_iters = 40): every
    restart finishes phase 1 without a raise, at least a quarter of them reach phase 2, and phase 2 accepts moves."""
    tag, make_funcs, seed, R, first = job
    prob = orc.Problem(make_funcs())
    X0 = orc.keyed_normal_matrix(seed, prob.n, R, first_index=first)
    reached = 0
    for r in range(R):
        rng = orc.Rng(orc.RNG_KEYED, seed)
        rng.set_restart(first + r)
        x, s1, s2 = prob.improve_cd_sep(X0[:, r], num_iters=oc.FAMILY_ITERS, rng=rng)      # raises where the reference would
        reached += s2[0] > 0 and s2[2] > 0
    assert 4 * reached >= R, (tag, reached, R)


def test_stream_plan_takes_the_one_constraint_family_and_no_other():
    """What cd_life2_config (csrc/cd_life_plan.h) reads of a problem, for the families of part 6: the lifecycle kernel takes at most
    two constraints per coordinate and four classes, so one4 is inside (several classes: the GENK kind on a positive diagonal, LINK
    on a zero one) and mix7 / mix23 (three constraints on a coordinate, 7 and more classes) are refused."""
    import test_gpu_cd_run_domain as dom
    for tag, obj, n, want in oc.FAMILY_STREAM:
        s = dom.shape(oc.family('one4', n, obj))
        assert (s['maxc'], s['Kreal'], s['objclass']) == (1, 4, 1 if obj == 'ridge' else 2), (tag, s)
        assert oc.stream_geometry(s) == want, (tag, s)
    for fam in ('mix7', 'mix23'):
        s = dom.shape(oc.family(fam, 48))
        assert s['maxc'] == 3 and s['Kreal'] > 4 and oc.stream_geometry(s) is None, (fam, s)
