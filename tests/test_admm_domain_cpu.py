"""Host-side checks of tests/admm_domain_cases.py, the reference and the case tables tests/test_gpu_admm_domain.py relies on:
the longdouble tier against exact rational arithmetic, the basis form against the oracle's onecons (golden G5 and the section-A
families), both float64 summation orders inside the derived bound with equal decisions on every case, the margins that make the
decisions robust, and the coverage of the dispatch domain by the case tables.  Needs no GPU."""
import numpy as np
import pytest

import admm_domain_cases as ac
from conftest import load_golden, RELSTR

LD = ac.LD


# ---------------------------------------------------------------------------------- the yardstick itself
@pytest.mark.parametrize('rows', [1, 2, 4, 8, 9])
def test_longdouble_tier_against_exact_rational_arithmetic(rows):
    """Every spectrum a size admits, three points each: the same decisions as the search whose phi is evaluated in
    fractions.Fraction, the same multiplier, xhat within the longdouble rounding bound of the exact one."""
    kinds = ('zero', 'onepos', 'oneneg', 'both', 'qzero', 'feasible', 'both_le')
    worst, pairs = 0.0, 0
    for t, kind in enumerate(kinds):
        if rows == 1 and kind in ('both_le',):
            continue
        rs = np.random.RandomState(100 * rows + t)
        lam, qhat, relop, rmode = ac.spectrum(kind, rows, rs, (2, 64))
        V = rs.randn(rows, 3) * 2.0
        r = ac.pick_r(rmode, lam, qhat, V, rs)
        slo, ehi = ac.brackets(lam[None])
        for c in range(3):
            a = ac.onecons_basis(lam, qhat, r, relop, slo[0], ehi[0], V[:, c], tier='ld')
            b = ac.onecons_basis(lam, qhat, r, relop, slo[0], ehi[0], V[:, c], exact=True)
            assert a.decisions == b.decisions and a.nu == b.nu, (kind, c)
            xe = np.array([LD(x.numerator) / LD(x.denominator) for x in b.xhat])
            bound = ac.xhat_bound(lam, qhat, V[:, c], a.nu, feasible=a.feasible, yardstick=True) + 2 * ac.ULD * np.abs(xe).astype(float)
            err = np.abs(a.xhat - xe).astype(float)
            assert np.all(err <= bound), (kind, c, err, bound)      # (+ 2 ulp: the exact quotient itself is rounded to longdouble here)
            if not a.feasible:
                worst = max(worst, float(np.max(err / bound)))
            pairs += 1
    print('\nlongdouble tier against exact arithmetic, rows = %d: %d pairs, worst error / bound %.3f' % (rows, pairs, worst))


def test_sums_in_kernel_order():
    """_sum_kernel against a literal replay of wave_sum (row_shr 1, 2, 4, 8, row_bcast 15, 31) and of the four-wave LDS sum."""
    rs = np.random.RandomState(3)
    for stride, rows in ((64, 130), (256, 8193), (64, 4096)):
        x = rs.randn(rows) * 10.0 ** rs.uniform(-3, 3, size=rows)
        epl = -(-rows // stride)
        pad = np.zeros(epl * stride); pad[:rows] = x
        lanes = np.zeros(stride)
        for e in range(epl):
            lanes = lanes + pad[e * stride:(e + 1) * stride]
        tot = []
        for w in range(stride // 64):
            v = lanes[64 * w:64 * w + 64].copy()
            for sh in (1, 2, 4, 8):                        # row_shr inside rows of 16 lanes: lanes without a source add 0
                src = np.zeros(64)
                for l in range(64):
                    if (l % 16) >= sh:
                        src[l] = v[l - sh]
                v = v + src
            for last, rows_to in ((15, (1, 3)), (31, (2, 3))):
                src = np.zeros(64)
                for rw in rows_to:
                    src[16 * rw:16 * rw + 16] = v[16 * (rw - 1) + 15] if last == 15 else v[31]
                v = v + src
            tot.append(v[63])
        t = tot[0]
        for w in tot[1:]:
            t = t + w
        assert ac._sum_kernel(x, stride) == t


# ---------------------------------------------------------------------------------- the basis form is onecons_qcqp
def test_basis_form_on_golden_g5(orc):
    z = load_golden('g5_onecons')
    N, n = z['P'].shape[0], z['P'].shape[1]
    worst = 0.0
    for i in range(N):
        lam, Q = z['lmb'][i], z['Q'][i]
        relop = RELSTR[int(z['relop'][i])]
        slo, ehi = ac.brackets(lam[None])
        qh = ac.qhat_like_set_eig(Q, z['q'][i])
        sv = ac.onecons_basis(lam, qh, float(z['r'][i]), relop, slo[0], ehi[0], Q.T.dot(z['z'][i]), tier='seq')
        x = z['z'][i] if sv.feasible else Q.dot(np.asarray(sv.xhat, dtype=np.float64))
        d = np.max(np.abs(x - z['x'][i]))
        worst = max(worst, d)
        assert sv.feasible == bool(z['early'][i]) or not np.any(z['P'][i]), i
        assert d < 1e-9 * (1 + np.max(np.abs(z['x'][i]))), (i, d)
        prob = orc.Problem([(np.eye(n), np.zeros(n), 0., None), (z['P'][i], z['q'][i], float(z['r'][i]), relop)])
        xo, _ = prob.onecons(1, z['z'][i], lam, Q)
        assert np.max(np.abs(x - xo)) < 1e-9 * (1 + np.max(np.abs(xo))), i
    print('\nbasis form against golden G5: %d cases, worst |dx| %.2e' % (N, worst))


@pytest.mark.parametrize('rows', [70, 100, 130])
def test_basis_form_on_section_a_families_against_the_oracle(orc, rows):
    """The section-A generators at small n, every spectrum: the oracle's onecons on (P_k, q_k, r_k) with the eigenpairs
    (lam_k, B_k') is a float64 evaluation of the same search: same point within the derived bound."""
    worst = 0.0
    for g, kinds in enumerate(ac._groups(3, 128)):
        case = ac.ACase(rows, kinds, False, 50 * rows + g).build()
        prob = orc.Problem(case.funcs())
        B = case.basis()
        for k in range(case.m):
            ref = case.reference(k)
            Qk = np.ascontiguousarray(B[k].T)
            for c in range(case.R):
                xo, _ = prob.onecons(k + 1, case.Z[:, c], case.lam[k], Qk)
                err = np.abs(np.asarray(xo, dtype=LD) - ref['x'][:, c]).astype(float)
                bd = ref['bound'][:, c]
                assert np.all(err[bd == 0] == 0) and np.all(err <= bd), (case.id, k, c)
                if (bd > 0).any():
                    worst = max(worst, float(np.max(err[bd > 0] / bd[bd > 0])))
    print('\noracle onecons against the basis form, rows = %d: worst error / bound %.3f' % (rows, worst))


# ---------------------------------------------------------------------------------- float64 orders, margins
@pytest.mark.parametrize('case', ac.A_CASES, ids=lambda c: c.id)
def test_float64_orders_inside_the_bound_with_equal_decisions(case):
    """Sequential and kernel-order float64 evaluations of every pair of every section-A case: the decisions of the longdouble
    tier, xhat within the bound; the smallest |phi| / scale met is >= 1e3 u and the cancellation factor <= 1e6."""
    case.build()
    worst = 0.0
    for k in range(case.m):
        ref = case.reference(k)
        assert ref['margin'] >= ac.MARGIN_MIN, (case.id, k, ref['margin'])
        assert ref['cancel'] <= ac.CANCEL_MAX, (case.id, k, ref['cancel'])
        for c in range(case.R):
            sl = case.solve(k, c, 'ld')
            ex = ac.xhat_bound(case.lam[k], case.qhat[k], case.V[k][:, c], sl.nu, case.e_v(k, c), sl.feasible)
            for tier in ('seq', 'kernel'):
                sv = case.solve(k, c, tier)
                assert sv.decisions == sl.decisions and sv.nu == sl.nu, (case.id, k, c, tier)
                err = np.abs(np.asarray(sv.xhat, dtype=LD) - sl.xhat).astype(float)
                assert np.all(err <= ex), (case.id, k, c, tier)
                if (ex > 0).any():
                    worst = max(worst, float(np.max(err[ex > 0] / ex[ex > 0])))
    print('\n%s: float64 tiers worst error / bound %.3f' % (case.id, worst))


@pytest.mark.parametrize('case', ac.C_CASES, ids=lambda c: c.id)
def test_section_c_decisions_are_robust(case):
    """Every projection of every section-C run, replayed on the host in the device's basis: equal decisions in the three tiers,
    float64 inside the bound, margin >= 1e3 u, cancellation factor <= 1e6."""
    st = ac.c_margins(case.build())
    print('\n%s: %d projections, smallest margin %.1e, largest cancellation factor %.1e, float64 worst error / bound %.3f' % (
        case.id, st['calls'], st['margin'], st['cancel'], st['worst']))
    assert st['calls'] > 0 and st['margin'] >= ac.MARGIN_MIN and st['cancel'] <= ac.CANCEL_MAX, st


def test_inverse_yardstick_against_exact_rational_arithmetic():
    import fractions
    rs = np.random.RandomState(2)
    n = 7
    A = rs.randn(n, n)
    M = A.T.dot(A) + 0.5 * np.eye(n)
    X, _ = ac.inverse_yardstick(M)
    Mf = [[fractions.Fraction(float(v)) for v in row] for row in M]
    for j in range(n):                                     # M x = e_j by Gaussian elimination in fractions
        aug = [row[:] + [fractions.Fraction(int(i == j))] for i, row in enumerate(Mf)]
        for c in range(n):
            p = next(i for i in range(c, n) if aug[i][c] != 0)
            aug[c], aug[p] = aug[p], aug[c]
            for i in range(n):
                if i != c:
                    f = aug[i][c] / aug[c][c]
                    aug[i] = [a - f * b for a, b in zip(aug[i], aug[c])]
        for i in range(n):
            x = aug[i][n] / aug[i][i]
            xl = LD(x.numerator) / LD(x.denominator)
            assert abs(X[i, j] - xl) <= 4 * ac.ULD * abs(xl), (i, j)


@pytest.mark.parametrize('n', ac.A_EIG_NS)
def test_real_eigenpairs_margins(n):
    funcs, lm, Q, Z = ac.eig_problem(n)
    for k in range(len(funcs) - 1):
        ref = ac.eig_reference(funcs, lm, Q, Z, k)
        assert ref['margin'] >= ac.MARGIN_MIN and ref['cancel'] <= ac.CANCEL_MAX, (n, k, ref['margin'], ref['cancel'])


def test_gemm_checker_accepts_float64_products_and_refuses_mutants():
    """Section B's checker on the host: NumPy's own product passes; one k-block of the second product dropped, or the rows of two
    row blocks swapped, does not."""
    n, m, R = ac.B_CASES[1]
    _, Q, Z = ac.gemm_problem(n, m, R)
    Qk, cols = Q[0], ac.sample_columns(R)
    good = Qk.dot(Qk.T.dot(Z))
    assert max(ac.gemm_check(good, Qk, Z, cols)) <= 1.0
    hat = Qk.T.dot(Z)
    hat[16:32] = 0.0
    swapped = good.copy()
    swapped[0:16], swapped[16:32] = good[16:32], good[0:16]
    for bad in (Qk.dot(hat), swapped):
        assert min(ac.gemm_check(bad, Qk, Z, cols)) > 1.0


# ---------------------------------------------------------------------------------- the tables cover the dispatch domain
def test_expected_instantiations_against_the_restated_launch_conditions():
    small = {1: 'small<1>', 2: 'small<2>', 4: 'small<4>', 8: 'small<8>'}
    for rows in range(1, 20000, 1):
        for lowrank in (True, False):
            name = ac.secular_instantiation(rows, lowrank)
            if lowrank and rows <= 8:
                assert name == small.get(rows)
                continue
            want = ('wave<2,1>' if rows <= 128 else 'wave<4,1>' if rows <= 256 else 'wave<8,1>' if rows <= 512 else 'wave<16,1>' if rows <= 1024
                    else 'wave<32,1>' if rows <= 2048 else 'wave<64,1>' if rows <= 4096 else 'wave<32,4>' if rows <= 8192
                    else 'wave<64,4>' if rows <= 16384 else None)
            assert name == want, (rows, lowrank)
            if name:                                       # the slots of a lane hold every row
                epl, stride = ac.wave_geometry(rows, lowrank)
                assert epl * stride >= rows and epl <= 64
    table = {1: 'small<1>', 2: 'small<2>', 4: 'small<4>', 8: 'small<8>', 9: 'wave<2,1>', 128: 'wave<2,1>', 129: 'wave<4,1>', 256: 'wave<4,1>',
             257: 'wave<8,1>', 512: 'wave<8,1>', 513: 'wave<16,1>', 1024: 'wave<16,1>', 1025: 'wave<32,1>', 2048: 'wave<32,1>',
             2049: 'wave<64,1>', 4096: 'wave<64,1>', 4097: 'wave<32,4>', 8192: 'wave<32,4>', 8193: 'wave<64,4>'}
    for case in ac.A_CASES:
        assert case.expected == table[case.rows], case.id
        assert case.R == 17 and case.m == (3 if case.rows <= 1025 else 2 if case.rows <= 4097 else 1)
    assert sorted(set(c.rows for c in ac.A_CASES)) == sorted(table)


def test_every_branch_and_every_switch_has_a_case():
    reached = set(c.expected for c in ac.A_CASES)
    assert reached == set(ac.ALL_SECULAR), set(ac.ALL_SECULAR) - reached       # all 12 branches of admm_launch_secular
    rows = set(c.rows for c in ac.A_CASES)
    for lo, hi in ac.A_SWITCHES:
        assert lo in rows and hi in rows
        assert ac.secular_instantiation(lo, True) != ac.secular_instantiation(hi, True)
    assert ac.secular_instantiation(8, True) != ac.secular_instantiation(9, True)
    # the lowrank && rows > 8 combination (every permutation case and dense9) and the full basis (set_eig, section B, section C)
    assert any(c.rows > 8 and c.lowrank for c in ac.A_CASES)
    assert all(ac.secular_instantiation(n, False).startswith('wave') for n in ac.A_EIG_NS)
    # every spectrum with every wave instantiation it is defined for; the slots e >= 32 of both EPL = 64 kernels
    for name in ac.ALL_SECULAR:
        kinds = set(k for c in ac.A_CASES if c.expected == name for k in c.kinds)
        assert {'both'} <= kinds, name
        if name.startswith('wave') and name != 'wave<2,1>':
            assert {'hi'} <= kinds, name
    for rows in (2049, 4096, 8193):
        assert any(c.rows == rows and 'hi' in c.kinds for c in ac.A_CASES)
        epl, stride = ac.wave_geometry(rows, True)
        assert epl == 64 and rows > 32 * stride
    assert set(k for c in ac.A_CASES for k in c.kinds) == set(ac.SPECTRA)
    relops = set()
    for c in ac.A_CASES[:12]:
        relops |= set(c.build().relop)
    assert relops == {'<=', '=='}


def test_both_gemm_kernels_and_split_planes_are_reached():
    seen1, seen2 = set(), set()
    for n, m, R in ac.B_CASES:
        g = ac.geometry(n, m, n, False, R)
        seen1.add(g['gemm1']); seen2.add(g['gemm2'])
    assert seen1 == seen2 == {'gemm_pk_small_kernel', 'gemm_pk_kernel'}
    # the shapes the issue names, and the derived one
    g = ac.geometry(256, 1, 256, False, 16384)
    assert g['gemm1'] == g['gemm2'] == 'gemm_pk_kernel'
    assert ac.geometry(256, 1, 256, False, 16384 - 128)['gemm1'] == 'gemm_pk_small_kernel'    # one group of 8 tiles fewer: 254 workgroups
    assert ac.geometry(128, 1, 128, False, 16384)['gemm1'] == 'gemm_pk_small_kernel'          # one group of 8 row blocks: 128 workgroups
    n, m, R = ac.B_FIRST_ONLY
    g = ac.geometry(n, m, n, False, R)
    assert (g['gemm1'], g['gemm2']) == ('gemm_pk_kernel', 'gemm_pk_small_kernel') and n % 16 != 0
    assert ac.geometry(n, m, n, False, R - 16)['gemm1'] == 'gemm_pk_small_kernel'             # R sits just above the switch
    ragged = [(n, m, R) for n, m, R in ac.B_CASES if n % 16 and (ac.n16_of(m * n) // 16) % 4 and ((R + 15) // 16) % 4]
    assert any(ac.geometry(n, m, n, False, R)['gemm1'] == 'gemm_pk_kernel' for n, m, R in ragged)
    assert any(ac.geometry(n, m, n, False, R)['gemm1'] == 'gemm_pk_small_kernel' for n, m, R in ragged)
    assert any(R == 1 for _, _, R in ac.B_CASES)
    # section C: split planes 1 and 2 of both products, both violation reductions of the small kernel, the wave kernel, unit bases
    geo = [c.geometry() for c in ac.C_CASES]
    assert set(g['run_zs1'] for g in geo) == {1, 2} and set(g['run_zs2'] for g in geo) == {1, 2}
    assert set(g['viol_reduction'] for g in geo) == {'lds', 'atomic', 'wave'}
    by = dict((c.id, c) for c in ac.C_CASES)
    assert by['n272-zs1'].geometry()['run_zs1'] == 2 and by['n272-zs1'].geometry()['KBn'] == 17      # 17 k-blocks: planes of 8 and 9
    assert by['m32-rp8-zs2'].geometry()['run_zs2'] == 2 and by['full-n48-m6-zs2'].geometry()['run_zs2'] == 2
    assert set(c.rp for c in ac.C_CASES if c.basis == 'reduced') >= {2, 4, 8, 9}
    assert set(c.m for c in ac.C_CASES) >= {15, 16, 17} and set(c.R for c in ac.C_CASES) >= {1, 15, 17, 33}
    assert set(c.basis for c in ac.C_CASES) == {'reduced', 'full', 'unit'}
    assert set((c.p0, c.solver) for c in ac.C_CASES) >= {('diag', 'diag'), ('dense', 'host'), ('dense', 'device')}
    assert set(c.debug for c in ac.C_CASES) >= {0, 2, 4}
    assert ac.gemm_zsplit(2, 2, 17) == 2 and ac.gemm_zsplit(2, 2, 15) == 1 and ac.gemm_zsplit(1, 1, 400) == 16
