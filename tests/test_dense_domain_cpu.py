"""Host-side checks of what tests/test_gpu_dense_domain.py relies on (tests/dense_domain_cases.py): the geometry table of
dense_chain_mw_kernel against mw_geometry, the placement of the '==' constraints in the slots of both chain kernels, the
oracle's walks (they move), and the gap / segment counts of the hand-built problems that fill the kernel's lists.  No GPU."""
import numpy as np
import pytest

import dense_domain_cases as dc


@pytest.fixture(scope='module')
def L():
    from qcqp_amd import _ffi
    return _ffi.lib()


def test_geometry_table_is_mw_geometry(L):
    """The table the GPU test documents its cases with is what mw_geometry returns; the grid of section A hits every slot
    count 1..8, all four template instantiations, and both placements of the serial thread (a free lane of the last wave, an
    extra wave); one constraint more than 3584 leaves the multi-wave kernel."""
    assert set(dc.GEOMETRY) == set(dc.A_GRID)
    for m, g in dc.GEOMETRY.items():
        assert dc.geometry(L, m) == g, (m, dc.geometry(L, m), g)
    gs = [dc.GEOMETRY[m] for m in dc.A_GRID]
    assert {g[0] for g in gs} == set(range(1, 9))
    assert {dc.template_of(g[0]) for g in gs} == {1, 2, 4, 8}
    assert {dc.template_of(dc.GEOMETRY[m][0]) for m in (897, 1793, 2241, 2689)} == {4, 8}      # instantiations with empty slots
    assert any(g[2] < g[1] for g in gs) and any(g[2] == g[1] for g in gs)
    for m in (63, 449, 511):
        assert dc.GEOMETRY[m][2] == m and dc.GEOMETRY[m][3] == 64 * (m // 64 + 1)             # free lane: no extra wave
    for m in (64, 448, 512):
        assert dc.GEOMETRY[m][2] == dc.GEOMETRY[m][1] and dc.GEOMETRY[m][3] == dc.GEOMETRY[m][1] + 64
    for m in dc.C_GRID:
        assert dc.geometry(L, m)[0] > 8
    assert dc.geometry(L, 3585)[0] == 9
    for m, n, R in dc.B_CASES:
        assert dc.geometry(L, m)[0] <= 8


def test_lds_limit_of_the_one_wave_kernel():
    """(DN_FARR_MIN m1p + DN_LDS_WAVE) doubles per wave in 160 KB: m1p = 5056, 79 slots per lane."""
    m = dc.largest_m_one_wave()
    assert m == 5055 and m == max(dc.C_GRID)
    assert (dc.DN_FARR_MIN * (m + 1) + dc.DN_LDS_WAVE) * 8 <= dc.LDS_BYTES
    assert (dc.DN_FARR_MIN * (m + 1 + 64) + dc.DN_LDS_WAVE) * 8 > dc.LDS_BYTES
    assert (m + 1) // 64 == 79


def test_equalities_sit_in_every_slot(L):
    """dense_mixed: '==' in the first and the last-but-one constraint and in every slot j >= 1 of dense_chain_mw_kernel
    (slot (k - 1) // Tc) and of dense_chain_kernel (slot k // 64); beyond m + 1 = 2048 the one-wave kernel holds equalities in
    slots >= 32."""
    ms = sorted({m for m in dc.A_GRID if m > 2} | {m for m, _, _ in dc.B_CASES} | set(dc.C_GRID) | set(dc.E_MS))
    for m in ms:
        top = dc.check_relop_placement(m, dc.equality_indices(m), dc.geometry(L, m))
        if m + 1 > 2048 and m != 2048:      # m = 2048: slot 32 holds the ball alone
            assert top >= 32, (m, top)
    for m in (63, 65, 600):                 # the family carries exactly that pattern, the rest stays '<='
        funcs = dc.family(3, m)
        assert dc.equalities(funcs) == dc.equality_indices(m)
        assert all(funcs[k][3] == '<=' for k in range(1, m + 1) if k not in set(dc.equality_indices(m)))
    for m in (1, 2):
        assert not dc.equalities(dc.family(3, m))


WALKS = [(m, dc.A_R, None, (0, 2)) for m in dc.A_GRID] + [dc.A_EXTRA + ((0, 2),)] + \
        [(m, dc.C_R, None, (0, 1, 2)) for m in dc.C_GRID] + [dc.C_EXTRA + ((0, 1, 2),)]


@pytest.mark.parametrize('m,R,restarts,blocks', WALKS, ids=['m%d-R%d' % (w[0], w[1]) for w in WALKS])
def test_oracle_walks_move(orc, m, R, restarts, blocks):
    """Against a vacuous walk: on the oracle alone, at least a quarter of the visits the GPU test compares change x_i; the
    phase-2 starts satisfy every '<=' constraint, so their slack is the violation of the equalities."""
    case = dc.walk_case(orc, m, R=R, restarts=restarts)
    moved, total = dc.moved_visits(case, blocks)
    assert total == 2 * len(case.restarts) * sum(min(16, case.n - 16 * b) for b in blocks)
    assert 4 * moved >= total, (m, moved, total)
    F = case.prob.eval_batch(case.X[2][:, list(case.restarts)], want_F=True)[2]
    eq = set(dc.equalities(case.funcs))
    le = [k for k in range(1, m + 1) if k not in eq]
    assert np.max(F[le]) <= 0.0
    for j, r in enumerate(case.restarts):
        ref = max(abs(F[k, j]) for k in eq) if eq else 0.0
        assert abs(case.slack[2][r] - ref) <= 1e-12 * (1.0 + ref)


@pytest.mark.parametrize('name,gaps,segments', [('g31', 31, 32), ('g32', 32, 33), ('g64', 64, 32), ('g65', 65, 32)])
def test_gap_problems_fill_the_lists(orc, name, gaps, segments):
    """The hand-built problems put exactly the stated number of gaps into [L, H] of coordinate 0 and leave the stated number
    of segments -- at the feasible starts (slack 0) and at the infeasible ones (phase 1 bisects the slack: gaps shrink, none
    disappears below the start's violation) -- and no other coordinate sees a gap.  DN_GC = 64 gaps and DN_SC = 32 segments
    are what the chain kernels keep."""
    funcs = dc.gap_problem(name)
    prob = orc.Problem(funcs)
    assert len(dc.gap_islands(name)) == segments - 1 and len(dc.gap_segments(name)) == segments
    X = dc.gap_starts(name, 12)
    for r in range(X.shape[1]):
        assert prob.max_violation(X[:, r]) == 0.0
        assert not dc.in_a_gap(name, X[0, r])
        assert dc.x0_feasible_set(orc, prob, funcs, X[:, r]) == (gaps, segments)
    Xi = dc.gap_starts(name, 12, feasible=False)
    for r in range(Xi.shape[1]):
        v = prob.max_violation(Xi[:, r])
        assert v > 1e-2 and dc.in_a_gap(name, Xi[0, r])
        assert dc.x0_feasible_set(orc, prob, funcs, Xi[:, r], s=0.5 * v) == (gaps, segments)
    # the other coordinates: the ball and the coupling constraint, one interval each
    for k in range(1, len(funcs)):
        t2, t1, _ = prob.onevar_coeffs(k, X[:, 0], 1)
        assert (t2 == 0.0 and t1 == 0.0) == (k <= len(funcs) - 3)
    assert (gaps <= dc.DN_GC) == (name != 'g65') and (segments <= dc.DN_SC) == (name != 'g32')
