"""CPU: mpas_dycore.convective.update, the numpy restatement of convective_diagnostics_update
(convective_diagnostics.F:99-198) that the GPU tests compare the device against, checked against a
plain loop transcription -- the scatter over the vertices in vertex-major order, the level sum one k
after the other -- on the same synthetic fields the GPU tests use."""
import numpy as np
import pytest

_CASES = {}


def case_for(n=162, K=5):
    from mpas_dycore.cases import jw_case
    if (n, K) not in _CASES:
        _CASES[(n, K)] = jw_case(n, K=K, ns=1, cache=False)
    return _CASES[(n, K)]


def synthetic(case, ph):
    """Smooth w (nCells, K + 1), vorticity (nVertices, K) and level-1-varying reconstructed winds
    (nCells, K) of both signs; ``ph`` shifts the patterns so that a second update raises some cells
    and leaves others.  Shared with tests/test_gpu_convective.py."""
    K = case["nVertLevels"]
    lonc, latc = np.asarray(case["lonCell"])[:, None], np.asarray(case["latCell"])[:, None]
    lonv, latv = np.asarray(case["lonVertex"])[:, None], np.asarray(case["latVertex"])[:, None]
    kw = (np.arange(K + 1) / K)[None, :]
    kk = ((np.arange(K) + 0.5) / K)[None, :]
    w = 5.0 * np.sin(2 * lonc + ph) * np.cos(latc) * np.sin(np.pi * kw) + 1.5 * np.sin(3 * latc + ph)
    vort = 1e-4 * (np.cos(3 * lonv - ph) * np.cos(latv) + 0.5 * np.sin(2 * latv + ph)) * (1.0 - 0.5 * kk)
    uz = 20.0 * np.cos(latc) * np.cos(lonc + ph) * (1.0 + kk)
    um = 8.0 * np.sin(2 * lonc - ph) * np.cos(latc) * (1.0 - kk)
    return w, vort, uz, um


def loops(case, w, vort, uz, um, running, flags, n_solve=None):
    """convective_diagnostics_update statement by statement, 0-based."""
    nC, nV, K = case["nCells"], case["nVertices"], case["nVertLevels"]
    n_solve = nC if n_solve is None else n_solve
    cov, kite = case["cellsOnVertex"], case["kiteAreasOnVertex"]
    area, zgrid = case["areaCell"], case["zgrid"]
    out = {n: np.array(a, dtype=np.float64) for n, a in running.items()}
    if flags & 1:
        for c in range(n_solve):
            m = w[c, 0]
            for k in range(1, K):
                m = max(m, w[c, k])
            out["w_velocity_max"][c] = max(out["w_velocity_max"][c], m)
    if flags & 2:
        for c in range(n_solve):
            out["wind_speed_level1_max"][c] = max(out["wind_speed_level1_max"][c],
                                                  np.sqrt(uz[c, 0] * uz[c, 0] + um[c, 0] * um[c, 0]))
    if flags & 4:
        uh = np.zeros((nC + 1, K))
        for v in range(nV):
            for j in range(3):
                c = cov[v, j] if cov[v, j] >= 0 else nC
                for k in range(K):
                    uh[c, k] = uh[c, k] + kite[v, j] * vort[v, k]
        for c in range(n_solve):
            for k in range(K):
                uh[c, k] = max(0.0, 0.5 * (w[c, k] + w[c, k + 1])) * max(0.0, uh[c, k] / area[c])
        for c in range(n_solve):
            z_agl = [zgrid[c, k] - zgrid[c, 0] for k in range(K + 1)]
            s = 0.0
            for k in range(K):
                zb = max(z_agl[k], 2000.0)
                zt = min(z_agl[k + 1], 5000.0)
                s = s + uh[c, k] * max(0.0, zt - zb)
            out["updraft_helicity_max"][c] = max(out["updraft_helicity_max"][c], s)
    return out


@pytest.mark.parametrize("n", [162, 642])
def test_update_equals_the_loop_transcription(n):
    from mpas_dycore import convective
    case = case_for(n)
    run_a = run_b = convective.zeros(case)
    for ph in (0.0, 1.3):
        f = synthetic(case, ph)
        run_a = convective.update(case, *f, run_a, convective.ALL)
        run_b = loops(case, *f, run_b, convective.ALL)
        for name in convective.FIELDS.values():
            assert np.all(np.isfinite(run_a[name]))
            assert np.array_equal(run_a[name], run_b[name]), (name, ph)
    assert np.mean(run_a["updraft_helicity_max"] > 0) > 0.15


def test_second_update_keeps_the_larger_value():
    from mpas_dycore import convective
    case = case_for(642)
    zero = convective.zeros(case)
    a = convective.update(case, *synthetic(case, 0.0), zero, convective.ALL)
    b_alone = convective.update(case, *synthetic(case, 1.3), zero, convective.ALL)
    ab = convective.update(case, *synthetic(case, 1.3), a, convective.ALL)
    for name in convective.FIELDS.values():
        assert np.array_equal(ab[name], np.maximum(a[name], b_alone[name])), name
        assert np.mean(ab[name] > a[name]) > 0.15 and np.mean((ab[name] == a[name]) & (a[name] != 0)) > 0.15, name
        assert np.array_equal(zero[name], np.zeros(case["nCells"]))  # inputs are not modified


def test_flags_update_only_the_named_fields():
    from mpas_dycore import convective
    case = case_for(162)
    f = synthetic(case, 0.0)
    start = {n: np.full(case["nCells"], -7.0) for n in convective.FIELDS.values()}
    full = convective.update(case, *f, start, convective.ALL)
    for bit, name in convective.FIELDS.items():
        got = convective.update(case, *f, start, bit)
        for other in convective.FIELDS.values():
            want = full[other] if other == name else start[other]
            assert np.array_equal(got[other], want), (name, other)
        assert not np.array_equal(got[name], start[name])
    none = convective.update(case, *f, start, 0)
    assert all(np.array_equal(none[n], start[n]) for n in start)
    with pytest.raises(ValueError):
        convective.update(case, *f, start, 8)


def test_owned_range_and_dropped_garbage_entries():
    """A block's numbering: only cells [0, n_solve) are advanced, and vertex entries that point
    outside the block (-1, the garbage cell at the C ABI) are dropped."""
    from mpas_dycore import convective, decomp
    case = case_for(642)
    blocks = decomp.decompose(case, decomp.partition_sfc(case["nCells"], 4))
    b = blocks[1]
    assert (np.asarray(b.case["cellsOnVertex"]) < 0).any()
    f = synthetic(b.case, 0.0)
    zero = convective.zeros(b.case)
    got = convective.update(b.case, *f, zero, convective.ALL, n_solve=b.solve[0])
    want = loops(b.case, *f, zero, convective.ALL, n_solve=b.solve[0])
    for name in convective.FIELDS.values():
        assert np.array_equal(got[name], want[name]), name
        assert not got[name][b.solve[0]:].any()
