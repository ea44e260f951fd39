"""CPU: the numpy restatement of the PV diagnostics (mpas_dycore.pv) against tests/golden/pv_x1.162.npz, which
tools/make_pv_golden.py produced with the reference's own pv_diagnostics.F compiled as it is.

* pv.py equals the fixture bit for bit: ertel_pv at levels 1..K-1 (level K is undefined in the reference,
  pv_diagnostics.F:997), iLev_DT, the members and the four interpolated fields in full;
* a plain-loop transcription of floodFill_tropo's in-place sweeps gives the members of pv.py's mask fixed point;
* a plain-loop transcription of calc_gradxu_cell / calc_grad_cell, which rebuild the geometry at every
  level, gives the bits of pv.py's per-cell table;
* the fixture exercises what it must (the conditions the generator asserted).
"""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pv_x1.162.npz")
KS = (4, 26, 63, 64, 150)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def mesh():
    from mpas_dycore import pv
    return pv.fixture_mesh()


@pytest.fixture(scope="module")
def hosts(golden, mesh):
    """The restatement on every state of the fixture, computed once."""
    from mpas_dycore import pv
    return {K: pv.fixture_driver(mesh, pv.fixture_state(golden, K)[0]) for K in KS}


def test_fixture_shape(golden, mesh):
    from mpas_dycore import pv
    assert tuple(golden["K"]) == KS and int(golden["mesh_level"]) == pv.FIXTURE_MESH_LEVEL
    assert mesh["nCells"] == 162 and os.path.getsize(GOLDEN) <= 1 << 20
    for K in KS:
        for name in pv.FIXTURE_FIELDS:
            assert golden[f"{name}_K{K}"].dtype == np.float32, name


@pytest.mark.parametrize("K", KS)
def test_restatement_equals_compiled_reference(golden, hosts, K):
    from mpas_dycore import pv
    _, ref = pv.fixture_state(golden, K)
    host = hosts[K]
    assert ref["ertel_pv"].shape == (162, K - 1)
    assert np.array_equal(host["ertel_pv"][:, :K - 1], ref["ertel_pv"])
    assert np.array_equal(host["iLev_DT"], ref["iLev_DT"]) and host["iLev_DT"].dtype == np.int32
    assert np.array_equal(host["inTropo"], ref["inTropo"])
    for name in pv.FIELDS_2D:
        assert np.array_equal(host[name], ref[name]), name


def _fill_loops(m, ertel_pv):
    """floodFill_tropo (:626-697) as it is written: in-place sweeps in cell and level order."""
    nC, K = ertel_pv.shape
    lat, ne, coc = m["latCell"], m["nEdgesOnCell"], m["cellsOnCell"]
    cand = np.zeros((nC + 1, K), dtype=np.int32)
    tropo = np.zeros((nC + 1, K), dtype=np.int32)
    for c in range(nC):
        s = np.copysign(1.0, lat[c])
        for k in range(K):
            if ertel_pv[c, k] * s - 2.0 < 0:
                cand[c, k] = 1
    changed = 0
    for c in range(nC):
        for k in range(min(K, 3)):
            if cand[c, k] > 0:
                tropo[c, k], cand[c, k] = 1, 0
                changed += 1
    while changed > 0:
        changed = 0
        for c in range(nC):
            for k in range(K):
                if cand[c, k] <= 0:
                    continue
                if k > 0 and tropo[c, k - 1] > 0:
                    tropo[c, k], cand[c, k] = 1, 0
                    changed += 1
                    continue
                for i in range(ne[c]):   # the Fortran's `cycle` here only ends this neighbour's turn
                    nb = coc[c, i] if coc[c, i] >= 0 else nC
                    if tropo[nb, k] > 0:
                        tropo[c, k], cand[c, k] = 1, 0
                        changed += 1
                if k < K - 1 and tropo[c, k + 1] > 0:
                    tropo[c, k], cand[c, k] = 1, 0
                    changed += 1
    return tropo[:nC] > 0


@pytest.mark.parametrize("K", (4, 26, 64))
def test_fill_fixed_point_is_order_independent(mesh, hosts, K):
    host = hosts[K]
    assert np.array_equal(_fill_loops(mesh, host["ertel_pv"]), host["inTropo"])


def _epv_loops(m, f, theta, rho, cells, K):
    """calc_epv (:1194-1215) with calc_gradxu_cell / calc_grad_cell transcribed per cell-level: the geometry
    is rebuilt at every level, as the reference does.  Level K's dv_dz takes velCellm."""
    from mpas_dycore import pv
    dot = lambda a, b: ((0.0 + a[0] * b[0]) + a[1] * b[1]) + a[2] * b[2]  # noqa: E731

    def unit(v):
        mag = np.sqrt(((0.0 + v[0] * v[0]) + v[1] * v[1]) + v[2] * v[2])
        return v / mag
    zg, w = f["zgrid"], f["w"]
    vel = np.stack([f["uReconstructX"], f["uReconstructY"], f["uReconstructZ"]], axis=-1)
    out = np.zeros((len(cells), K))
    for row, c in enumerate(cells):
        for k in range(K):
            xyz = [unit(m["cellTangentPlane"][c, 0]), unit(m["cellTangentPlane"][c, 1]), m["localVerticalUnitVectors"][c]]
            n = int(m["nEdgesOnCell"][c])
            normal, dv, dh = [], [], []
            for i in range(n):
                e = m["edgesOnCell"][c, i]
                sign = 1.0 if m["cellsOnEdge"][e, 0] == c else -1.0
                normal.append(unit(m["edgeNormalVectors"][e]) * sign)
                dv.append(m["dvEdge"][e])
                dh.append(100.0)
            avg = 0.0
            for i in range(n):
                avg = avg + dh[i]
            vol = m["areaCell"][c] * (avg / n)

            def horiz(vals, direction):
                rsum = 0.0
                for i in range(n):
                    face = dv[i] * dh[i]
                    face = face * dot(unit(normal[i]), direction)
                    rsum = rsum + vals[i] * face
                return rsum / vol

            def vert(val):
                z = lambda kk: 0.5 * (zg[c, kk] + zg[c, kk + 1])  # noqa: E731
                if k == 0:
                    return (val(1) - val(0)) / (z(1) - z(0))
                if k == K - 1:
                    return (val(k) - val(k - 1)) / (z(k) - z(k - 1))
                return 0.5 * ((val(k + 1) - val(k)) / (z(k + 1) - z(k)) + (val(k) - val(k - 1)) / (z(k) - z(k - 1)))
            nbrs = [m["cellsOnCell"][c, i] for i in range(n)]
            w0 = .5 * (w[c, k + 1] + w[c, k])
            w_e = [0.5 * (.5 * (w[b, k + 1] + w[b, k]) + w0) for b in nbrs]
            t_e = [0.5 * (theta[b, k] + theta[c, k]) for b in nbrs]
            vv = 0.0
            for i in range(n):
                v = m["verticesOnCell"][c, i]
                j = list(m["cellsOnVertex"][v]).index(c)
                vv = vv + m["kiteAreasOnVertex"][v, j] * f["vorticity"][v, k] / m["areaCell"][c]
            gxu = [horiz(w_e, xyz[1]) - vert(lambda kk: dot(vel[c, kk], xyz[1])),
                   vert(lambda kk: dot(vel[c, kk], xyz[0])) - horiz(w_e, xyz[0]), vv]
            ev = [dot(np.array([0.0, 0.0, 2.0 * pv.OMEGA]), x) for x in xyz]
            gxu = [(g + e) / rho[c, k] for g, e in zip(gxu, ev)]
            gth = [horiz(t_e, xyz[0]), horiz(t_e, xyz[1]), vert(lambda kk: theta[c, kk])]
            out[row, k] = dot(gxu, gth) * 1.0e6
    return out


@pytest.mark.parametrize("K", (4, 26))
def test_per_cell_table_changes_no_bit(golden, mesh, hosts, K):
    from mpas_dycore import pv
    f, _ = pv.fixture_state(golden, K)
    host = hosts[K]
    pent = np.flatnonzero(mesh["nEdgesOnCell"] == 5)[:3]
    cells = np.concatenate([pent, np.arange(0, 162, 9)])
    assert np.array_equal(_epv_loops(mesh, f, host["theta"], host["rho"], cells, K), host["ertel_pv"][cells])


@pytest.mark.parametrize("K", KS)
def test_fixture_exercises_the_branches(mesh, hosts, K):
    from mpas_dycore import pv
    c = pv.conditions(mesh, hosts[K]["ertel_pv"])
    assert c["none"] >= 3 and c["above"] >= 3, c
    assert c["interior"] >= 0.30 and c["north"] > 0 and c["south"] > 0, c
    assert c["small_dv_dl"] >= 3 and c["detached"] >= 3 and c["sideways"] >= 3, c
    assert c["sweeps"] >= 3 and c["pentagons"] == 12, c
