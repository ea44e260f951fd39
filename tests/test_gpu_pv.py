"""GPU: the Ertel PV and dynamic-tropopause diagnostics on the device (mpas_dyc_set_pv /
mpas_dyc_pv_diagnostics, pv.hip).

The arithmetic is + - * / sqrt only, so everything is compared bit for bit (np.array_equal):
* on the fixture's mesh (x1.162, every K of tests/golden/pv_x1.162.npz) against what the reference's own
  pv_diagnostics.F computed -- ertel_pv below level K, where the reference is defined -- and against the host
  restatement (mpas_dycore.pv, pinned to the same fixture by tests/test_pv_host.py) at every level;
* against the restatement on x1.642 with 600 owned cells (K = 26 and 64, the boundary of the fill's words
  and of the kernel's chunks), on a variable-resolution mesh with heptagons, and with maxEdges declared 10;
* structure: the captured step untouched, the lazily allocated group, four blocks against one, the errors.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pv_x1.162.npz")
KS = (4, 26, 63, 64, 150)
NS = 3
NSOLVE = 600
MARK, IMARK = 12345.678, -77
STEP_DT = 600.0
OUT = ("ertel_pv", "iLev_DT", "u_pv", "v_pv", "theta_pv", "vort_pv")
STATE_IN = ("theta_m", "rho_zz", "w")
DIAG_IN = ("uReconstructX", "uReconstructY", "uReconstructZ", "uReconstructZonal", "uReconstructMeridional", "vorticity")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _img(a):
    out = np.zeros((a.shape[0] + 1,) + a.shape[1:], dtype=a.dtype)
    out[:-1] = a
    return out


def _mesh_of(case):
    """The mesh arrays the restatement reads, with the vectors Dycore.set_pv uploads."""
    from mpas_dycore import reconstruct
    m = dict(case)
    m.update(reconstruct.initialize_vectors(case))
    return m


def _mark(dy, block=0):
    for name in OUT + ("theta", "rho"):
        nb = dy.field_bytes("diag", name, block)
        dy.set_raw("diag", name, np.full(nb // 4, IMARK, dtype=np.int32) if name == "iLev_DT" else np.full(nb // 8, MARK),
                   block=block)


def _outputs(dy, block=0):
    """The six outputs, theta and rho as element-major arrays with the garbage slot."""
    n1 = dy.nb[block]["cell"] + 1
    out = {}
    for name in OUT + ("theta", "rho"):
        a = dy.get_raw("diag", name, block=block).copy()
        out[name] = a.reshape(n1, -1) if a.size > n1 else a
    return out


def _device_inputs(dy, block=0, tl=1):
    f = {n: dy.get("state", n, tl, block) for n in STATE_IN}
    f["qv"] = dy.get("state", "scalars", tl, block)[:, :, 0].copy()
    f.update({n: dy.get("diag", n, block=block) for n in DIAG_IN})
    return f


def _upload(dy, f, ns):
    n, K = f["theta_m"].shape
    sc = np.zeros((n, K, ns))
    sc[:, :, 0] = f["qv"]
    dy.set_raw("state", "scalars", _img(sc), 1)
    for name in STATE_IN:
        dy.set_raw("state", name, _img(f[name]), 1)
    for name in DIAG_IN:
        dy.set_raw("diag", name, _img(f[name]))


def _check(got, want, n_solve, n, label):
    """got: _outputs of a marked context; want: pv.driver's.  Owned cells, all cells, and what must keep its bits."""
    assert np.array_equal(got["theta"][:n], want["theta"]) and np.array_equal(got["rho"][:n], want["rho"]), label
    assert np.array_equal(got["ertel_pv"][:n_solve], want["ertel_pv"][:n_solve]), f"{label}: ertel_pv"
    assert np.array_equal(got["iLev_DT"][:n], want["iLev_DT"]), f"{label}: iLev_DT"
    for name in ("u_pv", "v_pv", "theta_pv", "vort_pv"):
        assert np.array_equal(got[name][:n_solve], want[name]), f"{label}: {name}"
        assert np.all(got[name][n_solve:] == MARK), f"{label}: {name} written past the owned cells"
    assert np.all(got["ertel_pv"][n_solve:] == MARK) and got["iLev_DT"][n] == IMARK, label
    assert np.all(got["theta"][n] == MARK) and np.all(got["rho"][n] == MARK), label


@pytest.mark.parametrize("K", KS)
def test_fixture_mesh_against_compiled_reference(golden, K):
    from mpas_dycore import Dycore, pv
    from mpas_dycore.init_atm import build_case
    m = pv.fixture_mesh()
    f, ref = pv.fixture_state(golden, K)
    want = pv.fixture_driver(m, f)
    case = build_case({k: v for k, v in m.items() if k not in ("cellTangentPlane", "localVerticalUnitVectors",
                                                               "edgeNormalVectors")}, K=K, ns=1)
    n = case["nCells"]
    dy = Dycore(case, device=0)
    dy.set("mesh", "zgrid", f["zgrid"])
    dy.set("mesh", "zz", np.ones((n, K)))
    _upload(dy, f, 1)
    dy.set_pv(True)
    _mark(dy)
    dy.pv_diagnostics(1)
    got = _outputs(dy)
    assert dy.pv_sweeps() == pv.flood_fill_tropo(dict(m, nCells=n), want["ertel_pv"], count_sweeps=True)[2] >= 3
    dy.close()
    assert np.array_equal(got["ertel_pv"][:n, :K - 1], ref["ertel_pv"]), "ertel_pv against the compiled reference"
    assert np.array_equal(got["iLev_DT"][:n], ref["iLev_DT"])
    for name in pv.FIELDS_2D:
        assert np.array_equal(got[name][:n], ref[name]), f"{name} against the compiled reference"
    _check(got, want, n, n, f"x1.162 K={K}")


_CASES = {}


def _case(K):
    from mpas_dycore.cases import jw_case
    if K not in _CASES:
        _CASES[K] = jw_case(642, K=K, ns=NS, moist=True, cache=False)
    return _CASES[K]


def _synthetic(case, seed):
    """The JW case's stratification with seeded winds, w and vorticity of both signs."""
    n, nv, K = case["nCells"], case["nVertices"], case["nVertLevels"]
    rng = np.random.default_rng(seed)
    qv = np.array(case["scalars"], dtype=np.float64).reshape(n, K, NS)[:, :, 0].copy()
    f = {"qv": qv, "theta_m": np.asarray(case["theta"]) * (1.0 + 461.6 / 287.0 * qv),
         "rho_zz": np.asarray(case["rho"]) / np.asarray(case["zz"]), "w": 0.2 * (rng.random((n, K + 1)) - 0.5),
         "vorticity": 4.0e-5 * (rng.random((nv, K)) - 0.5)}
    for name, amp in (("uReconstructX", 20.0), ("uReconstructY", 20.0), ("uReconstructZ", 10.0), ("uReconstructZonal", 30.0),
                      ("uReconstructMeridional", 15.0)):
        f[name] = amp * (rng.random(n) - 0.5)[:, None] + (rng.random((n, K)) - 0.5)
    return f


@pytest.mark.parametrize("K", (26, 64))
def test_owned_cells_and_markers(K):
    """x1.642 with 600 owned cells: the cells 600..641 play the halo (their ertel_pv is the marker, which the
    fill reads as the reference would), and they and the garbage slots keep their bits."""
    from mpas_dycore import Dycore, pv
    case = _case(K)
    n = case["nCells"]
    f = _synthetic(case, 11 + K)
    dy = Dycore(case, device=0, moist_end=NS, solve=(NSOLVE, case["nEdges"], case["nVertices"]))
    _upload(dy, f, NS)
    dy.set_pv(True)
    _mark(dy)
    dy.pv_diagnostics(1)
    got = _outputs(dy)
    dy.close()
    want = pv.driver(_mesh_of(case), f, n_solve=NSOLVE, ertel_pv_held=np.full((n, K), MARK))
    assert 0 < np.count_nonzero((want["iLev_DT"] >= 2) & (want["iLev_DT"] <= K)) and np.ptp(want["theta_pv"]) > 1.0
    _check(got, want, NSOLVE, n, f"x1.642 K={K}")


def _after_steps(case, nsteps):
    """(outputs, the device's own inputs) after nsteps of the case and the shift."""
    from mpas_dycore import Dycore
    dy = Dycore(case, device=0, moist_end=NS)
    dy.init_diagnostics(float(case.get("dt", STEP_DT)))
    for it in range(1, nsteps + 1):
        dy.atm_timestep(float(case.get("dt", STEP_DT)), it)
        dy.shift_time_levels()
    dy.set_pv(True)
    _mark(dy)
    dy.pv_diagnostics(1)
    got, f = _outputs(dy), _device_inputs(dy)
    dy.close()
    return got, f


def test_variable_resolution_heptagons(varres_case_small):
    from mpas_dycore import pv
    case = varres_case_small
    n = case["nCells"]
    assert case["nEdgesOnCell"].max() == 7 and case["nEdgesOnCell"].min() == 5
    got, f = _after_steps(case, 1)
    want = pv.driver(_mesh_of(case), f)
    assert np.ptp(want["ertel_pv"]) > 1.0
    _check(got, want, n, n, "variable resolution")


def test_declared_max_edges_10(moist_case):
    """maxEdges declared 10 (pad_max_edges): the bits of the 6-wide mesh."""
    from mpas_dycore.mesh import pad_max_edges
    a, fa = _after_steps(moist_case, 1)
    b, _ = _after_steps(pad_max_edges(moist_case, 10, 20, "none"), 1)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    from mpas_dycore import pv
    _check(a, pv.driver(_mesh_of(moist_case), fa), moist_case["nCells"], moist_case["nCells"], "x1.642 after a step")


def _step_run(case, with_pv):
    from mpas_dycore import Dycore
    dy = Dycore(case, device=0, moist_end=NS)
    dy.init_diagnostics(STEP_DT)
    dy.use_graph(True)
    if with_pv:
        dy.set_pv(True)
    out = []
    for it in range(1, 4):
        dy.atm_timestep(STEP_DT, it)
        active, caps = dy.graph_active(), dy.graph_captures()
        dy.shift_time_levels()
        if with_pv:
            dy.pv_diagnostics(1)
        dy.synchronize()
        out.append(({m: dy.get("state", m, 1) for m in ("u", "w", "theta_m", "rho_zz", "scalars")}, active, caps))
    dy.close()
    return out


def test_captured_steps_untouched(moist_case):
    plain, with_pv = _step_run(moist_case, False), _step_run(moist_case, True)
    for it, ((s0, a0, c0), (s1, a1, c1)) in enumerate(zip(plain, with_pv)):
        assert a0 == a1 and c0 == c1, (it, a0, a1, c0, c1)
        for m in s0:
            assert np.array_equal(s0[m], s1[m]), f"step {it + 1} {m}"
    assert plain[-1][1] and plain[-1][2] == 2


def test_off_is_off(moist_case):
    from mpas_dycore import Dycore
    from mpas_dycore import fields as F
    case = moist_case
    n, K = case["nCells"], case["nVertLevels"]
    dy = Dycore(case, device=0, moist_end=NS)
    pools = [("diag", name) for name in F.PV_OUTPUTS] + [("mesh", name) for name in F.PV_MESH_INPUTS]
    for pool, name in pools:
        assert dy.field_bytes(pool, name) == 0, name
        assert not dy.lib.mpas_dyc_field_device_ptr(dy.h, pool.encode(), name.encode(), 1)
    dy.set_pv(False)
    dy.pv_diagnostics(1)                                    # switch off: nothing to do, nothing allocated
    for pool, name in pools:
        assert dy.field_bytes(pool, name) == 0, name
    dy.set_raw("diag", "u_pv", np.full(n + 1, 3.0))          # a first set_field allocates the group, zeroed
    assert dy.field_bytes("diag", "ertel_pv") == 8 * K * (n + 1) and dy.field_bytes("diag", "iLev_DT") == 4 * (n + 1)
    assert dy.field_bytes("mesh", "cellTangentPlane") == 8 * 6 * (n + 1)
    assert dy.field_bytes("mesh", "edgeNormalVectors") == 8 * 3 * (case["nEdges"] + 1)
    assert not dy.get_raw("diag", "ertel_pv").any() and not dy.get_raw("diag", "iLev_DT").any()
    dy.pv_diagnostics(1)                                    # still off
    assert np.all(dy.get_raw("diag", "u_pv") == 3.0)
    dy.close()


def test_four_blocks_equal_one_block(moist_case):
    """The six outputs on the owned cells, in global numbering, bit for bit: the call exchanges the halos of
    theta, uReconstructX/Y/Z, w and ertel_pv, which are spoilt first.  The fill does not communicate, so a
    block's fill can differ from the whole mesh's (the reference's own edge case, pv_diagnostics.F:696): the
    restatement first shows on the CPU that it does not for this state."""
    from mpas_dycore import Dycore, decomp, pv
    case = moist_case
    n, K = case["nCells"], case["nVertLevels"]

    def run(dy, blocks):
        dy.init_diagnostics(STEP_DT)
        for it in range(1, 4):
            dy.atm_timestep(STEP_DT, it)
            dy.shift_time_levels()
        dy.set_pv(True)
        if blocks is not None:
            for ib in range(dy.nblocks):
                own = blocks[ib].layer_end["cell"][0]
                for name in ("theta", "uReconstructX", "uReconstructY", "uReconstructZ", "ertel_pv"):
                    img = dy.get_raw("diag", name, block=ib).reshape(-1, K).copy()
                    img[own:-1] = 777.0
                    dy.set_raw("diag", name, img, block=ib)
        dy.pv_diagnostics(1)
        out = [_outputs(dy, ib) for ib in range(dy.nblocks)]
        dy.close()
        return out

    one = run(Dycore(case, device=0, moist_end=NS), None)[0]
    blocks = decomp.decompose(case, decomp.partition_sfc(n, 4))
    whole = pv.flood_fill_tropo(case, one["ertel_pv"][:n])[1]
    assert np.ptp(whole) > 0
    for b in blocks:
        mine = pv.flood_fill_tropo(b.case, one["ertel_pv"][b.glob["cell"]])[1]
        own = b.layer_end["cell"][0]
        assert np.array_equal(mine[:own], whole[b.glob["cell"][:own]]), "the per-block fill differs for this state"
    four = run(Dycore.from_blocks(blocks, device=0, moist_end=NS), blocks)
    for name in OUT:
        got = decomp.gather_owned(blocks, [o[name][:-1].astype(np.float64) for o in four], "cell", n)
        assert np.array_equal(got, one[name][:-1]), name


def test_error_returns(moist_case):
    import ctypes as C
    from mpas_dycore import Dycore, _lib
    from mpas_dycore import fields as F
    from mpas_dycore.dycore import _make_dims
    from mpas_dycore.layout import to_fortran
    case = moist_case
    EINVAL, ESTATE = -1, -3
    dy = Dycore(case, device=0, moist_end=NS)
    lib, h = dy.lib, dy.h
    assert lib.mpas_dyc_pv_diagnostics(h, 0) == EINVAL and lib.mpas_dyc_pv_diagnostics(h, 3) == EINVAL
    assert dy.field_bytes("diag", "ertel_pv") == 0                            # the failures allocated nothing
    # the switch on, the mesh vectors never set: each is named in turn
    assert lib.mpas_dyc_set_pv(h, 1) == 0
    vec = _mesh_of(case)
    for name in F.PV_MESH_INPUTS:
        assert lib.mpas_dyc_pv_diagnostics(h, 1) == ESTATE
        assert name.encode() in lib.mpas_dyc_last_error(h), lib.mpas_dyc_last_error(h)
        dy.set_raw("mesh", name, to_fortran({**case, name: vec[name]}, name))
    assert lib.mpas_dyc_pv_diagnostics(h, 1) == ESTATE and b"areaCell" in lib.mpas_dyc_last_error(h)
    dy.set_pv(True)                                                            # uploads the case's areaCell too
    assert lib.mpas_dyc_pv_diagnostics(h, 1) == 0 and lib.mpas_dyc_pv_diagnostics(h, 2) == 0
    out = (C.c_double * 10)(*([-1.0] * 10))
    assert lib.mpas_dyc_get_profile(h, out, 9) == 0 and out[9] == -1.0        # out[9] only when n covers it
    assert dy.pv_ms(1) > 0.0
    dy.close()
    # between the step and finish_step under the host's microphysics
    dy = Dycore(case, device=0, moist_end=NS)
    dy.init_diagnostics(STEP_DT)
    dy.set_physics(tendencies=True, microphysics=True)
    dy.set_pv(True)
    dy.atm_timestep(STEP_DT, 1)
    assert dy.lib.mpas_dyc_pv_diagnostics(dy.h, 2) == ESTATE
    dy.finish_step(STEP_DT)
    assert dy.lib.mpas_dyc_pv_diagnostics(dy.h, 2) == 0
    dy.close()
    # a host-only context keeps the switch, allocates nothing, and cannot run the diagnostics
    dims = _make_dims([case], [None], NS)
    cfg = _lib.make_config(case["config"])
    hh = C.c_void_p()
    assert lib.mpas_dyc_create_blocks(1, dims, C.byref(cfg), _lib.HOST_ONLY, C.byref(hh)) == 0
    try:
        assert lib.mpas_dyc_set_pv(hh, 1) == 0
        assert lib.mpas_dyc_field_bytes(hh, b"diag", b"ertel_pv") == 0
        assert lib.mpas_dyc_pv_diagnostics(hh, 1) == ESTATE
    finally:
        lib.mpas_dyc_destroy(hh)
