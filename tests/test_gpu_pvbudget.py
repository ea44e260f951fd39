"""GPU: the Ertel PV budget on the device (mpas_dyc_set_pv_budget / mpas_dyc_pv_budget_diagnostics, pvbudget.hip).

The arithmetic is + - * / only, so everything is compared bit for bit (np.array_equal):
* on the fixture's mesh (every K and source set of tests/golden/pvbudget.npz) against what the reference's own
  pv_diagnostics.F computed -- the 3-D terms below level K, where the reference is defined, and dtheta_dt_mix --
  and against the host restatement (mpas_dycore.pvbudget, pinned to the same fixture by
  tests/test_pvbudget_host.py) at every level; tend_u_phys and tend.w_euler keep their bits, a second call
  gives the same bits;
* against the restatement fed the device's own inputs on x1.642 after 3 steps with physics_get_tend on the
  device (K = 26; K = 150 for three chunks; 600 owned cells so that halo cells exist), on a variable-resolution
  mesh with heptagons, and with maxEdges declared 10;
* the step's tend.u_euler / w_euler / theta_euler against the oracle's after 2 steps;
* structure: four blocks against one, the captured step untouched, the lazily allocated group, the errors.
"""
import os

import numpy as np
import pytest

from conftest import rel_linf

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pvbudget.npz")
NS = 3
NSOLVE = 600
MARK = 12345.678
STEP_DT = 600.0
EINVAL, ESTATE = -1, -3
RAW = ("rthratenlw", "rthratensw", "rthblten", "rthcuten")
# (pool, name) of what the budget reads beyond the PV diagnostics' inputs; tend_u_phys only where it is allocated
TEND_IN = (("tend", "theta_euler"), ("tend", "u_euler"), ("tend", "w_euler"), ("diag", "rho_edge"), ("diag", "dtheta_dt_mp"))
PV_STATE = ("theta_m", "rho_zz", "w")
PV_DIAG = ("uReconstructX", "uReconstructY", "uReconstructZ", "uReconstructZonal", "uReconstructMeridional", "vorticity")
# the nine fields whose halos the call exchanges
EXCHANGED = tuple(("tend_physics", n) for n in RAW) + (("diag", "dtheta_dt_mp"), ("diag", "dtheta_dt_mix"),
                                                       ("diag", "tend_u_phys"), ("tend", "u_euler"), ("tend", "w_euler"))


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
    from mpas_dycore import fields as F, reconstruct
    m = dict(case)
    if not all(n in case for n in F.PV_MESH_INPUTS):
        with np.errstate(invalid="ignore"):
            m.update(reconstruct.initialize_vectors(case))
    return m


def _out_names():
    from mpas_dycore import pvbudget as B
    return B.OUT_3D + B.OUT_2D


def _mark(dy, block=0):
    for name in _out_names() + ("dtheta_dt_mix",):
        dy.set_raw("diag", name, np.full(dy.field_bytes("diag", name, block) // 8, MARK), block=block)


def _outputs(dy, block=0):
    """The ten outputs and dtheta_dt_mix as element-major arrays with the garbage slot, and the PV diagnostics'
    ertel_pv and iLev_DT."""
    n1 = dy.nb[block]["cell"] + 1
    out = {}
    for name in _out_names() + ("dtheta_dt_mix", "ertel_pv", "iLev_DT"):
        a = dy.get_raw("diag", name, block=block).copy()
        out[name] = a.reshape(n1, -1) if a.size > n1 else a
    return out


def _device_inputs(dy, block=0, tl=1):
    """What the restatement reads, as the device holds it."""
    f = {n: dy.get("state", n, tl, block) for n in PV_STATE}
    f["qv"] = dy.get("state", "scalars", tl, block)[:, :, 0].copy()
    f.update({n: dy.get("diag", n, block=block) for n in PV_DIAG})
    for pool, name in TEND_IN:
        f[{"theta_euler": "tend_theta_euler", "u_euler": "tend_u_euler", "w_euler": "tend_w_euler"}.get(name, name)] = \
            dy.get(pool, name, block=block)
    if dy.field_bytes("diag", "tend_u_phys", block):
        f["tend_u_phys"] = dy.get("diag", "tend_u_phys", block=block)
        f.update({n: dy.get("tend_physics", n, block=block) for n in RAW})
    return f


def _check(got, want, n_solve, n, label):
    """got: _outputs of a marked context; want: pvbudget.driver's.  Owned cells, and what must keep its bits."""
    from mpas_dycore import pvbudget as B
    assert np.array_equal(got["ertel_pv"][:n_solve], want["ertel_pv"][:n_solve]), f"{label}: ertel_pv"
    assert np.array_equal(got["iLev_DT"][:n], want["iLev_DT"]), f"{label}: iLev_DT"
    assert np.array_equal(got["dtheta_dt_mix"][:n], want["dtheta_dt_mix"]), f"{label}: dtheta_dt_mix"
    assert np.all(got["dtheta_dt_mix"][n] == MARK), label
    for name in B.OUT_3D + B.OUT_2D:
        assert np.all(np.isfinite(want[name])), f"{label}: {name} of the restatement"
        assert np.array_equal(got[name][:n_solve], want[name]), \
            f"{label}: {name}: {np.count_nonzero(got[name][:n_solve] != want[name])} of {want[name].size} differ"
        assert np.all(got[name][n_solve:] == MARK), f"{label}: {name} written past the owned cells"


# ---- 1. the fixture's mesh against the compiled reference ----
def _fixture_case(m, K):
    from mpas_dycore.init_atm import build_case
    return build_case({k: v for k, v in m.items() if k not in ("cellTangentPlane", "localVerticalUnitVectors",
                                                               "edgeNormalVectors", "coeffs_reconstruct")}, K=K, ns=1)


def _fixture_upload(dy, m, f):
    n, K = f["theta_m"].shape
    dy.set("mesh", "zgrid", f["zgrid"])
    dy.set("mesh", "zz", np.ones((n, K)))
    dy.set("mesh", "coeffs_reconstruct", m["coeffs_reconstruct"])
    dy.set_raw("state", "scalars", _img(f["qv"][:, :, None].copy()), 1)
    for name in PV_STATE:
        dy.set_raw("state", name, _img(f[name]), 1)
    for name in PV_DIAG + ("rho_edge", "dtheta_dt_mp", "tend_u_phys"):
        dy.set_raw("diag", name, _img(f[name]))
    for name in RAW:
        dy.set_raw("tend_physics", name, _img(f[name]))
    for name in ("theta_euler", "u_euler", "w_euler"):
        dy.set_raw("tend", name, _img(f["tend_" + name]))


@pytest.mark.parametrize("K", (4, 65))
@pytest.mark.parametrize("name", ("all", "none", "lwcu"))
def test_fixture_mesh_against_compiled_reference(golden, name, K):
    from mpas_dycore import Dycore, pvbudget as B
    m = B.fixture_mesh()
    flags = B.FIXTURE_SETS[name]
    f, _, ref = B.fixture_state(golden, K, name)
    want = B.fixture_driver(m, f, flags)                              # its own fill's iLev_DT, as the device's
    case = _fixture_case(m, K)
    n = case["nCells"]
    dy = Dycore(case, device=0)
    _fixture_upload(dy, m, f)
    dy.set_pv(True)
    dy.set_pv_budget(flags=flags)
    _mark(dy)
    kept = {pn: dy.get_raw(*pn).copy() for pn in (("diag", "tend_u_phys"), ("tend", "w_euler"))}
    dy.pv_budget_diagnostics(1)
    got = _outputs(dy)
    for pn, a in kept.items():
        assert np.array_equal(dy.get_raw(*pn).view(np.int64), a.view(np.int64)), f"{pn} changed its bits"
    dy.pv_budget_diagnostics(1)
    again = _outputs(dy)
    dy.close()
    for nm in B.OUT_3D:
        assert np.array_equal(got[nm][:n, :K - 1], ref[nm]), f"{nm} against the compiled reference"
    assert np.array_equal(got["dtheta_dt_mix"][:n], ref["dtheta_dt_mix"])
    _check(got, want, n, n, f"fixture K={K} {name}")
    for nm in got:
        assert np.array_equal(got[nm].view(np.int64 if got[nm].dtype == np.float64 else np.int32),
                              again[nm].view(np.int64 if got[nm].dtype == np.float64 else np.int32)), f"second call: {nm}"


# ---- 2. x1.642 after 3 steps with physics_get_tend on the device ----
_STEPPED = {}


def _stepped(K):
    """(outputs of a marked context, the device's own inputs, the Fortran images of every input) after 3 steps of
    test_gpu_todynamics' physics case (PBL and CU winds, LW, SW) and the shift."""
    from mpas_dycore import Dycore
    from test_gpu_todynamics import NS7, SET3, case7, upload_raw
    if K in _STEPPED:
        return _STEPPED[K]
    case, raw = case7(K)
    dt = float(case["dt"])
    dy = Dycore(case, device=0, moist_end=6)
    dy.init_diagnostics(dt)
    dy.set_todynamics(**SET3, **NS7)
    upload_raw(dy, raw)
    for it in range(1, 4):
        dy.atm_timestep(dt, it)
        dy.shift_time_levels()
    dy.set_pv(True)
    dy.set_pv_budget()                                                # the sources of set_todynamics: all four
    _mark(dy)
    dy.pv_budget_diagnostics(1)
    got, f = _outputs(dy), _device_inputs(dy)
    images = {("state", n): dy.get_raw("state", n, 1) for n in PV_STATE + ("scalars",)}
    images.update({("diag", n): dy.get_raw("diag", n) for n in PV_DIAG + ("tend_u_phys",)})
    images.update({pn: dy.get_raw(*pn) for pn in TEND_IN})
    images.update({("tend_physics", n): dy.get_raw("tend_physics", n) for n in RAW})
    dy.close()
    _STEPPED[K] = (case, got, f, images)
    return _STEPPED[K]


@pytest.mark.parametrize("K", (26, 150))
def test_after_three_steps_with_todynamics(K):
    from mpas_dycore import pvbudget as B
    case, got, f, _ = _stepped(K)
    n = case["nCells"]
    want = B.driver(_mesh_of(case), f, B.ALL)
    for name in ("depv_dt_lw", "depv_dt_sw", "depv_dt_bl", "depv_dt_cu", "depv_dt_mix", "depv_dt_fric"):
        assert np.ptp(want[name]) > 0, name
    assert f["tend_u_phys"].any() and np.ptp(want["depv_dt_diab_pv"]) > 0
    _check(got, want, n, n, f"x1.642 K={K} after 3 steps")


def test_owned_cells_and_markers():
    """The same inputs on a context with 600 owned cells: the cells 600..641 play the halo, and they and the garbage
    slots keep the marker in every output."""
    from mpas_dycore import Dycore, pvbudget as B
    case, _, f, images = _stepped(26)
    n, K = case["nCells"], case["nVertLevels"]
    dy = Dycore(case, device=0, moist_end=6, solve=(NSOLVE, case["nEdges"], case["nVertices"]))
    for (pool, name), img in images.items():
        dy.set_raw(pool, name, img, 1)
    dy.set_pv(True)
    dy.set_pv_budget(flags=B.ALL)
    _mark(dy)
    dy.set_raw("diag", "ertel_pv", np.full((n + 1) * K, MARK))
    dy.pv_budget_diagnostics(1)
    got = _outputs(dy)
    dy.close()
    want = B.driver(_mesh_of(case), f, B.ALL, n_solve=NSOLVE, ertel_pv_held=np.full((n, K), MARK))
    _check(got, want, NSOLVE, n, "x1.642 with 600 owned cells")


# ---- 3. other meshes ----
def _after_a_step(case, flags=None):
    """No physics_get_tend: tend_u_phys is absent and the edge kernel takes 0.0; no raw source."""
    from mpas_dycore import Dycore, pvbudget as B
    dy = Dycore(case, device=0, moist_end=NS)
    dt = float(case.get("dt", STEP_DT))
    dy.init_diagnostics(dt)
    dy.atm_timestep(dt, 1)
    dy.shift_time_levels()
    dy.set_pv(True)
    dy.set_pv_budget(flags=B.ON if flags is None else flags)
    _mark(dy)
    dy.pv_budget_diagnostics(1)
    got, f = _outputs(dy), _device_inputs(dy)
    assert dy.field_bytes("diag", "tend_u_phys") == 0 and dy.field_bytes("tend_physics", "rthblten") == 0
    dy.close()
    return got, f


def test_variable_resolution_heptagons(varres_case_small):
    from mpas_dycore import pvbudget as B
    case = varres_case_small
    n = case["nCells"]
    assert case["nEdgesOnCell"].max() == 7 and case["nEdgesOnCell"].min() == 5
    got, f = _after_a_step(case)
    assert "tend_u_phys" not in f
    want = B.driver(_mesh_of(case), f, B.ON)
    assert np.ptp(want["depv_dt_fric"]) > 0 and np.ptp(want["depv_dt_mix"]) > 0
    _check(got, want, n, n, "variable resolution")


def test_declared_max_edges_10(moist_case):
    """maxEdges declared 10 (pad_max_edges): the bits of the 6-wide mesh."""
    from mpas_dycore import pvbudget as B
    from mpas_dycore.mesh import pad_max_edges
    a, fa = _after_a_step(moist_case)
    b, _ = _after_a_step(pad_max_edges(moist_case, 10, 20, "none"))
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    _check(a, B.driver(_mesh_of(moist_case), fa, B.ON), moist_case["nCells"], moist_case["nCells"], "x1.642 after a step")


# ---- 4. the inputs are what the reference has ----
def test_euler_tendencies_match_the_reference(small_case):
    """tend.u_euler / w_euler / theta_euler as two steps leave them, on the owned elements, against the oracle's.
    The bound is tests/test_gpu_parity.py's for derived fields of a run of more than one step (rel Linf 1e-10; its
    one-step bound for them is 1e-11): the tendencies are sums of differences of the fields it bounds."""
    from mpas_dycore import Dycore
    from oracle import ref_runner
    if not ref_runner.available():
        pytest.skip("oracle/_ref not built")
    from test_gpu_parity import DT
    ref = ref_runner.run_reference(small_case, nsteps=2, dt=DT, dump_steps=[2], nthreads=4)[0][2]
    dy = Dycore(small_case, device=0)
    dy.init_diagnostics(DT)
    for it in (1, 2):
        dy.atm_timestep(DT, it)
        dy.shift_time_levels()
    dy.synchronize()
    errs = {}
    for name in ("u_euler", "w_euler", "theta_euler"):
        got, want = dy.get("tend", name), ref[f"tend.{name}"]
        errs[name] = rel_linf(got.reshape(want.shape), want)
        print(f"tend.{name}: rel Linf {errs[name]:.3e}, max |ref| {np.max(np.abs(want)):.3e}")
    dy.close()
    bad = {k: v for k, v in errs.items() if not v <= 1e-10}
    assert not bad, f"rel Linf above 1e-10: {bad} (all: {errs})"


# ---- 5. blocks ----
def test_four_blocks_equal_one_block():
    """The diabatic outputs on the owned cells, in global numbering, bit for bit with one block: the call
    exchanges the halos of the nine fields of EXCHANGED (and the PV diagnostics' six), which are spoilt first.
    Local edge numbering changes the curl's summation order -- in the reference too -- so depv_dt_fric and
    depv_dt_fric_pv of each block are compared with the restatement on that block's local mesh instead.  The fill
    does not communicate: the restatement first shows on the CPU that the per-block fill equals the whole
    mesh's for this state (tests/test_gpu_pv.py)."""
    from mpas_dycore import Dycore, decomp, pv, pvbudget as B
    from test_gpu_todynamics import NS7, SET3, block_partition, case7, upload_raw
    case, raw = case7(26)
    n, K = case["nCells"], case["nVertLevels"]
    dt = float(case["dt"])
    case1, one, _, _ = _stepped(26)
    assert case1 is case

    blocks = decomp.decompose(case, block_partition(case, K))
    whole = pv.flood_fill_tropo(case, one["ertel_pv"][:n])[1]
    for b in blocks:
        mine = pv.flood_fill_tropo(b.case, one["ertel_pv"][b.glob["cell"]])[1]
        own = b.layer_end["cell"][0]
        assert np.array_equal(mine[:own], whole[b.glob["cell"][:own]]), "the per-block fill differs for this state"

    dy = Dycore.from_blocks(blocks, device=0, moist_end=6)
    dy.init_diagnostics(dt)
    dy.set_todynamics(**SET3, **NS7)
    upload_raw(dy, raw, blocks)
    for it in range(1, 4):
        dy.atm_timestep(dt, it)
        dy.shift_time_levels()
    dy.set_pv(True)
    dy.set_pv_budget()
    for ib, b in enumerate(blocks):
        _mark(dy, ib)
        for pool, name in EXCHANGED + tuple(("diag", x) for x in ("theta", "uReconstructX", "uReconstructY", "uReconstructZ")):
            own = b.layer_end["edge" if name in ("tend_u_phys", "u_euler") else "cell"][0]
            img = dy.get_raw(pool, name, block=ib).copy()
            img = img.reshape(dy.nb[ib]["edge" if name in ("tend_u_phys", "u_euler") else "cell"] + 1, -1)
            img[own:-1] = 777.0
            dy.set_raw(pool, name, img, block=ib)
    dy.pv_budget_diagnostics(1)
    four = [_outputs(dy, ib) for ib in range(dy.nblocks)]
    fs = [_device_inputs(dy, ib) for ib in range(dy.nblocks)]
    thetas = [dy.get("diag", "theta", block=ib) for ib in range(dy.nblocks)]   # after its exchange
    dy.close()
    for name in B.OUT_3D[:-1] + ("depv_dt_diab_pv", "ertel_pv"):
        got = decomp.gather_owned(blocks, [o[name][:-1] for o in four], "cell", n)
        assert np.array_equal(got, one[name][:-1]), name
    for ib, b in enumerate(blocks):
        own = b.layer_end["cell"][0]
        want = B.driver(_mesh_of(b.case), fs[ib], B.ALL, n_solve=own, ertel_pv_held=four[ib]["ertel_pv"][:-1],
                        mix_held=four[ib]["dtheta_dt_mix"][:-1], theta_held=thetas[ib])
        _check(four[ib], want, own, b.case["nCells"], f"block {ib}")


# ---- 6. structure ----
def _step_run(case, with_budget):
    from mpas_dycore import Dycore
    dy = Dycore(case, device=0, moist_end=NS)
    dy.init_diagnostics(STEP_DT)
    dy.use_graph(True)
    if with_budget:
        dy.set_pv(True)
        dy.set_pv_budget()
    out = []
    for it in range(1, 4):
        dy.atm_timestep(STEP_DT, it)
        active, caps = dy.graph_active(), dy.graph_captures()
        dy.shift_time_levels()
        if with_budget:
            dy.pv_budget_diagnostics(1)
        dy.synchronize()
        out.append(({m: dy.get("state", m, 1) for m in ("u", "w", "theta_m", "rho_zz", "scalars")}, active, caps))
    dy.close()
    return out


def test_captured_steps_untouched(moist_case):
    plain, with_budget = _step_run(moist_case, False), _step_run(moist_case, True)
    for it, ((s0, a0, c0), (s1, a1, c1)) in enumerate(zip(plain, with_budget)):
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
    names = F.PVB_FIELDS
    for name in names:
        assert dy.field_bytes("diag", name) == 0, name
    dy.set_pv(True)
    dy.set_pv_budget(False)
    dy.pv_budget_diagnostics(1)                              # switch off: nothing to do, nothing allocated
    for name in names:
        assert dy.field_bytes("diag", name) == 0, name
    assert not dy.get_raw("diag", "ertel_pv").any()          # not even the PV diagnostics ran
    dy.set_raw("diag", "dtheta_dt_mp", np.full((n + 1) * K, 3.0))  # a first set_field allocates the group, zeroed
    assert dy.field_bytes("diag", "depv_dt_fric") == 8 * K * (n + 1) and dy.field_bytes("diag", "depv_dt_fric_pv") == 8 * (n + 1)
    assert not dy.get_raw("diag", "depv_dt_diab").any() and not dy.get_raw("diag", "dtheta_dt_mix").any()
    dy.pv_budget_diagnostics(1)                              # still off
    assert not dy.get_raw("diag", "depv_dt_diab").any() and np.all(dy.get_raw("diag", "dtheta_dt_mp") == 3.0)
    dy.close()


def test_error_returns(moist_case):
    import ctypes as C
    from mpas_dycore import Dycore, pvbudget as B
    case = moist_case
    n, K = case["nCells"], case["nVertLevels"]
    dy = Dycore({k: v for k, v in case.items() if k != "coeffs_reconstruct"}, device=0, moist_end=NS)
    lib, h = dy.lib, dy.h
    run = lib.mpas_dyc_pv_budget_diagnostics
    err = lambda: lib.mpas_dyc_last_error(h)  # noqa: E731
    assert run(h, 0) == EINVAL and run(h, 3) == EINVAL
    assert run(h, 1) == 0 and dy.field_bytes("diag", "depv_dt_diab") == 0          # off: nothing, and no allocation
    assert lib.mpas_dyc_set_pv_budget(h, 32) == EINVAL and lib.mpas_dyc_set_pv_budget(h, B.LW) == EINVAL
    assert lib.mpas_dyc_set_pv_budget(h, B.ON) == ESTATE and b"mpas_dyc_set_pv" in err()
    assert dy.field_bytes("diag", "depv_dt_diab") == 0                             # the failures allocated nothing
    # the PV diagnostics' own states: a mesh vector never set is named
    assert lib.mpas_dyc_set_pv(h, 1) == 0 and lib.mpas_dyc_set_pv_budget(h, B.ON) == 0
    assert dy.field_bytes("diag", "depv_dt_diab") == 8 * K * (n + 1)
    assert run(h, 1) == ESTATE and b"coeffs_reconstruct" in err()
    dy.set("mesh", "coeffs_reconstruct", case["coeffs_reconstruct"])
    assert run(h, 1) == ESTATE and b"areaTriangle" in err()
    dy.set("mesh", "areaTriangle", case["areaTriangle"])
    assert run(h, 1) == ESTATE and b"cellTangentPlane" in err()
    dy.set_pv(True)                                                                # uploads the vectors and areaCell
    # todynamics never set: without source bits the call runs, tend_u_phys is 0.0 and none of the 17 raw arrays exists
    assert run(h, 1) == 0 and run(h, 2) == 0
    assert dy.field_bytes("diag", "tend_u_phys") == 0 and dy.field_bytes("tend_physics", "rthratenlw") == 0
    # ... and with a source bit the raw array that was never allocated is named
    for bit, name in ((B.LW, b"rthratenlw"), (B.SW, b"rthratensw"), (B.BL, b"rthblten"), (B.CU, b"rthcuten")):
        assert lib.mpas_dyc_set_pv_budget(h, B.ON | bit) == 0
        assert run(h, 1) == ESTATE and name in err(), err()
    assert dy.field_bytes("tend_physics", "rthratenlw") == 0
    dy.set_raw("tend_physics", "rthcuten", np.zeros((n + 1) * K))                  # allocates the group
    assert run(h, 1) == 0
    assert lib.mpas_dyc_set_pv(h, 0) == 0 and run(h, 1) == ESTATE and b"mpas_dyc_set_pv" in err()
    assert lib.mpas_dyc_set_pv(h, 1) == 0
    out = (C.c_double * 14)(*([-1.0] * 14))
    assert lib.mpas_dyc_get_profile(h, out, 13) == 0 and out[13] == -1.0           # out[13] only when n covers it
    assert dy.pv_budget_ms(1) > 0.0
    dy.close()
    # between the step and finish_step under the host's microphysics
    dy = Dycore(case, device=0, moist_end=NS)
    dy.init_diagnostics(STEP_DT)
    dy.set_physics(tendencies=True, microphysics=True)
    dy.set_pv(True)
    dy.set_pv_budget()
    dy.atm_timestep(STEP_DT, 1)
    assert dy.lib.mpas_dyc_pv_budget_diagnostics(dy.h, 2) == ESTATE
    dy.finish_step(STEP_DT)
    assert dy.lib.mpas_dyc_pv_budget_diagnostics(dy.h, 2) == 0
    dy.close()
