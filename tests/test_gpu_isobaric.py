"""GPU: the isobaric diagnostics and mslp on the device (mpas_dyc_set_isobaric / mpas_dyc_isobaric_diagnostics,
isobaric.hip).

Yardsticks, strongest first:
* the kernels alone against the compiled reference: the columns and vertices of
  tests/golden/isobaric_columns.npz go into the first owned cells and vertices of an x1.642 context, and the
  expected fields are what the reference's own isobaric_diagnostics.F computed;
* the other owned elements, and a real moist JW state after three steps, against the host restatement
  (mpas_dycore.isobaric, pinned to the same fixture bit for bit by tests/test_isobaric_host.py);
* structure: four blocks against one, single bits, mask 0, the lazily allocated group, the step untouched,
  compute_slp's failure path, the error returns.
Two classes of outputs.  Whatever passes through log / exp / pow -- dewpoint_*, mslp, and height_* / w_* /
z_isobaric where the bracket contains the top interface's pressure2(K + 1) or the target lies above it --
is held to the project's parity bound, rel Linf <= 1e-10 (the device library's functions are not the C
library's), as tests/test_gpu_kessler.py holds its outputs.  Everything else is pure arithmetic on inputs
the device holds exactly: bit for bit.
"""
import os

import numpy as np
import pytest

from conftest import rel_linf

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "isobaric_columns.npz")
NS = 3
NSOLVE, NVSOLVE = 600, 1200     # owned cells / vertices of the stand-alone runs: the rest play the halo
MARK = 12345.678
BOUND = 1e-10
STEP_DT = 600.0
KS = (4, 26, 63, 64, 150)
_CASES = {}


def _case(K):
    from mpas_dycore.cases import jw_case
    if K not in _CASES:
        _CASES[K] = jw_case(642, K=K, ns=NS, moist=True, cache=False)
    return _CASES[K]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _img(a, last=None):
    out = np.zeros((a.shape[0] + 1,) + a.shape[1:], dtype=a.dtype)
    out[:-1] = a
    if last is not None:
        out[-1] = last
    return out


def _fields(case, cols=None):
    """MPAS-level inputs of every cell and vertex for a stand-alone call: a hydrostatic-looking state from
    the JW case with seeded winds, w, relhum and vorticity; the fixture's columns (if any) overwrite the
    first cells, its vertices the first vertices, and its garbage cell's pressures the garbage slot."""
    from mpas_dycore import kessler as ks
    n, nv, K = case["nCells"], case["nVertices"], case["nVertLevels"]
    rng = np.random.default_rng(7 + K)
    zz = np.asarray(case["zz"], dtype=np.float64)
    f = {"zgrid": np.array(case["zgrid"], dtype=np.float64)}
    f["qv"] = np.array(case["scalars"], dtype=np.float64).reshape(n, K, NS)[:, :, 0].copy()
    f["theta_m"] = np.asarray(case["theta"]) * (1.0 + ks.R_V / ks.R_D * f["qv"])
    rtheta_base = np.asarray(case["rho_base"]) / zz * np.asarray(case["theta_base"])
    f["exner"] = (zz * (ks.R_D / ks.P0) * (np.asarray(case["rho"]) / zz) * f["theta_m"]) ** ks.RCV
    f["pressure_base"] = zz * ks.R_D * (zz * (ks.R_D / ks.P0) * rtheta_base) ** ks.RCV * rtheta_base
    f["pressure_p"] = ks.P0 * f["exner"] ** (ks.CP / ks.R_D) - f["pressure_base"]
    f["relhum"] = rng.random((n, K))
    f["uzonal"] = 30.0 * (rng.random((n, K)) - 0.3)
    f["umeridional"] = 15.0 * (rng.random((n, K)) - 0.5)
    f["w"] = rng.random((n, K + 1)) - 0.5
    f["vorticity"] = 1.0e-4 * (rng.random((nv, K)) - 0.5)
    cov = np.array(case["cellsOnVertex"], dtype=np.int64)
    f["cellsOnVertex"] = np.where(cov >= 0, cov, n)
    f["kiteAreasOnVertex"] = np.array(case["kiteAreasOnVertex"], dtype=np.float64)
    f["areaTriangle"] = np.array(case["areaTriangle"], dtype=np.float64)
    garbage = {"pressure_p": np.zeros(K), "pressure_base": np.full(K, 5.0e4)}
    if cols is not None:
        nc, nfv = cols["theta_m"].shape[0], cols["vorticity"].shape[0]
        for name in ("theta_m", "qv", "exner", "relhum", "uzonal", "umeridional", "zgrid", "w", "pressure_p",
                     "pressure_base"):
            f[name][:nc] = cols[name]
        for name in ("vorticity", "kiteAreasOnVertex", "areaTriangle"):
            f[name][:nfv] = cols[name]
        f["cellsOnVertex"][:nfv] = np.where(cols["cellsOnVertex"] >= nc, n, cols["cellsOnVertex"])
        garbage = {m: cols[m + "_img"][-1] for m in garbage}
    for m in garbage:
        f[m + "_img"] = _img(f[m], garbage[m])
    return f


def _output_names():
    from mpas_dycore import isobaric as iso
    return iso.CELL_FIELDS, iso.VERTEX_FIELDS


def _standalone(case, f, flags=None, mark=True):
    """A context of NSOLVE owned cells and NVSOLVE owned vertices holding f on time level 1, the group
    allocated, and a marker in every output."""
    from mpas_dycore import Dycore, _lib
    n, K = case["nCells"], case["nVertLevels"]
    dy = Dycore(case, device=0, moist_end=NS, solve=(NSOLVE, case["nEdges"], NVSOLVE))
    dy.set("mesh", "zgrid", f["zgrid"])
    dy.set("mesh", "cellsOnVertex", np.where(f["cellsOnVertex"] >= n, -1, f["cellsOnVertex"]))
    dy.set("mesh", "kiteAreasOnVertex", f["kiteAreasOnVertex"])
    sc = np.zeros((n, K, NS))
    sc[:, :, 0] = f["qv"]
    dy.set_raw("state", "scalars", _img(sc), 1)
    dy.set_raw("state", "theta_m", _img(f["theta_m"]), 1)
    dy.set_raw("state", "w", _img(f["w"]), 1)
    dy.set_raw("diag", "pressure_p", f["pressure_p_img"])
    dy.set_raw("diag", "pressure_base", f["pressure_base_img"])
    for name, fld in (("exner", "exner"), ("uReconstructZonal", "uzonal"), ("uReconstructMeridional", "umeridional"),
                      ("vorticity", "vorticity")):
        dy.set_raw("diag", name, _img(f[fld]))
    dy.set_isobaric(_lib.ISO_ALL if flags is None else flags)
    dy.set("mesh", "areaTriangle", f["areaTriangle"])
    dy.set_raw("diag", "relhum", _img(f["relhum"]))
    if mark:
        _mark(dy)
    return dy


def _mark(dy):
    cells, verts = _output_names()
    for name in cells + verts:
        nb = dy.field_bytes("diag", name)
        dy.set_raw("diag", name, np.full(nb // 8, MARK))


def _outputs(dy, block=0):
    """Every output as an element-major array with the garbage slot: (n + 1,) or (n + 1, 5 / 13)."""
    dy.synchronize()
    cells, verts = _output_names()
    n1 = dy.nb[block]["cell"] + 1
    out = {}
    for name in cells + verts:
        a = dy.get_raw("diag", name, block=block).copy()
        out[name] = a.reshape(n1, -1) if name in ("t_isobaric", "z_isobaric") else a
    return out


def _mirror(f, ncell, nvert):
    from mpas_dycore import isobaric as iso
    want = iso.cells({m: f[m][:ncell] for m in ("pressure_p", "pressure_base", "theta_m", "qv", "exner", "relhum", "uzonal",
                                                 "umeridional", "zgrid", "w")})
    info = want.pop("info")
    v = iso.vertices(f["pressure_p_img"], f["pressure_base_img"], f["vorticity"][:nvert], f["cellsOnVertex"][:nvert],
                     f["kiteAreasOnVertex"][:nvert], f["areaTriangle"][:nvert])
    v.pop("info")
    want.update(v)
    return want, info


def _compare(got, want, info, sl_c, sl_v, label):
    """got against want on the cells sl_c / vertices sl_v (slices of got; want and info cover exactly
    them), in the two classes.  Returns the measured maxima of the bounded class."""
    from mpas_dycore import isobaric as iso
    worst = {}
    for name, w in want.items():
        g = got[name][sl_v if name in iso.VERTEX_FIELDS else sl_c]
        assert np.all(np.isfinite(g)), f"{label} {name}: not finite"
        group = name.rsplit("_", 1)[0]
        if group == "dewpoint" or name == "mslp":
            soft = np.ones(w.shape, dtype=bool)
        elif group in ("height", "w"):
            soft = info["iface"]["uses_top"][:, iso.HPA.index(int(name.rsplit("_", 1)[1][:-3]))]
        elif name == "z_isobaric":
            soft = info["z_isobaric"]["uses_top"]
        else:
            soft = np.zeros(w.shape, dtype=bool)
        hard = ~soft
        assert np.array_equal(g[hard], w[hard]), \
            f"{label} {name}: not bit for bit on {np.count_nonzero(g[hard] != w[hard])} of {hard.sum()} values"
        if soft.any():
            err = rel_linf(g[soft], w[soft])
            worst[name] = err
            assert err <= BOUND, f"{label} {name}: rel Linf {err:.3e} > {BOUND:g}"
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print(f"{label}: bounded class, worst rel Linf " + ", ".join(f"{n} {e:.2e}" for n, e in top))
    return worst


def _untouched(after, before, what):
    from mpas_dycore import isobaric as iso
    for name, a in after.items():
        own = NVSOLVE if name in iso.VERTEX_FIELDS else NSOLVE
        assert np.array_equal(a[own:], before[name][own:]), f"{what} {name}: a halo element or the garbage slot was written"


@pytest.mark.parametrize("K", KS)
def test_kernels_against_compiled_reference(golden, K):
    """One mpas_dyc_isobaric_diagnostics, all bits on, against the compiled reference on the fixture's 40
    columns and 32 vertices and against the host restatement on the other owned elements.  K = 4: the k +- 2
    weights of pressure2 and compute_slp's klo / khi edge; 63: the 64 interfaces fill a wavefront; 64: the
    interfaces spill into a second chunk by one; 150: three chunks.
    Measured rel Linf on an MI355X (profiles/isobaric_new_tests.log), worst over the five K, bounded class
    (bound 1e-10): dewpoint_* 4.1e-16, mslp 2.9e-16, height_* / w_* / z_isobaric against the top interface
    2.8e-16; everything else bit for bit."""
    from mpas_dycore import isobaric as iso
    case = _case(K)
    cols, ref = iso.fixture_columns(golden, f"K{K}")
    nc, nfv = cols["theta_m"].shape[0], cols["vorticity"].shape[0]
    f = _fields(case, cols)
    dy = _standalone(case, f)
    before = _outputs(dy)
    dy.isobaric_diagnostics(1)
    after = _outputs(dy)
    levels = (dy.get_raw("diag", "t_iso_levels").copy(), dy.get_raw("diag", "z_iso_levels").copy())
    dy.close()
    want_all, info_all = _mirror(f, NSOLVE, NVSOLVE)
    # the fixture's elements against the reference (the restatement only says which class a value is in)
    info_fix = {k: {m: a[:nc] for m, a in v.items()} for k, v in info_all.items() if k in ("iface", "z_isobaric")}
    _compare(after, ref, info_fix, slice(0, nc), slice(0, nfv), f"K={K} fixture")
    rest = {n: a[(nfv if n in iso.VERTEX_FIELDS else nc):] for n, a in want_all.items()}
    info_rest = {k: {m: a[nc:] for m, a in v.items()} for k, v in info_all.items() if k in ("iface", "z_isobaric")}
    _compare(after, rest, info_rest, slice(nc, NSOLVE), slice(nfv, NVSOLVE), f"K={K} rest")
    _untouched(after, before, f"K={K}")
    for name, a in after.items():
        own = NVSOLVE if name in iso.VERTEX_FIELDS else NSOLVE
        assert not np.any(a[:own] == MARK), f"{name}: an owned element was not written"
    assert np.array_equal(levels[0], iso.T_ISO_LEVELS) and np.array_equal(levels[1], iso.Z_ISO_LEVELS)


def test_real_state_against_restatement():
    """The moist JW case at K = 26, ns = 3: after three steps and the shift, with a non-trivial relhum and
    all bits on, every output (the vertex ones included) against the restatement on the device's own
    fields, in the two classes."""
    from mpas_dycore import Dycore
    case = _case(26)
    n, nv, K = case["nCells"], case["nVertices"], 26
    dy = Dycore(case, device=0, moist_end=NS)
    dy.init_diagnostics(STEP_DT)
    for it in range(1, 4):
        dy.atm_timestep(STEP_DT, it)
        dy.shift_time_levels()
    dy.set_isobaric()
    kk, cc = np.meshgrid(np.arange(K), np.arange(n))
    relhum = 50.0 + 45.0 * np.sin(0.37 * cc + 0.9 * kk)
    dy.set("diag", "relhum", relhum)
    dy.isobaric_diagnostics(1)
    got = _outputs(dy)
    f = {"zgrid": np.asarray(case["zgrid"], dtype=np.float64), "relhum": relhum,
         "theta_m": dy.get("state", "theta_m", 1), "qv": dy.get("state", "scalars", 1)[:, :, 0].copy(),
         "w": dy.get("state", "w", 1), "exner": dy.get("diag", "exner"),
         "uzonal": dy.get("diag", "uReconstructZonal"), "umeridional": dy.get("diag", "uReconstructMeridional"),
         "vorticity": dy.get("diag", "vorticity"),
         "pressure_p_img": dy.get_raw("diag", "pressure_p").reshape(n + 1, K).copy(),
         "pressure_base_img": dy.get_raw("diag", "pressure_base").reshape(n + 1, K).copy()}
    dy.close()
    f["pressure_p"], f["pressure_base"] = f["pressure_p_img"][:-1], f["pressure_base_img"][:-1]
    cov = np.array(case["cellsOnVertex"], dtype=np.int64)
    f["cellsOnVertex"] = np.where(cov >= 0, cov, n)
    f["kiteAreasOnVertex"] = np.asarray(case["kiteAreasOnVertex"], dtype=np.float64)
    f["areaTriangle"] = np.asarray(case["areaTriangle"], dtype=np.float64)
    want, info = _mirror(f, n, nv)
    assert np.ptp(want["temperature_500hPa"]) > 1.0 and np.ptp(want["vorticity_500hPa"]) > 0.0 and want["mslp"].min() > 9.0e4
    _compare(got, want, info, slice(0, n), slice(0, nv), "JW x1.642x26 after 3 steps")


def test_four_blocks_equal_one_block():
    """Every output on the owned elements, mapped to global numbering, bit for bit: the call exchanges
    the halo of pressure_p, which the vertex pressure of an owned vertex reads.  The halo is spoilt first
    so that the exchange inside the call is what makes it right."""
    from mpas_dycore import Dycore, decomp, isobaric as iso
    case = _case(26)
    n, K = case["nCells"], 26
    kk, cc = np.meshgrid(np.arange(K), np.arange(n))
    relhum = 50.0 + 45.0 * np.sin(0.37 * cc + 0.9 * kk)

    def run(dy, blocks):
        dy.init_diagnostics(STEP_DT)
        for it in range(1, 3):
            dy.atm_timestep(STEP_DT, it)
            dy.shift_time_levels()
        dy.set_isobaric()
        for ib in range(dy.nblocks):
            rows = np.arange(n) if blocks is None else blocks[ib].glob["cell"]
            dy.set("diag", "relhum", relhum[rows], block=ib)
            if blocks is not None:  # spoil the halo of pressure_p
                own = blocks[ib].layer_end["cell"][0]
                img = dy.get_raw("diag", "pressure_p", block=ib).reshape(-1, K).copy()
                img[own:-1] = 777.0
                dy.set_raw("diag", "pressure_p", img, block=ib)
        dy.isobaric_diagnostics(1)
        out = [_outputs(dy, ib) for ib in range(dy.nblocks)]
        dy.close()
        return out

    one = run(Dycore(case, device=0, moist_end=NS), None)[0]
    blocks = decomp.decompose(case, decomp.partition_sfc(n, 4))
    four = run(Dycore.from_blocks(blocks, device=0, moist_end=NS), blocks)
    n_glob = {"cell": n, "vertex": case["nVertices"]}
    for name in iso.CELL_FIELDS + iso.VERTEX_FIELDS:
        loc = "vertex" if name in iso.VERTEX_FIELDS else "cell"
        got = decomp.gather_owned(blocks, [o[name][:-1] for o in four], loc, n_glob[loc])
        assert np.array_equal(got, one[name][:-1]), name


def _step_run(case, with_isobaric):
    from mpas_dycore import Dycore
    dy = Dycore(case, device=0, moist_end=NS)
    dy.init_diagnostics(STEP_DT)
    dy.use_graph(True)
    if with_isobaric:
        dy.set_isobaric()
    out = []
    for it in range(1, 4):
        dy.atm_timestep(STEP_DT, it)
        active, caps = dy.graph_active(), dy.graph_captures()
        dy.shift_time_levels()
        if with_isobaric:
            dy.isobaric_diagnostics(1)
        dy.synchronize()
        out.append(({m: dy.get("state", m, 1) for m in ("u", "w", "theta_m", "rho_zz", "scalars")}, active, caps))
    dy.close()
    return out


def test_structure():
    """Single bits write their own group only; mask 0 writes nothing; a context that never asked holds
    none of the fields; a run that calls the diagnostics between steps leaves the state's bits, the graph
    replay and the capture count as they are."""
    from mpas_dycore import Dycore, _lib, isobaric as iso
    case = _case(26)
    dy = Dycore(case, device=0, moist_end=NS)
    for name in iso.CELL_FIELDS + iso.VERTEX_FIELDS + ("relhum", "t_iso_levels", "z_iso_levels"):
        assert dy.field_bytes("diag", name) == 0, name
        assert not dy.lib.mpas_dyc_field_device_ptr(dy.h, b"diag", name.encode(), 1)
    dy.set_isobaric(0)
    assert dy.field_bytes("diag", "mslp") == 0
    dy.isobaric_diagnostics(1)                               # mask 0: nothing to do, nothing allocated
    assert dy.field_bytes("diag", "mslp") == 0
    dy.set("diag", "relhum", np.full((case["nCells"], 26), 40.0))     # a first set_field allocates the group
    assert dy.field_bytes("diag", "mslp") == 8 * (case["nCells"] + 1)
    assert dy.field_bytes("diag", "z_isobaric") == 8 * 13 * (case["nCells"] + 1)
    assert dy.field_bytes("diag", "vorticity_500hPa") == 8 * (case["nVertices"] + 1)
    assert dy.field_bytes("diag", "t_iso_levels") == 40 and not dy.get("diag", "mslp").any()
    assert np.array_equal(dy.get_raw("diag", "z_iso_levels"), iso.Z_ISO_LEVELS)
    dy.close()

    f = _fields(case)
    dy = _standalone(case, f, flags=0)
    before = _outputs(dy)
    dy.isobaric_diagnostics(1)
    after = _outputs(dy)
    for name in before:
        assert np.array_equal(after[name], before[name]), f"mask 0 wrote {name}"
    for i in range(12):
        bit = 1 << i
        dy.set_isobaric(bit)
        dy.isobaric_diagnostics(1)
        after = _outputs(dy)
        mine = iso.group_fields(bit)
        for name in after:
            own = NVSOLVE if name in iso.VERTEX_FIELDS else NSOLVE
            if name in mine:
                assert not np.any(after[name][:own] == MARK), f"bit {bit}: {name} not written"
                assert np.all(after[name][own:] == MARK), f"bit {bit}: {name} halo written"
            else:
                assert np.array_equal(after[name], before[name]), f"bit {bit} changed {name}"
        before = after
    # all bits at once give what the single bits gave
    dy.set_isobaric(_lib.ISO_ALL)
    _mark(dy)
    dy.isobaric_diagnostics(1)
    together = _outputs(dy)
    dy.close()
    for name in before:
        assert np.array_equal(together[name], before[name]), f"{name}: single bit and all bits differ"

    plain, with_iso = _step_run(case, False), _step_run(case, True)
    for it, ((s0, a0, c0), (s1, a1, c1)) in enumerate(zip(plain, with_iso)):
        assert a0 == a1 and c0 == c1, (it, a0, a1, c0, c1)
        for m in s0:
            assert np.array_equal(s0[m], s1[m]), f"step {it + 1} {m}"
    assert plain[-1][1] and plain[-1][2] == 2


def test_mslp_failure_path(golden):
    """Three of the extra K = 4 columns have no level 100 hPa above the ground: the owned mslp is all 0.0,
    as the reference returns it, and the other outputs are what they are without the failure."""
    from mpas_dycore import isobaric as iso
    case = _case(4)
    cols, ref = iso.fixture_columns(golden, "fail")
    nc, nfv = cols["theta_m"].shape[0], cols["vorticity"].shape[0]
    assert not ref["mslp"].any()
    f = _fields(case, cols)
    dy = _standalone(case, f)
    before = _outputs(dy)
    dy.isobaric_diagnostics(1)
    after = _outputs(dy)
    dy.close()
    assert not after["mslp"][:NSOLVE].any() and np.all(after["mslp"][NSOLVE:] == MARK)
    want_all, info_all = _mirror(f, NSOLVE, NVSOLVE)
    assert not want_all["mslp"].any() and info_all["slp"]["fail"].sum() == 3
    info_fix = {k: {m: a[:nc] for m, a in v.items()} for k, v in info_all.items() if k in ("iface", "z_isobaric")}
    _compare(after, ref, info_fix, slice(0, nc), slice(0, nfv), "failure set, fixture")
    info_own = {k: v for k, v in info_all.items() if k in ("iface", "z_isobaric")}
    _compare(after, want_all, info_own, slice(0, NSOLVE), slice(0, NVSOLVE), "failure set, owned")
    _untouched(after, before, "failure set")


def test_error_returns():
    import ctypes as C
    from mpas_dycore import Dycore, _lib
    from mpas_dycore.dycore import _make_dims
    case = _case(26)
    EINVAL, ESTATE = -1, -3
    dy = Dycore(case, device=0, moist_end=NS)
    lib, h = dy.lib, dy.h
    assert lib.mpas_dyc_set_isobaric(h, 4096) == EINVAL and lib.mpas_dyc_set_isobaric(h, -1) == EINVAL
    assert dy.field_bytes("diag", "mslp") == 0                                # the failures allocated nothing
    assert lib.mpas_dyc_isobaric_diagnostics(h, 0) == EINVAL and lib.mpas_dyc_isobaric_diagnostics(h, 3) == EINVAL
    # the vorticity group without areaTriangle
    assert lib.mpas_dyc_set_isobaric(h, _lib.ISO_VORTICITY) == 0
    assert lib.mpas_dyc_isobaric_diagnostics(h, 1) == ESTATE
    assert b"areaTriangle" in lib.mpas_dyc_last_error(h)
    dy.set_isobaric(_lib.ISO_VORTICITY)                                       # uploads the case's areaTriangle
    assert lib.mpas_dyc_isobaric_diagnostics(h, 1) == 0
    assert lib.mpas_dyc_isobaric_diagnostics(h, 2) == 0
    out = (C.c_double * 9)(*([-1.0] * 9))
    assert lib.mpas_dyc_get_profile(h, out, 8) == 0 and out[8] == -1.0        # out[8] only when n covers it
    assert dy.isobaric_diagnostics_ms(1) > 0.0
    dy.close()
    # between the step and finish_step under the host's microphysics
    dy = Dycore(case, device=0, moist_end=NS)
    dy.init_diagnostics(STEP_DT)
    dy.set_physics(tendencies=True, microphysics=True)
    dy.set_isobaric(_lib.ISO_MSLP)
    dy.atm_timestep(STEP_DT, 1)
    assert dy.lib.mpas_dyc_isobaric_diagnostics(dy.h, 2) == ESTATE
    dy.finish_step(STEP_DT)
    assert dy.lib.mpas_dyc_isobaric_diagnostics(dy.h, 2) == 0
    dy.close()
    # a host-only context keeps the mask, allocates nothing, and cannot run the diagnostics
    dims = _make_dims([case], [None], NS)
    cfg = _lib.make_config(case["config"])
    hh = C.c_void_p()
    assert lib.mpas_dyc_create_blocks(1, dims, C.byref(cfg), _lib.HOST_ONLY, C.byref(hh)) == 0
    try:
        assert lib.mpas_dyc_set_isobaric(hh, _lib.ISO_ALL) == 0
        assert lib.mpas_dyc_field_bytes(hh, b"diag", b"mslp") == 0
        assert lib.mpas_dyc_isobaric_diagnostics(hh, 1) == ESTATE
        assert lib.mpas_dyc_set_isobaric(hh, 1 << 12) == EINVAL
    finally:
        lib.mpas_dyc_destroy(hh)
