"""GPU: physics_get_tend on the device (mpas_dyc_set_todynamics / mpas_dyc_physics_get_tend, csrc/todynamics.hip).

1. the compiled reference's fixture (tests/golden/todynamics.npz) through the kernels, bit for bit;
2. the kernels against the numpy restatement (mpas_dycore.todynamics, pinned to the same fixture by
   tests/test_todynamics_host.py) at the level counts where the code takes another path;
3. the step with the hook against a step whose host couples with the restatement and uploads the four arrays
   (the path tests/test_gpu_physics.py pins to the compiled reference), bit for bit;
4. the same with IAU, device Kessler, LBCs and graph replay;
5. several blocks on every transport against one block;
6. the raw tendencies' device pointers: stable, and a write through one acts like set_field;
7. errors.
Every comparison is on the 64-bit patterns."""
import ctypes as C
import os

import numpy as np
import pytest

from mpas_dycore import fields as F
from mpas_dycore import todynamics as T
from test_forecast_case import partition
from test_gpu_forecast import ACTS, _dtr, _forecast, _set_lbc_pool

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "todynamics.npz")
NS7 = dict(index_qc=2, index_qr=3, index_qi=4, index_qs=5, index_ni=7)  # 1-based: qv qc qr qi qs qg ni
SET3 = dict(pbl="bl_mynn", convection="cu_ntiedtke", lw=True, sw=True)
SET4 = dict(convection="cu_kain_fritsch")
COUPLED = (("tend_physics", "tend_ru_physics"), ("tend_physics", "tend_rtheta_physics"),
           ("tend_physics", "tend_rho_physics"), ("tend", "scalars_tend"))
STATE = ("u", "w", "theta_m", "rho_zz", "scalars")
ESTATE = -3
_MEMO = {}


def _img(a):
    out = np.zeros((a.shape[0] + 1,) + a.shape[1:], dtype=np.float64)
    out[:-1] = a
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), f"{what}: {np.count_nonzero(g != w)} of {g.size} values differ in their bits"


with_vectors = T.with_vectors  # the case with east / north / edgeNormalVectors, which Dycore and set_todynamics upload


RAW_SCALE = 0.002  # of cases.raw_physics_forcing: its drying aloft then cools the top level by about 1.4 K per 5760 s step


def case7(K):
    """x1.642 with qv qc qr qi qs qg ni (moist_end = 6) and smooth raw tendencies."""
    from mpas_dycore.cases import jw_case, raw_physics_forcing
    if K not in _MEMO:
        case = with_vectors(jw_case(642, K, ns=7, moist=True, cache=False))
        _MEMO[K] = (case, raw_physics_forcing(case, RAW_SCALE))
    return _MEMO[K]


def idx0(idx1):
    """set_todynamics' 1-based indices (0: absent) -> the restatement's 0-based ones (index_qv = 0)."""
    return dict(index_qv=0, **{n: v - 1 for n, v in idx1.items()})


def upload_raw(dy, raw, blocks=None):
    for ib in range(dy.nblocks):
        for n, a in raw.items():
            dy.set_raw("tend_physics", n, _img(a if blocks is None else a[blocks[ib].glob["cell"]]), block=ib)


def host_coupling(dy, case, flags, idx, raw, tup=None):
    """The restatement on the context's own fields of time level 1."""
    return T.physics_get_tend(flags, idx, raw, dy.get("state", "rho_zz", 1), dy.get("diag", "rho_edge"),
                              dy.get("state", "theta_m", 1), dy.get("state", "scalars", 1), case, tup)


def device_outputs(dy):
    out = {n: dy.get_raw(p, n) for p, n in COUPLED}
    out.update({n: dy.get_raw("tend_physics", n) for n in T.EDGE_FIELDS})
    out["tend_u_phys"] = dy.get_raw("diag", "tend_u_phys")
    return out


# ---- 1. the fixture on the device ----
@pytest.mark.parametrize("K", T.FIXTURE_KS)
def test_fixture_on_the_device(K):
    from mpas_dycore import Dycore
    from mpas_dycore.cases import jw_dt, jw_len_disp
    from mpas_dycore.init_atm import build_case
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    lvl = T.FIXTURE_MESH_LEVEL
    m = T.fixture_mesh()
    assert np.array_equal(m["cellsOnEdge"], g["mesh_cellsOnEdge"])
    case = build_case(m, K=K, ns=T.FIXTURE_NUM_SCALARS, moist=True,
                      config=dict(config_len_disp=jw_len_disp(lvl), config_dt=jw_dt(lvl)))
    case.update({n: g[f"mesh_{n}"] for n in ("east", "north", "edgeNormalVectors")})
    nC, nE, ns = case["nCells"], case["nEdges"], T.FIXTURE_NUM_SCALARS
    assert ((nC + 1) * K) % 2 == K % 2  # the cell kernel's two forms
    dy = Dycore(case, device=0, moist_end=6)
    for n in ("rho_zz", "theta_m"):
        dy.set_raw("state", n, _img(g[f"{n}_K{K}"]), 1)
    dy.set_raw("state", "scalars", _img(g[f"scalars_K{K}"]), 1)
    dy.set_raw("diag", "rho_edge", _img(g[f"rho_edge_K{K}"]))
    upload_raw(dy, {n: g[f"{n}_K{K}"] for n in T.RAW_CELL})
    for name in T.FIXTURE_SETS:
        flags, idx, calls = T.fixture_set(name)
        for n in T.EDGE_FIELDS:  # the reference starts each set from zeroed edge arrays
            dy.set_raw("tend_physics", n, np.zeros((nE + 1, K)))
        dy.set_raw("diag", "tend_u_phys", np.zeros((nE + 1, K)))
        for p, n in COUPLED:  # what the call must overwrite everywhere, halo and garbage slot included
            dy.set_raw(p, n, np.full(dy.field_bytes(p, n) // 8, np.nan))
        one = {n: idx[n] + 1 for n in ("index_qc", "index_qr", "index_qi", "index_qs", "index_ni")}
        dy.set_todynamics(flags=flags, **one)
        if not flags:  # all off: the hook is off, and the call says so
            assert dy.lib.mpas_dyc_physics_get_tend(dy.h) == ESTATE
            continue
        for _ in range(calls):
            dy.physics_get_tend()
        dy.synchronize()
        got = device_outputs(dy)
        for n in T.FIXTURE_OUTPUTS:
            ref = g[f"ref_{name}_{n}_K{K}"]
            img = got[n].reshape((nC + 1, K, ns) if n == "scalars_tend" else (-1, K))
            _same(img[:-1], ref, f"K={K} {name} {n}")
            assert not np.any(_bits(img[-1])), f"K={K} {name} {n}: garbage slot is not +0.0"
    dy.close()


# ---- 2. shapes ----
@pytest.mark.parametrize("K", [4, 5, 26, 63, 64, 150])
def test_kernels_equal_the_restatement(K):
    """Even and odd (nCells + 1) K (643 cells + 1: even at K = 4, odd at 5), both sides of the one-wavefront
    limit (63 / 64), the edge kernel's 16-, 32- and 64-lane groups and its stride above 64 levels, one wide
    build.  Scheme sets 3 and 4."""
    from mpas_dycore import Dycore
    case, raw = case7(K)
    dt = float(case["dt"])
    dy = Dycore(case, device=0, moist_end=6)
    dy.init_diagnostics(dt)
    upload_raw(dy, raw)
    nC, nE = case["nCells"], case["nEdges"]
    assert ((nC + 1) * K) % 2 == K % 2
    for kw in (SET3, SET4):
        flags = T.scheme_flags(**kw)
        dy.set_raw("diag", "tend_u_phys", np.zeros((nE + 1, K)))
        dy.set_todynamics(**kw, **NS7)
        dy.physics_get_tend()
        dy.synchronize()
        want = host_coupling(dy, case, flags, idx0(NS7), raw)
        got = device_outputs(dy)
        for n in T.FIXTURE_OUTPUTS:
            if want[n] is None:
                continue
            img = got[n].reshape((nC + 1, K, 7) if n == "scalars_tend" else (-1, K))
            _same(img[:-1], want[n], f"K={K} {kw} {n}")
            assert not np.any(_bits(img[-1])), f"K={K} {kw} {n}: garbage slot"
        assert np.any(want["tend_rtheta_physics"]) and np.any(want["scalars_tend"][:, :, 1])
    dy.close()


# ---- 3. the step ----
def run_hook(K, nsteps, mode, rqv=True):
    """x1.642 x K, ns = 7, scheme set 3.  mode "device": set_todynamics, the raw tendencies uploaded once;
    "host": set_physics(tendencies) and before every step the restatement's four arrays from the context's own
    fields; "off": neither."""
    from mpas_dycore import Dycore
    case, raw = case7(K)
    dt = float(case["dt"])
    flags = T.scheme_flags(**SET3)
    dy = Dycore(case, device=0, moist_end=6)
    dy.init_diagnostics(dt)
    dy.use_graph(True)
    if mode == "device":
        dy.set_todynamics(**SET3, rqvdynten=rqv, **NS7)
        upload_raw(dy, raw)
    elif mode == "host":
        dy.set_physics(tendencies=True, rqvdynten=rqv)
    out = []
    for it in range(1, nsteps + 1):
        if mode == "host":
            dy.synchronize()
            t = host_coupling(dy, case, flags, idx0(NS7), raw)
            for p, n in COUPLED:
                dy.set_raw(p, n, _img(t[n]))
        dy.atm_timestep(dt, it)
        dy.shift_time_levels()
        dy.synchronize()
        s = {n: dy.get("state", n, 1) for n in STATE}
        if mode != "off":
            s["rqvdynten"] = dy.get("tend_physics", "rqvdynten")
        out.append(s)
    extra = dict(captures=dy.graph_captures(), active=dy.graph_active())
    dy.close()
    return out, extra


def test_step_with_the_hook_equals_the_host_coupled_step():
    a, ax = run_hook(26, 3, "device")
    b, _ = run_hook(26, 3, "host")
    off, ox = run_hook(26, 3, "off")
    assert ax["active"] and ax["captures"] == ox["captures"]  # one per buffer layout, as without the hook
    for it in range(3):
        for n in STATE + ("rqvdynten",):
            _same(a[it][n], b[it][n], f"step {it + 1} {n}")
            assert np.all(np.isfinite(a[it][n])), (it, n)
    assert np.any(a[2]["rqvdynten"])
    d = np.max(np.abs(a[2]["theta_m"] - off[2]["theta_m"])) / np.max(np.abs(off[2]["theta_m"]))
    print(f"hook on vs off after 3 steps: theta_m rel Linf {d:.3e}")
    assert d > ACTS == 1e-8


# ---- 4. with the other hooks ----
FORECAST_IDX = dict(index_qc=2, index_qr=3, index_qi=0, index_qs=0, index_ni=0)  # qv qc qr: no ice, no number


def run_forecast(mode, nsteps=4, upload_between=True, K=26):
    """cases.forecast_case(K) with IAU (window 2.5 dt: 3 forced steps, 1 free), device Kessler and LBCs in both
    modes, scheme set 3.  "device": the hook, graph replay; "host": set_physics(tendencies), the restatement's
    arrays before each step.  upload_between: a new rthratenlw between steps 2 and 3, in both alike."""
    from mpas_dycore import Dycore
    from mpas_dycore.cases import raw_physics_forcing
    case, lbc, inc, _ = _forecast(K)
    if "forecast_raw" not in _MEMO:
        _MEMO["forecast_raw"] = (with_vectors(case), raw_physics_forcing(case, 0.1))
    full, raw = _MEMO["forecast_raw"]
    raw = dict(raw)
    dt, window = float(case["dt"]), inc["window"]
    flags = T.scheme_flags(**SET3)
    dy = Dycore(dict(full, **{n: inc[n] for n in F.IAU_FIELD}), device=0, moist_end=3)
    _set_lbc_pool(dy, case, lbc, None)
    dy.init_diagnostics(dt)
    dy.use_graph(mode == "device")
    if mode == "device":
        dy.set_todynamics(**SET3, **FORECAST_IDX)
        upload_raw(dy, raw)
    else:
        dy.set_physics(tendencies=True)
    dy.set_iau(True, window)
    dy.set_microphysics("kessler", 2, 3, 0.0)
    out = []
    for it in range(1, nsteps + 1):
        if it == 3 and upload_between:
            raw["rthratenlw"] = raw["rthratenlw"] * -3.0
            if mode == "device":
                dy.set_raw("tend_physics", "rthratenlw", _img(raw["rthratenlw"]))
        if mode == "host":
            dy.synchronize()
            t = host_coupling(dy, full, flags, idx0(FORECAST_IDX), raw)
            for p, n in COUPLED:
                dy.set_raw(p, n, _img(t[n]))
        dy.set_lbc(True, _dtr(lbc, dt, it))
        dy.atm_timestep(dt, it)
        dy.shift_time_levels()
        dy.synchronize()
        out.append({n: dy.get("state", n, 1) for n in STATE})
        out[-1]["rainnc"] = dy.get("diag_physics", "rainnc")
    extra = dict(captures=dy.graph_captures(), active=dy.graph_active())
    dy.close()
    return out, extra


def test_hook_with_iau_kessler_lbc_and_graph_replay():
    a, ax = run_forecast("device")
    b, _ = run_forecast("host")
    plain, px = run_forecast("device", upload_between=False)
    assert ax["active"] and ax["captures"] == px["captures"], (ax, px)  # an upload captures nothing
    for it in range(4):
        for n in STATE + ("rainnc",):
            _same(a[it][n], b[it][n], f"step {it + 1} {n}")
            assert np.all(np.isfinite(a[it][n])), (it, n)
    for n in STATE:
        _same(a[1][n], plain[1][n], f"step 2 {n} (before the upload)")
    assert not np.array_equal(a[2]["theta_m"], plain[2]["theta_m"]), "the uploaded rthratenlw did not reach step 3"


# ---- 5. blocks ----
def block_partition(case, K):
    """test_forecast_case.partition; at an odd K with cell 0 moved to block 3, which then has an odd number of
    cells with an odd number owned: (nCells + 1) K is even, the cell kernel takes its two-value form, and the
    pair across the owned range's end holds one owned and one unowned element."""
    part = partition(case, K).copy()
    if K % 2:
        part[0] = 3
    return part


def run_blocks(transport, nsteps=3, K=26):
    """Scheme set 3 on the 4 blocks of block_partition (or one block: transport None); the raw wind tendencies
    of every block's halo cells are uploaded as NaN, so only the exchange can fill them.  First one eager
    physics_get_tend (its exchange runs outside a step) into coupled arrays filled with NaN: its results are
    element 0 of the list returned, and the unowned elements, the garbage slot included, must be +0.0."""
    from mpas_dycore import Dycore, decomp
    case, raw = case7(K)
    dt = float(case["dt"])
    n_glob = {"cell": case["nCells"], "edge": case["nEdges"]}
    if transport is None:
        blocks, nb = None, 1
        dy = Dycore(case, device=0, moist_end=6)
    else:
        blocks = decomp.decompose(case, block_partition(case, K))
        nb = len(blocks)
        if K % 2:
            assert any((b.solve[0] * K) % 2 == 1 and ((b.case["nCells"] + 1) * K) % 2 == 0 for b in blocks)
        assert nb >= 3 and all("east" in b.case and "edgeNormalVectors" in b.case for b in blocks)
        kw = {} if transport == "copies" else dict(comm_id=Dycore.comm_unique_id(), nranks=1, rank=0, rccl_local=True,
                                                   p2p=transport == "p2p")
        dy = Dycore.from_blocks(blocks, device=0, moist_end=6, **kw)
        if transport != "copies":
            dy.set_overlap(transport == "rccl")
    dy.init_diagnostics(dt)
    dy.use_graph(True)
    dy.set_todynamics(**SET3, **NS7)
    upload_raw(dy, raw, blocks)
    if blocks is not None:
        for ib, b in enumerate(blocks):
            for n in ("rublten", "rvblten", "rucuten", "rvcuten"):
                img = _img(raw[n][b.glob["cell"]])
                img[b.solve[0]:-1] = np.nan
                dy.set_raw("tend_physics", n, img, block=ib)

    def gather(pool, name, loc):
        if blocks is None:
            return dy.get(pool, name, 1)
        return decomp.gather_owned(blocks, [dy.get(pool, name, 1, block=i) for i in range(nb)], loc, n_glob[loc])

    def coupled():
        s = {n: gather(p, n, "edge" if n == "tend_ru_physics" else "cell") for p, n in COUPLED}
        s["tend_u_phys"] = gather("diag", "tend_u_phys", "edge")
        return s
    for ib in range(nb):
        for p, n in COUPLED:
            dy.set_raw(p, n, np.full(dy.field_bytes(p, n, block=ib) // 8, np.nan), block=ib)
    dy.physics_get_tend()
    dy.synchronize()
    for ib in range(nb):
        c = case if blocks is None else blocks[ib].case
        owned = (c["nCells"], c["nEdges"]) if blocks is None else blocks[ib].solve[:2]
        for p, n in COUPLED:
            edge = n == "tend_ru_physics"
            img = dy.get_raw(p, n, block=ib).reshape((c["nEdges"] if edge else c["nCells"]) + 1, -1)
            assert not np.any(_bits(img[owned[1] if edge else owned[0]:])), f"{transport} block {ib} {n}: unowned is not +0.0"
            assert np.all(np.isfinite(img)), f"{transport} block {ib} {n}"
    out = [coupled()]
    for it in range(1, nsteps + 1):
        dy.atm_timestep(dt, it)
        dy.shift_time_levels()
        dy.synchronize()
        s = {n: gather("state", n, "edge" if n == "u" else "cell") for n in STATE}
        s.update(coupled())
        out.append(s)
    dy.close()
    return out


@pytest.mark.parametrize("transport,K", [("copies", 26), ("rccl", 26), ("p2p", 26), ("copies", 27)])
def test_blocks_equal_one_block(transport, K):
    """The eager call, then three steps.  K = 27: a block whose owned range ends inside a pair of the cell kernel."""
    if ("one", K) not in _MEMO:
        _MEMO[("one", K)] = run_blocks(None, K=K)
    one = _MEMO[("one", K)]
    got = run_blocks(transport, K=K)
    for it in range(4):
        for n in one[it]:
            assert np.all(np.isfinite(got[it][n])), f"{transport} K={K} call {it} {n}: the halo exchange left a NaN"
            _same(got[it][n], one[it][n], f"{transport} K={K} call {it} (0: the eager call) {n}")
    assert np.any(one[0]["tend_rtheta_physics"]) and np.any(one[3]["tend_u_phys"]) and np.any(one[3]["tend_ru_physics"])


# ---- 6. zero-copy ----
def test_raw_tendency_pointers_are_stable_and_writable():
    import torch
    from mpas_dycore import Dycore
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    K = 26
    case, raw = case7(K)
    dt = float(case["dt"])
    new = _img(raw["rthblten"] * -2.0)
    runs = {}
    for mode in ("none", "set", "ptr"):
        dy = Dycore(case, device=0, moist_end=6)
        dy.init_diagnostics(dt)
        dy.use_graph(True)
        dy.set_todynamics(**SET3, **NS7)
        upload_raw(dy, raw)
        ptr = lambda: dy.lib.mpas_dyc_field_device_ptr(dy.h, b"tend_physics", b"rthblten", 1)  # noqa: E731
        p0 = ptr()
        assert p0
        for it in (1, 2):
            dy.atm_timestep(dt, it)
            dy.shift_time_levels()
        dy.synchronize()
        assert ptr() == p0, "tend_physics.rthblten moved"
        captures = dy.graph_captures()
        if mode == "set":
            dy.set_raw("tend_physics", "rthblten", new)
        elif mode == "ptr":  # a producer on the GPU: device to device from a torch tensor
            t = torch.from_numpy(new).to("cuda:0")
            torch.cuda.synchronize()
            assert t.numel() * 8 == dy.field_bytes("tend_physics", "rthblten")
            assert hip.hipMemcpy(C.c_void_p(p0), C.c_void_p(t.data_ptr()), t.numel() * 8, 3) == 0  # DeviceToDevice
        dy.atm_timestep(dt, 3)
        dy.shift_time_levels()
        dy.synchronize()
        assert dy.graph_captures() == captures and dy.graph_active()
        runs[mode] = {n: dy.get("state", n, 1) for n in STATE}
        dy.close()
    assert not np.array_equal(runs["none"]["theta_m"], runs["set"]["theta_m"])
    for n in STATE:
        _same(runs["ptr"][n], runs["set"][n], f"{n}: written through the pointer vs set_raw")


# ---- 7. errors ----
def test_errors():
    from mpas_dycore import Dycore, DycoreError
    from mpas_dycore.cases import jw_case
    K = 8
    case = jw_case(642, K, ns=7, moist=True, cache=False)   # no east / north / edgeNormalVectors
    dt = float(case["dt"])
    dy = Dycore(case, device=0, moist_end=6)
    dy.init_diagnostics(dt)
    assert dy.field_bytes("tend_physics", "rublten") == 0 and dy.field_bytes("mesh", "east") == 0  # held by none so far
    with pytest.raises(DycoreError, match="no scheme set"):
        dy.physics_get_tend()
    dy.set_todynamics(**SET3, **NS7)
    assert dy.field_bytes("tend_physics", "rublten") == (case["nCells"] + 1) * K * 8
    assert not np.any(dy.get_raw("tend_physics", "rthcuten")) and not np.any(dy.get_raw("diag", "tend_u_phys"))
    vec = with_vectors(case)
    for missing, have in (("mesh.east", ()), ("mesh.north", ("east",)), ("mesh.edgeNormalVectors", ("east", "north"))):
        for n in have[-1:]:
            dy.set("mesh", n, vec[n])
        for call in (dy.physics_get_tend, lambda: dy.atm_timestep(dt, 1)):
            with pytest.raises(DycoreError, match=rf"\(-3\).*{missing}"):
                call()
    dy.set("mesh", "edgeNormalVectors", vec["edgeNormalVectors"])
    dy.physics_get_tend()
    dy.set_todynamics(lw=True, **NS7)   # no wind flag: nothing to project
    dy.physics_get_tend()
    dy.set_raw("tend_physics", "rthratenlw", np.full((case["nCells"] + 1, K), 1e-6))
    dy.physics_get_tend()
    assert np.any(dy.get_raw("tend_physics", "tend_rtheta_physics"))
    dy.set_todynamics()                 # off: the coupled arrays go back to zeros
    for p, n in COUPLED:
        assert not np.any(_bits(dy.get_raw(p, n))), f"{n} after the hook went off"
    dy.set_todynamics(lw=True, **NS7)
    with pytest.raises(DycoreError, match=r"\(-3\)"):
        dy.set_physics(tendencies=True)
    with pytest.raises(DycoreError, match=r"\(-1\)"):
        dy.set_todynamics(flags=T.PBL_MYNN)
    # between mpas_dyc_timestep and mpas_dyc_finish_step (the host's microphysics): the setter is accepted, as
    # the other hooks' setters are; the call that enqueues work is refused, as theirs are
    dy.set_physics(tendencies=False, microphysics=True)
    dy.atm_timestep(dt, 1)
    with pytest.raises(DycoreError, match="finish_step"):
        dy.physics_get_tend()
    dy.set_todynamics(**SET4, **NS7)
    dy.finish_step(dt)
    dy.shift_time_levels()
    dy.physics_get_tend()
    dy.synchronize()
    assert np.all(np.isfinite(dy.get("state", "theta_m", 1)))
    dy.close()
