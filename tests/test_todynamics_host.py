"""physics_get_tend's numpy restatement (mpas_dycore.todynamics) against the compiled reference's results in
tests/golden/todynamics.npz (tools/make_todynamics_golden.py), the conditions that make the fixture tell a
changed association apart, the Python flag mapping, and the hook's host side on a host-only context: argument
errors, exclusivity with the host's coupled tendencies, and the exchange plan with and without the wind flags.
No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from mpas_dycore import _lib, decomp
from mpas_dycore import todynamics as T
from mpas_dycore.dycore import _make_dims, plan_exchanges

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "todynamics.npz")
EINVAL, ESTATE = -1, -3


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def fixture_inputs(g, K):
    mesh = {n: g[f"mesh_{n}"] for n in T.FIXTURE_MESH}
    raw = {n: g[f"{n}_K{K}"] for n in T.RAW_CELL}
    state = {n: g[f"{n}_K{K}"] for n in T.FIXTURE_STATE}
    return mesh, raw, state


def test_fixture_file_is_small_and_complete(golden):
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert tuple(golden["K"]) == T.FIXTURE_KS and int(golden["mesh_level"]) == T.FIXTURE_MESH_LEVEL
    assert any(K % 2 == 0 for K in T.FIXTURE_KS) and any(K % 2 == 1 for K in T.FIXTURE_KS)
    assert len(T.FIXTURE_SETS) == 9
    nC = golden["mesh_latCell"].size
    for K in T.FIXTURE_KS:
        assert golden[f"scalars_K{K}"].shape == (nC, K, T.FIXTURE_NUM_SCALARS)
        assert ((nC + 1) * K) % 2 == K % 2
        for n in T.RAW_CELL:  # realistic magnitude means both signs
            assert golden[f"{n}_K{K}"].min() < 0 < golden[f"{n}_K{K}"].max(), n


@pytest.mark.parametrize("K", T.FIXTURE_KS)
@pytest.mark.parametrize("name", list(T.FIXTURE_SETS))
def test_restatement_equals_the_compiled_reference(golden, name, K):
    mesh, raw, state = fixture_inputs(golden, K)
    host = T.fixture_run(name, raw, state, mesh)
    flags, _, _ = T.fixture_set(name)
    for n in T.FIXTURE_OUTPUTS:
        ref = golden[f"ref_{name}_{n}_K{K}"]
        got = np.zeros_like(ref) if host[n] is None else host[n]
        assert T.same_bits(got, ref), (name, K, n)
    assert (host["rublten_Edge"] is not None) == bool(flags & T.PBL)
    assert (host["rucuten_Edge"] is not None) == bool(flags & T.CU_WINDS)


def test_fixture_cases_show_what_they_are_for(golden):
    for K in T.FIXTURE_KS:
        ref = lambda name, n: golden[f"ref_{name}_{n}_K{K}"]  # noqa: E731
        for n in T.FIXTURE_OUTPUTS:
            assert not np.any(ref("off", n)), n
        # the accumulation: after two calls with the PBL off tend_u_phys is twice the projection
        e = ref("cu_tiedtke_twice", "rucuten_Edge")
        assert np.any(e) and T.same_bits(ref("cu_tiedtke_twice", "tend_u_phys"), (0.0 + e) + e)
        # an absent index_qi equals a zero rqiblten: qi's plane is zero, the rest is bl_ysu's but for qi's plane
        iqi = T.FIXTURE_INDICES["index_qi"]
        assert not np.any(ref("bl_ysu_no_qi", "scalars_tend")[:, :, iqi]) and np.any(ref("bl_ysu", "scalars_tend")[:, :, iqi])
        for n in ("tend_ru_physics", "tend_rtheta_physics", "tend_u_phys"):
            assert T.same_bits(ref("bl_ysu_no_qi", n), ref("bl_ysu", n))
        # untouched planes are 0.0: qg always, qr / qs outside cu_kain_fritsch, ni outside bl_mynn
        full = ref("bl_mynn_cu_ntiedtke_lw_sw", "scalars_tend")
        for i, touched in enumerate((True, True, False, True, False, False, True)):
            assert bool(np.any(full[:, :, i])) == touched, i
        kf = ref("cu_kain_fritsch", "scalars_tend")
        assert np.any(kf[:, :, 2]) and np.any(kf[:, :, 4]) and not np.any(kf[:, :, 6])
        assert not np.any(ref("bl_mynn_cu_ntiedtke_lw_sw", "tend_rho_physics"))


@pytest.mark.parametrize("K", T.FIXTURE_KS)
def test_fixture_tells_a_changed_association_apart(golden, K):
    mesh, raw, state = fixture_inputs(golden, K)
    name = "bl_mynn_cu_ntiedtke_lw_sw"
    ref = lambda n: golden[f"ref_{name}_{n}_K{K}"]  # noqa: E731
    share = lambda a, b: float(np.mean(np.ascontiguousarray(a).view(np.int64) != np.ascontiguousarray(b).view(np.int64)))  # noqa: E731
    a = T.fixture_run(name, raw, state, mesh, T.variant_theta_m_right)["tend_rtheta_physics"]
    b = T.fixture_run(name, raw, state, mesh, T.variant_theta_sum_first)["tend_rtheta_physics"]
    c = T.fixture_run(name, raw, state, mesh, T.variant_dot_right)
    shares = dict(theta_m_right=share(a, ref("tend_rtheta_physics")), theta_sum_first=share(b, ref("tend_rtheta_physics")),
                  dot_right=share(np.stack([c["rublten_Edge"], c["rucuten_Edge"]]),
                                  np.stack([ref("rublten_Edge"), ref("rucuten_Edge")])))
    print(f"K{K}: shares that differ with one association changed: {shares}")
    for n, v in shares.items():
        assert v >= T.MIN_SENSITIVE_SHARE == 0.10, (K, n, v)


def test_init_dirs_gives_orthogonal_unit_vectors(golden):
    east, north = T.init_dirs(golden["mesh_latCell"], golden["mesh_lonCell"])
    assert np.array_equal(east, golden["mesh_east"]) and np.array_equal(north, golden["mesh_north"])
    eps = np.finfo(np.float64).eps
    for v in (east, north):
        assert np.max(np.abs(np.sum(v * v, axis=1) - 1.0)) <= 4 * eps
    assert np.max(np.abs(np.sum(east * north, axis=1))) <= 4 * eps
    assert not np.any(east[:, 2])
    # east x north points outwards
    lat, lon = golden["mesh_latCell"], golden["mesh_lonCell"]
    up = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], axis=1)
    assert np.max(np.abs(np.cross(east, north) - up)) <= 8 * eps


def test_scheme_names_map_to_flags():
    f = T.scheme_flags
    assert f() == 0 and f("off", "off", "off", "off") == 0
    assert f("bl_ysu") == T.PBL == _lib.TODYN_PBL
    assert f("bl_mynn") == T.PBL | T.PBL_MYNN == _lib.TODYN_PBL | _lib.TODYN_PBL_MYNN
    assert f(convection="cu_kain_fritsch") == T.CU | T.CU_KF == _lib.TODYN_CU | _lib.TODYN_CU_KF
    assert f(convection="cu_tiedtke") == f(convection="cu_ntiedtke") == T.CU | T.CU_WINDS == _lib.TODYN_CU | _lib.TODYN_CU_WINDS
    assert f(convection="cu_grell_freitas") == T.CU
    assert f(lw=True) == T.LW == _lib.TODYN_LW and f(sw="rrtmg_sw") == T.SW == _lib.TODYN_SW
    assert f(lw="off", sw=False) == 0
    assert f("bl_mynn", "cu_ntiedtke", True, True, rqvdynten=True) == 1 + 2 + 4 + 16 + 32 + 64 + 128
    assert T.RQVDYNTEN == _lib.TODYN_RQVDYNTEN and T.ALL == _lib.TODYN_ALL == 255
    with pytest.raises(ValueError, match="config_pbl_scheme"):
        f("bl_nope")
    with pytest.raises(ValueError, match="config_convection_scheme"):
        f(convection="cu_kf")


@pytest.fixture(scope="module")
def case7():
    from mpas_dycore.cases import jw_case
    return jw_case(642, 8, ns=7, moist=True, cache=False)


@pytest.fixture()
def host_ctx(case7):
    lib = _lib.load()
    dims = _make_dims([case7], [None], 6)
    cfg = _lib.make_config(case7["config"])
    h = C.c_void_p()
    assert lib.mpas_dyc_create_blocks(1, dims, C.byref(cfg), _lib.HOST_ONLY, C.byref(h)) == 0
    yield lib, h
    lib.mpas_dyc_destroy(h)


def test_set_todynamics_argument_errors(host_ctx):
    lib, h = host_ctx
    st = lambda flags, *idx: lib.mpas_dyc_set_todynamics(h, flags, *(idx or (2, 3, 4, 5, 7)))  # noqa: E731
    assert lib.mpas_dyc_set_todynamics(None, 1, 2, 3, 4, 5, 7) == EINVAL
    assert st(256) == EINVAL and st(-1) == EINVAL                                   # unknown bits
    assert b"unknown flag" in lib.mpas_dyc_last_error(h)
    assert st(T.PBL_MYNN) == EINVAL                                                 # a sub-flag without its parent
    assert st(T.CU_KF) == EINVAL and st(T.CU_WINDS) == EINVAL and st(T.PBL | T.CU_KF) == EINVAL
    assert st(T.CU | T.CU_KF | T.CU_WINDS) == EINVAL                                # Kain-Fritsch has no wind tendencies
    assert st(T.PBL, 8, 3, 4, 5, 7) == EINVAL and st(T.PBL, 2, 3, 4, 5, 8) == EINVAL  # above num_scalars = 7
    assert st(T.PBL, 1, 3, 4, 5, 7) == EINVAL and st(T.PBL, 2, 3, 1, 5, 7) == EINVAL  # equal to index_qv = 1
    assert b"index" in lib.mpas_dyc_last_error(h)
    assert st(T.PBL, 0, 0, 0, 0, 0) == 0 and st(T.PBL, -1, 3, -5, 5, 7) == 0          # absent scalars
    for name in T.FIXTURE_SETS:
        assert st(T.fixture_set(name)[0]) == 0, name
    assert st(T.ALL & ~T.CU_KF) == 0 and st(0) == 0
    assert lib.mpas_dyc_physics_get_tend(h) == ESTATE                                # no fields on a host-only context
    assert lib.mpas_dyc_physics_get_tend(None) == EINVAL


def test_exclusive_with_the_hosts_coupled_tendencies(host_ctx):
    lib, h = host_ctx
    TEND, RQV, MICRO = 1, 2, 4
    assert lib.mpas_dyc_set_todynamics(h, T.PBL, 2, 3, 4, 5, 7) == 0
    assert lib.mpas_dyc_set_physics(h, TEND) == ESTATE and b"set_todynamics" in lib.mpas_dyc_last_error(h)
    assert lib.mpas_dyc_set_physics(h, TEND | RQV) == ESTATE
    assert lib.mpas_dyc_set_physics(h, MICRO) == 0 and lib.mpas_dyc_set_physics(h, 0) == 0   # the host's microphysics may stay
    assert lib.mpas_dyc_set_todynamics(h, 0, 0, 0, 0, 0, 0) == 0
    assert lib.mpas_dyc_set_physics(h, TEND) == 0                                    # the other order
    assert lib.mpas_dyc_set_todynamics(h, T.LW, 2, 3, 4, 5, 7) == ESTATE
    assert b"MPAS_DYC_PHYSICS_TENDENCIES" in lib.mpas_dyc_last_error(h)
    assert lib.mpas_dyc_set_todynamics(h, 0, 0, 0, 0, 0, 0) == 0                     # off is always allowed
    assert lib.mpas_dyc_set_physics(h, 0) == 0
    assert lib.mpas_dyc_set_todynamics(h, T.LW, 2, 3, 4, 5, 7) == 0


def test_exchange_plan_with_and_without_the_wind_flags(case7):
    """Two blocks on two ranks: the wind flags add one exchange point per step (mpas_dyc_plan_exchanges runs
    two steps) with the raw wind tendencies' cell-halo messages; without them the plan is the plain one."""
    part = decomp.partition_sfc(case7["nCells"], 2)
    dt = float(case7["dt"])

    def plan(flags):
        blocks, placement = decomp.rank_blocks(case7, 2, 0, 1, cell_part=part)
        return plan_exchanges(blocks, placement, 0, 2, dt, moist_end=6, todynamics=flags)
    msgs0, keys0 = plan(0)
    for flags in (T.LW | T.SW, T.CU | T.CU_KF, T.CU, T.RQVDYNTEN | T.LW):
        msgs, keys = plan(flags)
        assert keys == keys0 and np.array_equal(msgs, msgs0), flags
    assert not any("blten" in k or "cuten" in k for k in keys0)
    cell_halo = next(m["count"] for m in msgs0[msgs0["direction"] == _lib.RECV])  # noqa: F841
    for flags, names in ((T.PBL, ("rublten", "rvblten")), (T.CU | T.CU_WINDS, ("rucuten", "rvcuten")),
                         (T.PBL | T.CU | T.CU_WINDS, ("rublten", "rvblten", "rucuten", "rvcuten"))):
        msgs, keys = plan(flags)
        new = [i for i, k in enumerate(keys) if "blten" in k or "cuten" in k]
        assert len(new) == 2 and len(keys) == len(keys0) + 2, (flags, keys)
        assert [k for i, k in enumerate(keys) if i not in new] == keys0
        for i in new:
            for n in ("rublten", "rvblten", "rucuten", "rvcuten"):
                assert (n in keys[i]) == (n in names), (flags, keys[i])
            m = msgs[msgs["point"] == i]
            assert set(m["direction"]) == {_lib.SEND, _lib.RECV} and np.all(m["peer_rank"] == 1)
        rest = msgs[~np.isin(msgs["point"], new)].copy()
        for i in sorted(new, reverse=True):
            rest["point"][rest["point"] > i] -= 1
        assert np.array_equal(rest, msgs0)
