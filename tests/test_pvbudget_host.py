"""The PV budget's numpy restatement (mpas_dycore.pvbudget) against the compiled reference's results in
tests/golden/pvbudget.npz (tools/make_pvbudget_golden.py), what the fixture shows (sources that are off, the two
summation orders that matter), the Python flag mapping, and mpas_dyc_set_pv_budget on a host-only context.
Everything is + - * /, so every comparison is bit for bit.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from mpas_dycore import _lib
from mpas_dycore import pvbudget as B
from mpas_dycore.dycore import _make_dims

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pvbudget.npz")
EINVAL, ESTATE = -1, -3


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def mesh():
    return B.fixture_mesh()


@pytest.fixture(scope="module")
def restated(golden, mesh):
    """The restatement of every (K, source set), computed once."""
    out = {}
    for K in B.FIXTURE_KS:
        for name, flags in B.FIXTURE_SETS.items():
            f, ilev, _ = B.fixture_state(golden, K, name)
            out[K, name] = B.fixture_driver(mesh, f, flags, ilev=ilev)
    return out


def test_fixture_file_is_small_and_complete(golden, mesh):
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert tuple(golden["K"]) == B.FIXTURE_KS and int(golden["mesh_level"]) == B.FIXTURE_MESH_LEVEL
    assert 4 in B.FIXTURE_KS and 65 in B.FIXTURE_KS                  # one past the kernel's 64-level chunk
    assert set(B.FIXTURE_SETS.values()) == {B.ALL, B.ON, B.ON | B.LW | B.CU}
    n, ne = mesh["nCells"], mesh["nEdges"]
    assert np.count_nonzero(mesh["nEdgesOnCell"] == 5) == 12
    for K in B.FIXTURE_KS:
        for name in B.FIXTURE_FIELDS:
            a = golden[f"{name}_K{K}"]
            assert a.dtype == np.float32 and np.all(np.isfinite(a)), name
        for name in B.FIXTURE_CELL_FIELDS + B.FIXTURE_EDGE_FIELDS[:2]:   # the tendencies: zero-mean, both signs
            a = golden[f"{name}_K{K}"].astype(np.float64)
            assert a.shape[0] == (ne if name in B.FIXTURE_EDGE_FIELDS else n)
            assert (a > 0).any() and (a < 0).any() and abs(a.mean()) < 1.0e-3 * np.abs(a).max(), name
        ilev = golden[f"iLev_DT_K{K}"]
        assert ilev.shape == (n,) and {0, 1, 2, K, K + 1} <= set(ilev.tolist()) and ilev[0] != 1
        if n >= K + 2:
            assert set(ilev.tolist()) == set(range(K + 2))
        for n3 in B.OUT_3D:
            assert golden[f"ref_all_{n3}_K{K}"].shape == (n, K - 1)
        for name in ("none", "lwcu"):
            for n3 in B.FIXTURE_SET_FIELDS:
                assert f"ref_{name}_{n3}_K{K}" in golden, (name, n3)


@pytest.mark.parametrize("K", B.FIXTURE_KS)
@pytest.mark.parametrize("name", list(B.FIXTURE_SETS))
def test_restatement_equals_the_compiled_reference(golden, restated, name, K):
    _, _, ref = B.fixture_state(golden, K, name)
    host = restated[K, name]
    for n in B.OUT_3D:
        assert np.array_equal(host[n][:, :K - 1], ref[n]), f"{n} below level K"
        assert np.all(np.isfinite(host[n]))
    assert np.array_equal(host["dtheta_dt_mix"], ref["dtheta_dt_mix"])
    for n in B.OUT_2D:
        assert np.array_equal(host[n], ref[n]), n
    assert np.ptp(ref["depv_dt_fric"]) > 0 and np.ptp(ref["depv_dt_diab"]) > 0


@pytest.mark.parametrize("K", B.FIXTURE_KS)
def test_a_source_that_is_off_gives_exact_zeros(golden, restated, K):
    ref = {name: B.fixture_state(golden, K, name)[2] for name in B.FIXTURE_SETS}
    for got in (ref, {name: {n: restated[K, name][n][:, :K - 1] for n in B.OUT_3D} for name in B.FIXTURE_SETS}):
        for n in ("depv_dt_lw", "depv_dt_sw", "depv_dt_bl", "depv_dt_cu"):
            assert got["all"][n].any()
            assert not got["none"][n].any(), n
        assert got["lwcu"]["depv_dt_lw"].any() and got["lwcu"]["depv_dt_cu"].any()
        assert not got["lwcu"]["depv_dt_sw"].any() and not got["lwcu"]["depv_dt_bl"].any()
        # depv_dt_mix is guarded by dtheta_dt_mp's association (:1460): with no raw tendency both are still there
        none = got["none"]
        assert none["depv_dt_mp"].any() and none["depv_dt_mix"].any()
        assert np.array_equal(none["depv_dt_diab"], none["depv_dt_mp"] + none["depv_dt_mix"])


@pytest.mark.parametrize("K", B.FIXTURE_KS)
def test_the_two_summation_orders_matter(golden, mesh, K):
    """The curl in edgesOnVertex order and the sum from mix down to lw each change the share of elements that the
    tool recorded: the fixture tells both apart."""
    f, ilev, ref = B.fixture_state(golden, K)
    by_slot = B.fixture_driver(mesh, f, B.ALL, ilev=ilev, curl_order="edgesOnVertex")
    reverse = B.fixture_driver(mesh, f, B.ALL, ilev=ilev, reverse_sum=True)
    share_curl = float(np.mean(by_slot["depv_dt_fric"][:, :K - 1] != ref["depv_dt_fric"]))
    share_sum = float(np.mean(reverse["depv_dt_diab"][:, :K - 1] != ref["depv_dt_diab"]))
    assert share_curl == float(golden[f"share_curl_K{K}"]) > 0
    assert share_sum == float(golden[f"share_sum_K{K}"]) > 0
    # each variant changes its own term only
    assert np.array_equal(by_slot["depv_dt_diab"][:, :K - 1], ref["depv_dt_diab"])
    assert np.array_equal(reverse["depv_dt_fric"][:, :K - 1], ref["depv_dt_fric"])


def test_flag_mapping():
    from mpas_dycore import todynamics as T
    assert (B.ON, B.LW, B.SW, B.BL, B.CU, B.ALL) == (_lib.PVB_ON, _lib.PVB_LW, _lib.PVB_SW, _lib.PVB_BL, _lib.PVB_CU,
                                                     _lib.PVB_ALL) == (1, 2, 4, 8, 16, 31)
    assert B.flags_from_todynamics(0) == 0
    assert B.flags_from_todynamics(T.PBL | T.PBL_MYNN) == B.BL and B.flags_from_todynamics(T.CU | T.CU_WINDS) == B.CU
    assert B.flags_from_todynamics(T.LW | T.SW | T.RQVDYNTEN) == B.LW | B.SW
    assert B.flags_from_todynamics(T.ALL) | B.ON == B.ALL
    for bad in (32, B.LW, B.ALL + 32):
        with pytest.raises(ValueError):
            B.check_flags(bad)
    B.check_flags(0), B.check_flags(B.ON), B.check_flags(B.ALL)


@pytest.fixture()
def host_ctx():
    from mpas_dycore.cases import jw_case
    case = jw_case(642, 8, ns=1, cache=False)
    lib = _lib.load()
    dims = _make_dims([case], [None], 1)
    cfg = _lib.make_config(case["config"])
    h = C.c_void_p()
    assert lib.mpas_dyc_create_blocks(1, dims, C.byref(cfg), _lib.HOST_ONLY, C.byref(h)) == 0
    yield lib, h
    lib.mpas_dyc_destroy(h)


def test_set_pv_budget_errors_on_a_host_only_context(host_ctx):
    lib, h = host_ctx
    assert lib.mpas_dyc_set_pv_budget(None, 0) == EINVAL
    assert lib.mpas_dyc_set_pv_budget(h, 0) == 0                     # 0 is always allowed
    assert lib.mpas_dyc_set_pv_budget(h, 32) == EINVAL and b"unknown" in lib.mpas_dyc_last_error(h)
    assert lib.mpas_dyc_set_pv_budget(h, B.ALL | 64) == EINVAL
    for src in (B.LW, B.SW, B.BL, B.CU, B.LW | B.CU):                # a source bit without ON
        assert lib.mpas_dyc_set_pv_budget(h, src) == EINVAL and b"MPAS_DYC_PVB_ON" in lib.mpas_dyc_last_error(h)
    # ON needs the PV diagnostics, whose outputs the budget reads
    assert lib.mpas_dyc_set_pv_budget(h, B.ON) == ESTATE and b"mpas_dyc_set_pv" in lib.mpas_dyc_last_error(h)
    assert lib.mpas_dyc_set_pv_budget(h, B.ALL) == ESTATE
    assert lib.mpas_dyc_set_pv(h, 1) == 0
    for flags in (B.ON, B.ON | B.LW | B.CU, B.ALL, 0):
        assert lib.mpas_dyc_set_pv_budget(h, flags) == 0
    assert lib.mpas_dyc_set_pv_budget(h, B.ALL) == 0
    # a host-only context keeps the mask, allocates nothing and cannot run the diagnostics
    assert lib.mpas_dyc_field_bytes(h, b"diag", b"depv_dt_diab") == 0
    assert lib.mpas_dyc_pv_budget_diagnostics(h, 1) == ESTATE
    assert lib.mpas_dyc_pv_budget_diagnostics(h, 0) == EINVAL and lib.mpas_dyc_pv_budget_diagnostics(None, 1) == EINVAL
    assert lib.mpas_dyc_set_pv(h, 0) == 0
    assert lib.mpas_dyc_set_pv_budget(h, B.ON) == ESTATE and lib.mpas_dyc_set_pv_budget(h, 0) == 0
