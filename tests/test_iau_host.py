"""Incremental analysis update, host side (no GPU): the weight of a step (atm_iau_coef,
mpas_atm_iau.F:22-78) on a planner-only context, the `iau` stream file (Registry.xml:1092-1102)
through mpas_files.read_iau / write_iau, and the increments' way through the block decomposition."""
import ctypes as C

import numpy as np
import pytest

from mpas_dycore import _lib, decomp, mpas_files
from mpas_dycore.cases import jw_case
from mpas_dycore.dycore import _make_dims

EINVAL, ESTATE = -1, -3


@pytest.fixture(scope="module")
def case():
    return jw_case(642, K=8, ns=3, moist=True, cache=False)


def _increments(case, seed=11):
    rng = np.random.default_rng(seed)
    nC, nE, K, ns = case["nCells"], case["nEdges"], case["nVertLevels"], case["num_scalars"]
    return dict(u_amb=rng.standard_normal((nE, K)), theta_amb=rng.standard_normal((nC, K)),
                rho_amb=1e-2 * rng.standard_normal((nC, K)), scalars_amb=1e-4 * rng.standard_normal((nC, K, ns)))


def _host_only(case):
    lib = _lib.load()
    dims = _make_dims([case], [None], 3)
    cfg = _lib.make_config(case["config"])
    h = C.c_void_p()
    assert lib.mpas_dyc_create_blocks(1, dims, C.byref(cfg), _lib.HOST_ONLY, C.byref(h)) == 0
    return lib, h


def _weight(lib, h, dt, it):
    w = C.c_double(-1.0)
    assert lib.mpas_dyc_iau_weight(h, dt, it, C.byref(w)) == 0
    return w.value


def test_iau_weight_on_a_host_only_context(case):
    lib, h = _host_only(case)
    try:
        # off (the default): no step is forced
        assert [_weight(lib, h, 180.0, it) for it in range(1, 6)] == [0.0] * 5
        # window / dt = 2.5: nint rounds the half away from zero, so three steps are forced (C's
        # nearbyint and Python's round give 2)
        assert lib.mpas_dyc_set_iau(h, 1, 450.0) == 0
        assert [_weight(lib, h, 180.0, it) for it in range(1, 5)] == [1.0 / 450.0] * 3 + [0.0]
        assert lib.mpas_dyc_set_iau(h, 1, 0.0) == EINVAL
        assert lib.mpas_dyc_set_iau(h, 1, -5.0) == EINVAL
        assert [_weight(lib, h, 180.0, it) for it in range(1, 5)] == [1.0 / 450.0] * 3 + [0.0]  # kept
        assert _weight(lib, h, 100.0, 4) == 1.0 / 450.0 and _weight(lib, h, 100.0, 5) == 1.0 / 450.0  # nint(4.5) = 5
        assert _weight(lib, h, 100.0, 6) == 0.0
        assert lib.mpas_dyc_set_iau(h, 0, 0.0) == 0
        assert [_weight(lib, h, 180.0, it) for it in range(1, 5)] == [0.0] * 4
        # the pool exists by name, but a planner-only context holds no fields
        buf = np.zeros((case["nEdges"] + 1) * case["nVertLevels"])
        assert lib.mpas_dyc_field_bytes(h, b"tend_iau", b"u") == buf.nbytes
        assert lib.mpas_dyc_set_field(h, b"tend_iau", b"u", 1, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == ESTATE
        assert lib.mpas_dyc_get_field(h, b"tend_iau", b"u", 1, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == ESTATE
    finally:
        lib.mpas_dyc_destroy(h)


@pytest.mark.parametrize("version", [2, 5])
def test_iau_file_roundtrip(tmp_path, case, version):
    inc = _increments(case)
    names = ["qv", "qc", "qr"]
    p = str(tmp_path / f"x1.642.AmB.v{version}.nc")
    mpas_files.write_iau(p, inc["u_amb"], inc["theta_amb"], inc["rho_amb"], inc["scalars_amb"], names, version=version)
    from mpas_dycore import ncio
    raw = ncio.read(p)
    assert raw.version == version and raw.dims["Time"] == 1
    assert raw.vars["qc_amb"].dims == ("Time", "nCells", "nVertLevels")
    got = mpas_files.read_iau(p, names)
    assert sorted(got) == sorted(inc)
    for n in inc:  # the case's element order: no reordering on the way
        assert got[n].shape == inc[n].shape and np.array_equal(got[n], inc[n]), n
    # a file without qr_amb (its package was inactive): that constituent reads back as zeros
    q = str(tmp_path / f"x1.642.AmB.noqr.v{version}.nc")
    mpas_files.write_iau(q, inc["u_amb"], inc["theta_amb"], inc["rho_amb"], inc["scalars_amb"], ["qv", "qc", None],
                         version=version)
    assert "qr_amb" not in ncio.read(q)
    got = mpas_files.read_iau(q, names)
    assert np.array_equal(got["scalars_amb"][:, :, :2], inc["scalars_amb"][:, :, :2])
    assert got["scalars_amb"].shape == inc["scalars_amb"].shape and not got["scalars_amb"][:, :, 2].any()
    for n in ("u_amb", "theta_amb", "rho_amb"):
        assert np.array_equal(got[n], inc[n]), n


def test_decompose_slices_the_increments(case):
    from mpas_dycore import fields as F
    inc = _increments(case, seed=5)
    full = dict(case, **inc)
    blocks = decomp.decompose(full, decomp.partition_sfc(case["nCells"], 4))
    n_glob = {"cell": case["nCells"], "edge": case["nEdges"]}
    for n, a in inc.items():
        loc = F.LOCATION[n]
        per = [b.case[n] for b in blocks]
        for b, s in zip(blocks, per):  # owned and halo elements of the block, in its local order
            assert s.shape == (b.glob[loc].size,) + a.shape[1:] and np.array_equal(s, a[b.glob[loc]]), n
        assert np.array_equal(decomp.gather_owned(blocks, per, loc, n_glob[loc]), a), n
    assert set(F.IAU_FIELD) == set(inc) and set(F.IAU_FIELD.values()) == {"u", "theta", "rho", "scalars"}
