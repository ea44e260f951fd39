"""GPU: cape, cin, storm-relative helicity and the surface / 1 km / 6 km fields on the device
(mpas_dyc_set_convective / mpas_dyc_convective_diagnostics, convcompute.hip).

Yardsticks, strongest first:
* the kernels against the compiled reference: the columns of tests/golden/convective_columns.npz go into the
  first owned cells of an x1.642 context of 130 owned cells (two full blocks of the ascent kernel and a
  two-lane tail), and the expected fields are what the reference's own convective_diagnostics.F computed;
* the other owned cells (mpas_dycore.convcompute.synthetic_fields: unstable soundings) against the host
  restatement, pinned to the same fixture bit for bit by tests/test_convcompute_host.py;
* structure: mask 0, single bits with the reference's quirks, the lazily allocated group, the step
  untouched, four blocks against one, the error returns.
Two classes of outputs.  cape, cin and dewpoint_surface pass through the device library's exp / log / pow:
rel Linf <= 1e-10, the project's parity bound, on the columns the restatement classifies as stable (their
discrete decisions do not move under a 4 ulp drift of those functions; the classification never looks at
the device's output); borderline columns, at most 2 % of those compared, must be finite with cape, cin >= 0.
The other nine written outputs are + - * / and sqrt on inputs the device holds exactly: bit for bit.
"""
import os

import numpy as np
import pytest

from conftest import rel_linf

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convective_columns.npz")
NS = 3
NSOLVE = 130
MARK = 12345.678
BOUND = 1e-10
STEP_DT = 600.0
KS = (4, 26, 64, 150)
_CASES, _WANT = {}, {}


def _case(K):
    from mpas_dycore.cases import jw_case
    if K not in _CASES:
        _CASES[K] = jw_case(642, K=K, ns=NS, moist=True, cache=False)
    return _CASES[K]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _img(a):
    out = np.zeros((a.shape[0] + 1,) + a.shape[1:], dtype=a.dtype)
    out[:-1] = a
    return out


def _fields(K, golden=None):
    """synthetic_fields of the case with the fixture's columns (if any) in the first cells; the restatement
    of the owned cells and their classification, computed once per K and left unchanged."""
    from mpas_dycore import convcompute as cc
    key = (K, golden is not None)
    if key not in _WANT:
        f = cc.synthetic_fields(_case(K), K)
        ref = None
        if golden is not None:
            cols, ref = cc.fixture_columns(golden, f"K{K}")
            for name in cc.INPUTS:
                f[name][:cols[name].shape[0]] = cols[name]
        base, stable, _ = cc.classify({name: f[name][:NSOLVE] for name in cc.INPUTS})
        _WANT[key] = (f, ref, base, stable)
    return _WANT[key]


def _standalone(case, f, flags=None, mark=True):
    """A context of NSOLVE owned cells holding f on time level 1, the group allocated, a marker in every output."""
    from mpas_dycore import Dycore, _lib
    n, K = case["nCells"], case["nVertLevels"]
    dy = Dycore(case, device=0, moist_end=NS, solve=(NSOLVE, case["nEdges"], case["nVertices"]))
    dy.set("mesh", "zgrid", f["zgrid"])
    sc = np.zeros((n, K, NS))
    sc[:, :, 0] = f["qv"]
    dy.set_raw("state", "scalars", _img(sc), 1)
    dy.set_raw("state", "theta_m", _img(f["theta_m"]), 1)
    for name, fld in (("exner", "exner"), ("pressure_p", "pressure_p"), ("pressure_base", "pressure_base"),
                      ("uReconstructZonal", "uzonal"), ("uReconstructMeridional", "umeridional")):
        dy.set_raw("diag", name, _img(f[fld]))
    dy.set_convective(_lib.CONV_ALL if flags is None else flags)
    if flags == 0:
        dy.set("diag", "cape", np.zeros(n))        # mask 0 allocates nothing: a first set_field does
    if mark:
        _mark(dy)
    return dy


def _mark(dy):
    from mpas_dycore import convcompute as cc
    for name in cc.OUTPUTS:
        dy.set_raw("diag", name, np.full(dy.field_bytes("diag", name) // 8, MARK))


def _outputs(dy, block=0):
    from mpas_dycore import convcompute as cc
    dy.synchronize()
    return {name: dy.get_raw("diag", name, block=block).copy() for name in cc.OUTPUTS}


def _compare(got, want, cells, stable, label):
    """got[cells] against want (which covers exactly them) in the two classes; the measured maxima."""
    from mpas_dycore import convcompute as cc
    worst = {}
    for name in cc.WRITTEN:
        g, w = got[name][cells], want[name]
        assert np.all(np.isfinite(g)), f"{label} {name}: not finite"
        if name not in cc.SOFT:
            assert np.array_equal(g, w), f"{label} {name}: not bit for bit on {np.count_nonzero(g != w)} of {w.size} cells"
            continue
        sel = np.ones(w.shape, dtype=bool) if name == "dewpoint_surface" else stable
        worst[name] = rel_linf(g[sel], w[sel]) if sel.any() else 0.0
    print(f"{label}: bounded class, rel Linf " + ", ".join(f"{n} {e:.2e}" for n, e in worst.items())
          + f"; {np.count_nonzero(~stable)} borderline of {stable.size}")
    for name, err in worst.items():
        assert err <= BOUND, f"{label} {name}: rel Linf {err:.3e} > {BOUND:g}"
    assert np.count_nonzero(~stable) <= 0.02 * stable.size
    assert np.all(got["cape"][cells] >= 0.0) and np.all(got["cin"][cells] >= 0.0)
    return worst


@pytest.mark.parametrize("K", KS)
def test_kernels_against_compiled_reference(golden, K):
    """One mpas_dyc_convective_diagnostics, all bits on: cells 0..39 against the compiled reference, cells
    40..129 against the host restatement.  K = 4: the column top below 6000 m and zp(1) above 1000 m (both
    clamps of column_height_value); 64: the levels fill a wavefront of the shear kernel exactly; 150: three
    chunks, and layers thinner than 100 Pa next to thick ones.
    Measured rel Linf on an MI355X (profiles/convcompute_new_tests.log), worst over the four K, bounded class
    (bound 1e-10): cape 7.3e-14, cin 1.1e-13, dewpoint_surface 1.9e-16; the other nine outputs bit for bit;
    no borderline column among the 4 x 130."""
    from mpas_dycore import convcompute as cc
    case = _case(K)
    f, ref, base, stable = _fields(K, golden)
    nc = ref["cape"].shape[0]
    dy = _standalone(case, f)
    before = _outputs(dy)
    dy.convective_diagnostics(1)
    after = _outputs(dy)
    dy.close()
    _compare(after, ref, slice(0, nc), stable[:nc], f"K={K} fixture")
    _compare(after, {n: base[n][nc:] for n in cc.WRITTEN}, slice(nc, NSOLVE), stable[nc:], f"K={K} rest")
    for name in cc.OUTPUTS:
        assert np.array_equal(after[name][NSOLVE:], before[name][NSOLVE:]) and np.all(after[name][NSOLVE:] == MARK), \
            f"{name}: a halo cell or the garbage slot was written"
        if name in ("lcl", "lfc"):
            assert np.all(after[name] == MARK), f"{name} was written"
        else:
            assert not np.any(after[name][:NSOLVE] == MARK), f"{name}: an owned cell was not written"


def test_bounded_work_column():
    """The K = 26 column whose pressure alternates between 1000 and 10 hPa ends by the sub-step cap, on the
    device as in the restatement: the same cape and cin within the bound.  It costs about fifteen ordinary
    columns with or without the guard."""
    from mpas_dycore import convcompute as cc
    case = _case(26)
    f = {name: a.copy() for name, a in _fields(26)[0].items()}
    alt = cc.alternating_column(26)
    for name in cc.INPUTS:
        f[name][1] = alt[name][0]
    want = cc.compute({name: f[name][:2] for name in cc.INPUTS})
    assert want["info"]["end"][1] == cc.END_CAP and want["info"]["end"][0] != cc.END_CAP
    dy = _standalone(case, f)
    dy.convective_diagnostics(1)
    got = _outputs(dy)
    dy.close()
    for name in ("cape", "cin"):
        assert np.isfinite(got[name][1])
        err = rel_linf(got[name][:2], want[name])
        print(f"alternating column: {name} {got[name][1]:.6g} (restatement {want[name][1]:.6g}), rel Linf {err:.2e}")
        assert err <= BOUND, (name, err)
    for name in cc.WRITTEN:
        if name not in cc.SOFT:
            assert np.array_equal(got[name][:2], want[name]), name


def _step_run(case, with_conv):
    from mpas_dycore import Dycore
    dy = Dycore(case, device=0, moist_end=NS)
    dy.init_diagnostics(STEP_DT)
    dy.use_graph(True)
    if with_conv:
        dy.set_convective()
    out = []
    for it in range(1, 4):
        dy.atm_timestep(STEP_DT, it)
        active, caps = dy.graph_active(), dy.graph_captures()
        dy.shift_time_levels()
        if with_conv:
            dy.convective_diagnostics(1)
        dy.synchronize()
        out.append(({m: dy.get("state", m, 1) for m in ("u", "w", "theta_m", "rho_zz", "scalars")}, active, caps))
    dy.close()
    return out


def test_structure():
    """Mask 0 writes nothing; each single bit writes exactly what the reference's quirks say; all bits at once
    equal the single bits; a context that never asked holds none of the fields; a run that calls the
    diagnostics between graph-replayed steps leaves the state's bits, the replay and the capture count alone."""
    from mpas_dycore import Dycore, _lib, convcompute as cc
    case = _case(26)
    n = case["nCells"]
    dy = Dycore(case, device=0, moist_end=NS)
    for name in cc.OUTPUTS:
        assert dy.field_bytes("diag", name) == 0, name
        assert not dy.lib.mpas_dyc_field_device_ptr(dy.h, b"diag", name.encode(), 1)
    dy.set_convective(0)
    dy.convective_diagnostics(1)                             # mask 0: nothing to do, nothing allocated
    assert dy.field_bytes("diag", "cape") == 0
    dy.set("diag", "srh_0_3km", np.full(n, 1.0))              # a first set_field allocates the group
    for name in cc.OUTPUTS:
        assert dy.field_bytes("diag", name) == 8 * (n + 1), name
    assert not dy.get("diag", "cape").any()
    dy.close()

    f = _fields(26)[0]
    dy = _standalone(case, f, flags=0)
    before = _outputs(dy)
    dy.convective_diagnostics(1)
    after = _outputs(dy)
    for name in before:
        assert np.array_equal(after[name], before[name]), f"mask 0 wrote {name}"
    single = {}
    for i in range(14):
        bit = 1 << i
        _mark(dy)
        dy.set_convective(bit)
        dy.convective_diagnostics(1)
        after = _outputs(dy)
        mine = cc.written_by(bit)
        for name in cc.OUTPUTS:
            if name in mine:
                assert not np.any(after[name][:NSOLVE] == MARK), f"bit {bit}: {name} not written"
                assert np.all(after[name][NSOLVE:] == MARK), f"bit {bit}: {name} halo written"
                if name in single:
                    assert np.array_equal(single[name], after[name]), f"bit {bit}: {name} differs from an earlier bit's"
                single[name] = after[name]
            else:
                assert np.all(after[name] == MARK), f"bit {bit} wrote {name}"
    assert set(single) == set(cc.WRITTEN)
    dy.set_convective(_lib.CONV_ALL)
    _mark(dy)
    dy.convective_diagnostics(1)
    together = _outputs(dy)
    dy.close()
    for name in cc.WRITTEN:
        assert np.array_equal(together[name], single[name]), f"{name}: single bit and all bits differ"

    plain, with_conv = _step_run(case, False), _step_run(case, True)
    for it, ((s0, a0, c0), (s1, a1, c1)) in enumerate(zip(plain, with_conv)):
        assert a0 == a1 and c0 == c1, (it, a0, a1, c0, c1)
        for m in s0:
            assert np.array_equal(s0[m], s1[m]), f"step {it + 1} {m}"
    assert plain[-1][1] and plain[-1][2] == 2


def test_four_blocks_equal_one_block():
    """Every written output on the owned cells, mapped to global numbering, bit for bit (each column is
    computed from its own data alone, so the device functions see the same arguments)."""
    from mpas_dycore import Dycore, decomp, convcompute as cc
    case = _case(26)
    n, K = case["nCells"], 26
    f = cc.synthetic_fields(case, K)

    def run(dy, blocks):
        dy.set_convective()
        for ib in range(dy.nblocks):
            rows = np.arange(n) if blocks is None else blocks[ib].glob["cell"]
            sc = np.zeros((rows.size, K, NS))
            sc[:, :, 0] = f["qv"][rows]
            dy.set_raw("state", "scalars", _img(sc), 1, block=ib)
            dy.set_raw("state", "theta_m", _img(f["theta_m"][rows]), 1, block=ib)
            dy.set("mesh", "zgrid", f["zgrid"][rows], block=ib)
            for name, fld in (("exner", "exner"), ("pressure_p", "pressure_p"), ("pressure_base", "pressure_base"),
                              ("uReconstructZonal", "uzonal"), ("uReconstructMeridional", "umeridional")):
                dy.set_raw("diag", name, _img(f[fld][rows]), block=ib)
        dy.convective_diagnostics(1)
        out = [_outputs(dy, ib) for ib in range(dy.nblocks)]
        dy.close()
        return out

    one = run(Dycore(case, device=0, moist_end=NS), None)[0]
    blocks = decomp.decompose(case, decomp.partition_sfc(n, 4))
    four = run(Dycore.from_blocks(blocks, device=0, moist_end=NS), blocks)
    assert one["cape"][:-1].max() > 100.0
    for name in cc.WRITTEN:
        got = decomp.gather_owned(blocks, [o[name][:-1] for o in four], "cell", n)
        assert np.array_equal(got, one[name][:-1]), name


def test_error_returns():
    import ctypes as C
    from mpas_dycore import Dycore, _lib
    from mpas_dycore.dycore import _make_dims
    case = _case(26)
    EINVAL, ESTATE = -1, -3
    dy = Dycore(case, device=0, moist_end=NS)
    lib, h = dy.lib, dy.h
    assert lib.mpas_dyc_set_convective(h, 16384) == EINVAL and lib.mpas_dyc_set_convective(h, -1) == EINVAL
    assert b"unknown flag bits" in lib.mpas_dyc_last_error(h)
    assert dy.field_bytes("diag", "cape") == 0                                # the failures allocated nothing
    assert lib.mpas_dyc_convective_diagnostics(h, 0) == EINVAL and lib.mpas_dyc_convective_diagnostics(h, 3) == EINVAL
    assert lib.mpas_dyc_set_convective(h, _lib.CONV_ALL) == 0
    assert dy.field_bytes("diag", "cape") == 8 * (case["nCells"] + 1)
    assert lib.mpas_dyc_convective_diagnostics(h, 1) == 0 and lib.mpas_dyc_convective_diagnostics(h, 2) == 0
    out = (C.c_double * 12)(*([-1.0] * 12))
    assert lib.mpas_dyc_get_profile(h, out, 11) == 0 and out[11] == -1.0      # out[11] only when n covers it
    assert dy.convective_diagnostics_ms(1) > 0.0
    assert lib.mpas_dyc_get_profile(h, out, 12) == 0 and out[11] > 0.0
    dy.close()
    # between the step and finish_step under the host's microphysics
    dy = Dycore(case, device=0, moist_end=NS)
    dy.init_diagnostics(STEP_DT)
    dy.set_physics(tendencies=True, microphysics=True)
    dy.set_convective(_lib.CONV_CAPE)
    dy.atm_timestep(STEP_DT, 1)
    assert dy.lib.mpas_dyc_convective_diagnostics(dy.h, 2) == ESTATE
    assert b"finish_step" in dy.lib.mpas_dyc_last_error(dy.h)
    dy.finish_step(STEP_DT)
    assert dy.lib.mpas_dyc_convective_diagnostics(dy.h, 2) == 0
    dy.close()
    # a host-only context keeps the mask, allocates nothing, and cannot run the diagnostics
    dims = _make_dims([case], [None], NS)
    cfg = _lib.make_config(case["config"])
    hh = C.c_void_p()
    assert lib.mpas_dyc_create_blocks(1, dims, C.byref(cfg), _lib.HOST_ONLY, C.byref(hh)) == 0
    try:
        assert lib.mpas_dyc_set_convective(hh, _lib.CONV_ALL) == 0
        assert lib.mpas_dyc_field_bytes(hh, b"diag", b"cape") == 0
        assert lib.mpas_dyc_convective_diagnostics(hh, 1) == ESTATE
        assert lib.mpas_dyc_set_convective(hh, 1 << 14) == EINVAL
    finally:
        lib.mpas_dyc_destroy(hh)
