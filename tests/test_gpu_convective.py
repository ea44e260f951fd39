"""GPU: the convective running maxima on the device (mpas_dyc_set_diag_update / diag_update /
diag_reset; csrc/convdiag.hip) against mpas_dycore.convective.update, the numpy restatement of
convective_diagnostics_update (convective_diagnostics.F:99-198), bit for bit.

There is no compiled-reference parity for this routine: the oracle's harness driver does not call
mpas_atm_diag_update.  tests/test_convective_host.py pins the restatement to a loop transcription.

Measured on an MI355X (printed by the tests): 4 blocks against one block, updraft_helicity_max
relative Linf 1.5e-16 .. 1.8e-16 on the synthetic fields (K = 26, 27) and 1.3e-16 after 3 steps of the
moist JW run (where it is non-zero on 45 % of the cells); w_velocity_max and wind_speed_level1_max
identical.
"""
import numpy as np
import pytest

from conftest import rel_linf
# the synthetic fields are shared with the CPU file, which lies next to this one: pytest puts this
# directory on sys.path for both (as for conftest), so keep the two files together
from test_convective_host import synthetic

pytestmark = pytest.mark.gpu

FIELDS = ("w_velocity_max", "wind_speed_level1_max", "updraft_helicity_max")
INPUTS = (("state", "w"), ("diag", "vorticity"), ("diag", "uReconstructZonal"), ("diag", "uReconstructMeridional"))
STATE = ("u", "w", "theta_m", "rho_zz", "scalars")
PARITY = 1e-10   # the project's parity bound (README, conftest.rel_linf)
_CASES = {}


def _case(K, moist=False):
    from mpas_dycore.cases import jw_case
    key = (K, moist)
    if key not in _CASES:
        _CASES[key] = jw_case(642, K=K, ns=3 if moist else 1, moist=moist, cache=False)
    return _CASES[key]


def _upload(dy, fields, block=0):
    """Element-major arrays into the device fields (the image has the garbage slot appended)."""
    for (pool, name), a in zip(INPUTS, fields):
        img = np.zeros((a.shape[0] + 1,) + a.shape[1:])
        img[:-1] = a
        dy.set_raw(pool, name, img, 1, block)


def _maxima(dy, block=0, raw=False):
    """The three fields of a block: (nCells,), or with raw the whole image with the garbage slot."""
    dy.synchronize()
    out = {n: dy.get_raw("diag", n, block=block) for n in FIELDS}
    return out if raw else {n: a[:-1] for n, a in out.items()}


def _same(got, want, what):
    for n in FIELDS:
        assert np.all(np.isfinite(got[n])), f"{what}: {n} is not finite"
        assert np.array_equal(got[n], want[n]), \
            f"{what}: {n} differs on {np.count_nonzero(got[n] != want[n])} cells, max |diff| {np.max(np.abs(got[n] - want[n])):.3e}"


def _synthetic_run(case, what, phases=(0.0, 1.3)):
    """Two uploads of the synthetic fields (phase 0.0, then 1.3) with diag_update after each, against
    the restatement; returns the restatement's fields after each call."""
    from mpas_dycore import Dycore, convective
    dy = Dycore(case, device=0, moist_end=case["num_scalars"])
    dy.set_diag_update()
    want, steps = convective.zeros(case), []
    for ph in phases:
        f = synthetic(case, ph)
        _upload(dy, f)
        dy.diag_update()
        want = convective.update(case, *f, want, convective.ALL)
        got = _maxima(dy, raw=True)
        _same({n: a[:-1] for n, a in got.items()}, want, f"{what}, phase {ph}")
        assert all(got[n][-1] == 0.0 for n in FIELDS), "the garbage slot was written"
        steps.append(want)
    dy.close()
    # what keeps the comparison from passing on trivia
    a, b = steps[0]["updraft_helicity_max"], steps[1]["updraft_helicity_max"]
    frac = (np.mean(a > 0), np.mean(b > a), np.mean((b == a) & (a != 0)))
    print(f"{what}: uph > 0 on {frac[0]:.1%}, raised by the second call {frac[1]:.1%}, first value kept {frac[2]:.1%}")
    assert min(frac) >= 0.15, frac
    return steps


@pytest.mark.parametrize("K", [4, 26, 27, 63, 64, 150])
def test_synthetic_fields_one_block(K):
    """K = 4: the 2-5 km band lies inside level 1; 150: it covers 17 levels; 63 / 64: the lane
    stride's boundary for the K and K + 1 arrays (and the 64-lane / 128-lane builds)."""
    case = _case(K)
    _synthetic_run(case, f"K={K}")
    z = case["zgrid"] - case["zgrid"][:, :1]
    nband = np.sum((np.minimum(z[:, 1:], 5000.0) - np.maximum(z[:, :-1], 2000.0)) > 0, axis=1)
    if K == 4:
        assert nband.max() == 1 and np.all(z[:, 1] > 5000.0)
    if K == 150:
        assert nband.max() >= 17
    assert case["zgrid"][:, 0].min() < -100.0 and case["zgrid"][:, 0].max() > 100.0  # AGL is not MSL here


def test_synthetic_fields_varres_mesh(varres_case_small):
    """Heptagons, a declared stride of 7.  Most of this mesh's cells lie in its refined region, where
    a second phase of 1.3 raises only 11.8 % of them (the restatement alone, on the CPU); 2.6 raises
    24.4 %, so the conditions against trivia hold here as on the uniform mesh."""
    case = varres_case_small
    assert case["maxEdges"] == 7 and case["nEdgesOnCell"].max() == 7
    _synthetic_run(case, "varres", phases=(0.0, 2.6))


def _assemble(blocks, per_block, n_cells):
    from mpas_dycore import decomp
    return {n: decomp.gather_owned(blocks, [m[n] for m in per_block], "cell", n_cells) for n in FIELDS}


def _check_assembled(got, one, what):
    for n in FIELDS[:2]:
        assert np.array_equal(got[n], one[n]), f"{what}: {n} of the blocks differs from one block"
    err = rel_linf(got[FIELDS[2]], one[FIELDS[2]])
    print(f"{what}: updraft_helicity_max, blocks against one block, rel Linf {err:.3e}")
    assert err <= PARITY, err
    return err


@pytest.mark.parametrize("K", [26, 27])
def test_synthetic_fields_four_blocks(K):
    """Each block equals the restatement on its own numbering bit for bit; assembled over the owned
    cells, w and wind-speed maxima equal the one-block result bit for bit, the updraft helicity
    within the parity bound (its vertex sums run in each block's own vertex order)."""
    from mpas_dycore import Dycore, convective, decomp
    case = _case(K)
    blocks = decomp.decompose(case, decomp.partition_sfc(case["nCells"], 4))
    dy = Dycore.from_blocks(blocks, device=0)
    dy.set_diag_update()
    want = [convective.zeros(b.case) for b in blocks]
    one = convective.zeros(case)
    for ph in (0.0, 1.3):
        full = synthetic(case, ph)
        one = convective.update(case, *full, one, convective.ALL)
        for ib, b in enumerate(blocks):
            f = tuple(a[b.glob[loc]] for a, loc in zip(full, ("cell", "vertex", "cell", "cell")))
            _upload(dy, f, ib)
            want[ib] = convective.update(b.case, *f, want[ib], convective.ALL, n_solve=b.solve[0])
        dy.diag_update()
        got = [_maxima(dy, ib) for ib in range(len(blocks))]
        for ib, b in enumerate(blocks):
            _same(got[ib], want[ib], f"K={K} block {ib}, phase {ph}")
            assert not any(got[ib][n][b.solve[0]:].any() for n in FIELDS), "a halo cell was written"
        _check_assembled(_assemble(blocks, got, case["nCells"]), one, f"K={K}, phase {ph}")
    dy.close()
    assert np.mean(one["updraft_helicity_max"] > 0) >= 0.15


def _run(case, nsteps, diag, blocks=None):
    """nsteps of the moist run with a captured step; diag: diag_update after every shift, checked
    against the restatement advanced from the downloaded fields.  Returns the final state (one
    block), the maxima per block and the graph counters."""
    from mpas_dycore import Dycore, convective
    dt = float(case["dt"])
    ns = case["num_scalars"]
    dy = Dycore(case, device=0, moist_end=ns) if blocks is None else Dycore.from_blocks(blocks, device=0, moist_end=ns)
    cases = [case] if blocks is None else [b.case for b in blocks]
    solves = [None] if blocks is None else [b.solve[0] for b in blocks]
    dy.init_diagnostics(dt)
    dy.use_graph(True)
    if diag:
        dy.set_diag_update()
    want = [convective.zeros(c) for c in cases]
    active = []
    for it in range(1, nsteps + 1):
        dy.atm_timestep(dt, it)
        active.append(dy.graph_active())
        dy.shift_time_levels()
        if not diag:
            continue
        dy.diag_update()
        dy.synchronize()
        for ib, c in enumerate(cases):
            f = [dy.get(pool, name, 1, ib) for pool, name in INPUTS]
            want[ib] = convective.update(c, *f, want[ib], convective.ALL, n_solve=solves[ib])
            _same(_maxima(dy, ib), want[ib], f"step {it} block {ib}")
    dy.synchronize()
    state = {n: dy.get("state", n, 1) for n in STATE} if blocks is None else None
    return dy, state, want, (active, dy.graph_captures())


def test_real_run_with_a_captured_step():
    from mpas_dycore import convective, decomp
    case = _case(26, moist=True)
    dy0, plain, _, graph0 = _run(case, 3, diag=False)
    dy0.close()
    dy, state, one, graph = _run(case, 3, diag=True)
    # the step, its graph and its results are what they are without the diag calls
    for n in STATE:
        assert np.array_equal(state[n], plain[n]), f"{n} changed by the diag calls"
    assert graph[0] == [True] * 3 and graph == graph0, (graph, graph0)
    one = one[0]
    assert np.mean(one["w_velocity_max"] != 0) > 0.9 and np.mean(one["wind_speed_level1_max"] > 0) > 0.9
    print(f"moist JW, 3 steps: updraft_helicity_max > 0 on {np.mean(one['updraft_helicity_max'] > 0):.1%} of the cells, "
          f"max {one['updraft_helicity_max'].max():.3e}")
    # reset of one field: the whole array, the other two untouched
    dy.diag_reset(w_max=False, wsp_max=False, uh_max=True)
    got = _maxima(dy, raw=True)
    assert not got["updraft_helicity_max"].any()
    for n in FIELDS[:2]:
        assert np.array_equal(got[n][:-1], one[n]), n
    dy.close()
    # 4 blocks: each against the restatement on its numbering (inside _run), assembled against one
    # block -- the step leaves valid vorticity on the halo vertices of owned cells
    blocks = decomp.decompose(case, decomp.partition_sfc(case["nCells"], 4))
    dyb, _, per_block, graphb = _run(case, 3, diag=True, blocks=blocks)
    dyb.close()
    assert graphb[0] == [True] * 3
    _check_assembled(_assemble(blocks, per_block, case["nCells"]), one, "moist JW, 3 steps, 4 blocks")


def test_api():
    import ctypes as C
    from mpas_dycore import Dycore, _lib, convective, decomp
    from mpas_dycore.dycore import DycoreError, _make_dims
    case = _case(26)
    dy = Dycore(case, device=0)
    with pytest.raises(DycoreError):       # a context that never asked holds none of the fields
        dy.get_raw("diag", "w_velocity_max")
    dy.diag_update()                       # mask 0: nothing to do, nothing allocated
    with pytest.raises(DycoreError):
        dy.get_raw("diag", "w_velocity_max")
    dy.set_diag_update()
    for n, a in _maxima(dy, raw=True).items():
        assert a.shape == (case["nCells"] + 1,) and not a.any(), n
    # unknown bits
    for call in (dy.lib.mpas_dyc_set_diag_update, dy.lib.mpas_dyc_diag_reset):
        assert call(dy.h, 8) == -1 and call(dy.h, -1) == -1   # MPAS_DYC_EINVAL
    # mask 0 is a no-op
    f = synthetic(case, 0.0)
    _upload(dy, f)
    dy.set_diag_update(flags=0)
    dy.diag_update()
    assert not any(a.any() for a in _maxima(dy).values())
    # a mask updates only the named field
    dy.set_diag_update(w_max=False, wsp_max=True, uh_max=False)
    dy.diag_update()
    want = convective.update(case, *f, convective.zeros(case), convective.WIND_SPEED_LEVEL1_MAX)
    _same(_maxima(dy), want, "wind speed only")
    assert want["wind_speed_level1_max"].all()
    # set / get round trip (a restart puts the fields back), the update goes on from there
    rng = np.random.default_rng(5)
    back = {n: rng.uniform(0.0, 30.0, case["nCells"]) for n in FIELDS}
    for n, a in back.items():
        dy.set("diag", n, a)
    got = _maxima(dy)
    assert all(np.array_equal(got[n], back[n]) for n in FIELDS)
    assert dy.lib.mpas_dyc_field_device_ptr(dy.h, b"diag", b"updraft_helicity_max", 1)
    dy.set_diag_update()
    dy.diag_update()
    _same(_maxima(dy), convective.update(case, *f, back, convective.ALL), "after set")
    # ESTATE between the step and finish_step of a microphysics host
    dt = float(case["dt"])
    dy.init_diagnostics(dt)
    dy.set_physics(tendencies=True, microphysics=True)
    dy.atm_timestep(dt, 1)
    assert dy.lib.mpas_dyc_diag_update(dy.h) == -3     # MPAS_DYC_ESTATE
    dy.finish_step(dt)
    dy.shift_time_levels()
    dy.diag_update()
    dy.synchronize()
    dy.close()
    # a first set_field allocates all three, zeroed, without set_diag_update
    dy = Dycore(case, device=0)
    dy.set("diag", "w_velocity_max", back["w_velocity_max"])
    got = _maxima(dy)
    assert np.array_equal(got["w_velocity_max"], back["w_velocity_max"])
    assert not got["wind_speed_level1_max"].any() and not got["updraft_helicity_max"].any()
    dy.close()
    # a host-only context: ESTATE
    lib = _lib.load()
    blocks = decomp.decompose(case, decomp.partition_sfc(case["nCells"], 2))
    h = C.c_void_p()
    dims = _make_dims([b.case for b in blocks], [b.solve for b in blocks], 1)
    cfg = _lib.make_config(case["config"])
    assert lib.mpas_dyc_create_blocks(len(blocks), dims, C.byref(cfg), _lib.HOST_ONLY, C.byref(h)) == 0
    try:
        assert lib.mpas_dyc_set_diag_update(h, 7) == 0
        assert lib.mpas_dyc_diag_update(h) == -3
        assert lib.mpas_dyc_diag_reset(h, 7) == -3
    finally:
        lib.mpas_dyc_destroy(h)


def test_table_follows_a_new_cells_on_vertex():
    """The (vertex, j) table is a derived table: setting cellsOnVertex again rebuilds it.  The same
    mesh with its vertices' three cells rotated (j -> j + 1, kite areas moved along) has the same
    sums in the same vertex order, so the result must not change; with the kite areas left in place
    it must."""
    from mpas_dycore import Dycore, convective
    case = _case(26)
    f = synthetic(case, 0.0)
    want = convective.update(case, *f, convective.zeros(case), convective.UPDRAFT_HELICITY_MAX)
    dy = Dycore(case, device=0)
    dy.set_diag_update(w_max=False, wsp_max=False, uh_max=True)
    _upload(dy, f)
    dy.diag_update()
    _same(_maxima(dy), want, "as uploaded")
    rolled = dict(case, cellsOnVertex=np.roll(case["cellsOnVertex"], 1, axis=1))
    dy.set("mesh", "cellsOnVertex", rolled["cellsOnVertex"])
    dy.diag_reset()
    dy.diag_update()
    moved = convective.update(rolled, *f, convective.zeros(case), convective.UPDRAFT_HELICITY_MAX)
    _same(_maxima(dy), moved, "cellsOnVertex rolled, kite areas in place")
    assert not np.array_equal(moved["updraft_helicity_max"], want["updraft_helicity_max"])
    dy.set("mesh", "kiteAreasOnVertex", np.roll(case["kiteAreasOnVertex"], 1, axis=1))
    dy.diag_reset()
    dy.diag_update()
    _same(_maxima(dy), want, "both rolled")
    dy.close()
