"""GPU: the incremental analysis update (config_IAU_option = 'on') of the time step.

There is no compiled-reference parity for this branch: the oracle's harness driver pins
config_IAU_option to 'off'.  The check is structural instead.  By the reference's own construction
(mpas_atm_time_integration.F:459-469) an IAU step is a step whose physics tendencies are the
physics tendencies plus the IAU terms of atm_add_tend_anal_incr (mpas_atm_iau.F:168-211), and the
physics-tendency path is pinned to the compiled reference by test_gpu_physics.py.  So a context
with IAU on (A) must give, bit for bit, what a context with IAU off and physics coupling on (B)
gives when the host forms those sums itself: `iau_terms` below restates :168-211 in numpy, every
binary operation in the Fortran's order, from B's own rho_edge, rho_zz, theta_m and scalars of time
level 1 read before each step.

window = 2.5 dt: nint gives 3 forced steps, the fourth is free.
"""
import numpy as np
import pytest

from conftest import physics_forcing

pytestmark = pytest.mark.gpu

RVORD = 461.6 / 287.0   # mpas_constants.F: rv / rgas, as csrc/dycore.h
NS = 3                  # qv, qc, qr: all of them moist (moist_start..moist_end = 1..3)
STATE = [("u", "edge"), ("w", "cell"), ("theta_m", "cell"), ("rho_zz", "cell"), ("scalars", "cell")]
_CASES = {}


def _case(K, monotonic):
    from mpas_dycore.cases import jw_case
    if K not in _CASES:
        _CASES[K] = jw_case(642, K=K, ns=NS, moist=True, cache=False)
    c = dict(_CASES[K])
    c["config"] = dict(c["config"], config_monotonic=monotonic)
    return c


def increments(case):
    """The smooth analysis increments of mpas_dycore.cases.iau_increments (shared with the forecast case)."""
    from mpas_dycore.cases import iau_increments
    return iau_increments(case)


def iau_terms(wgt, inc, zz, rho_edge, rho_zz, theta_m, scalars, phys):
    """mpas_atm_iau.F:168-211 on top of the physics tendencies `phys` (tend_ru_physics,
    tend_rtheta_physics, tend_rho_physics, scalars_tend; element-major).  qv is scalar 0 and every
    scalar is moist.  Each line is one Fortran statement with its operations in its order."""
    if not wgt > 1.0e-12:                                                                  # :118
        return {n: a.copy() for n, a in phys.items()}
    u_amb, theta_amb, rho_amb, s_amb = inc["u_amb"], inc["theta_amb"], inc["rho_amb"], inc["scalars_amb"]
    qv = scalars[:, :, 0]
    ru = phys["tend_ru_physics"] + ((wgt * rho_edge) * u_amb)                              # :170
    rho_t = phys["tend_rho_physics"] + ((wgt * rho_amb) / zz)                              # :177
    theta = theta_m / (1.0 + (RVORD * qv))                                                 # :190
    tend_th = 0.0 + (wgt * ((theta_amb * rho_zz) + ((theta * rho_amb) / zz)))              # :163, :197
    st = phys["scalars_tend"] + (wgt * ((s_amb * rho_zz[:, :, None])                       # :198-199
                                        + ((scalars * rho_amb[:, :, None]) / zz[:, :, None])))
    tend_th = ((1.0 + (RVORD * qv)) * tend_th) + ((RVORD * theta) * st[:, :, 0])           # :207-208
    rtheta = phys["tend_rtheta_physics"] + tend_th                                         # :209
    return dict(tend_ru_physics=ru, tend_rtheta_physics=rtheta, tend_rho_physics=rho_t, scalars_tend=st)


def _img(a):
    out = np.zeros((a.shape[0] + 1,) + a.shape[1:])
    out[:-1] = a
    return out


def _zero_phys(case):
    K = case["nVertLevels"]
    return dict(tend_ru_physics=np.zeros((case["nEdges"], K)), tend_rtheta_physics=np.zeros((case["nCells"], K)),
                tend_rho_physics=np.zeros((case["nCells"], K)), scalars_tend=np.zeros((case["nCells"], K, NS)))


def _set_phys(dy, t):
    for n in ("tend_ru_physics", "tend_rtheta_physics", "tend_rho_physics"):
        dy.set_raw("tend_physics", n, _img(t[n]))
    dy.set_raw("tend", "scalars_tend", _img(t["scalars_tend"]))


def _state(dy):
    dy.synchronize()
    return {n: dy.get("state", n, 1) for n, _ in STATE}


def _same(a, b, what):
    for n, _ in STATE:
        assert np.all(np.isfinite(b[n])), f"{what}: {n} is not finite"
        assert np.array_equal(a[n], b[n]), f"{what}: {n} differs, max |diff| {np.nanmax(np.abs(a[n] - b[n])):.3e}"


def _same_bits(a, b, what):
    """Bit for bit in the strict sense, on the 64-bit patterns: also where a run has left the
    model's range and holds NaNs, which np.array_equal on the values never calls equal."""
    for n, _ in STATE:
        assert np.array_equal(a[n].view(np.uint64), b[n].view(np.uint64)), f"{what}: the bits of {n} differ"


def _window(case):
    dt = float(case["dt"])
    return dt, 2.5 * dt


def run_iau(case, nsteps, phys=None, graph=None):
    """Context A: IAU on, increments uploaded with the case.  phys: the host's physics tendencies."""
    from mpas_dycore import Dycore
    dt, window = _window(case)
    dy = Dycore(dict(case, **increments(case)), device=0, moist_end=NS)
    dy.init_diagnostics(dt)
    if graph is not None:
        dy.use_graph(graph)
    if phys is not None:
        dy.set_physics(tendencies=True)
        _set_phys(dy, phys)
    dy.set_iau(True, window)
    out, extra = [], {}
    for it in range(1, nsteps + 1):
        if phys is not None:
            dy.set_raw("tend", "scalars_tend", _img(phys["scalars_tend"]))
        dy.atm_timestep(dt, it)
        extra.setdefault("graph", []).append(dy.graph_active())
        dy.shift_time_levels()
        out.append(_state(dy))
        if it == 2 and phys is not None:
            extra["tend_physics"] = {n: dy.get("tend_physics", n) for n in
                                     ("tend_ru_physics", "tend_rtheta_physics", "tend_rho_physics")}
    extra["captures"] = dy.graph_captures()
    extra["dy"] = dy
    return out, extra


def run_host_sums(case, nsteps, phys=None):
    """Context B: IAU off, physics coupling on; before every step the host sets the tendencies to
    the physics tendencies + the IAU terms, formed from B's own fields."""
    from mpas_dycore import Dycore
    dt, window = _window(case)
    inc = increments(case)
    dy = Dycore(case, device=0, moist_end=NS)
    dy.init_diagnostics(dt)
    dy.set_physics(tendencies=True)
    base = phys if phys is not None else _zero_phys(case)
    out = []
    for it in range(1, nsteps + 1):
        dy.synchronize()
        wgt = dy.iau_weight(dt, it)
        assert wgt == 0.0  # IAU is off in B: the weight is the test's own
        wgt = 1.0 / window if it <= 3 else 0.0
        t = iau_terms(wgt, inc, case["zz"], dy.get("diag", "rho_edge"), dy.get("state", "rho_zz", 1),
                      dy.get("state", "theta_m", 1), dy.get("state", "scalars", 1), base)
        _set_phys(dy, t)
        dy.atm_timestep(dt, it)
        dy.shift_time_levels()
        out.append(_state(dy))
    dy.close()
    return out


def _equivalence(K, monotonic, nsteps):
    case = _case(K, monotonic)
    a, ex = run_iau(case, nsteps)
    ex["dy"].close()
    b = run_host_sums(case, nsteps)
    for it in range(nsteps):
        _same(a[it], b[it], f"K={K} step {it + 1}")
    return a


@pytest.mark.parametrize("monotonic", [True, False])
def test_iau_equals_host_formed_tendencies(monotonic):
    """IAU on, no physics flag from the host == physics coupling with 0 + the IAU terms, over the
    three forced steps and the free fourth."""
    a = _equivalence(26, monotonic, 4)
    for n, _ in STATE:
        assert np.all(np.isfinite(a[-1][n])), n


@pytest.mark.parametrize("scale", [1.0, 0.1])
def test_iau_with_host_physics_and_the_hosts_arrays_untouched(scale):
    """Host physics (conftest.physics_forcing) + IAU == the host's sums of both, and the host's
    tend_physics arrays still hold what the host set after a forced step.

    scale = 1.0 is the forcing of the physics tests as it stands.  Its coupled qv tendency is
    -5e-7 aloft, where rho_zz is 5e-3; mpas_atm_iau.F:207-208 multiplies scalars_tend(qv) -- the physics'
    part included -- by Rv/Rd theta, about 2400 K at the top, and adds it to the theta_m tendency: with
    this mesh's dt of 5760 s that is theta_m < 0 after step 1 and NaNs from step 2 on, with IAU on the
    device and with the host's sums alike (measured: min theta_m -150 K after step 1 whichever
    increment is non-zero).  So at scale 1.0 the values are compared while they are finite (step 1) and
    the bit patterns at every step; scale = 0.1 stays finite over the four steps (theta_m 1369, 1222,
    1125, 1126 K at most) and is compared by value at every step."""
    case = _case(26, True)
    phys = physics_forcing(case, scale)
    a, ex = run_iau(case, 4, phys=phys)
    ex["dy"].close()
    b = run_host_sums(case, 4, phys=phys)
    for it in range(4):
        _same_bits(a[it], b[it], f"with physics x {scale}, step {it + 1}")
        if scale < 1.0 or it == 0:
            _same(a[it], b[it], f"with physics x {scale}, step {it + 1}")
    for n, got in ex["tend_physics"].items():  # after a forced step: still what the host set
        assert np.array_equal(got, phys[n]), n


def test_iau_forcing_acts_and_switches_off():
    from mpas_dycore import Dycore
    case = _case(26, True)
    dt, _ = _window(case)
    zero = _zero_phys(case)
    # a free run on the physics-on / zero-tendency path
    dy = Dycore(case, device=0, moist_end=NS)
    dy.init_diagnostics(dt)
    dy.set_physics(tendencies=True)
    _set_phys(dy, zero)
    dy.atm_timestep(dt, 1)
    dy.shift_time_levels()
    free = _state(dy)
    dy.close()
    a, ex = run_iau(case, 1, phys=zero)
    dy = ex["dy"]
    for n in ("u", "theta_m", "rho_zz"):
        assert not np.array_equal(a[0][n], free[n]), n
    assert not np.array_equal(a[0]["scalars"][:, :, 0], free["scalars"][:, :, 0]), "qv"
    # IAU off again: the next step is the physics-on / zero-tendency step from A's state
    dy.set_iau(False)
    dy.set_raw("tend", "scalars_tend", _img(zero["scalars_tend"]))
    dy.atm_timestep(dt, 2)
    dy.shift_time_levels()
    got = _state(dy)
    dy.close()
    b = Dycore(case, device=0, moist_end=NS)
    b.init_diagnostics(dt)
    b.set_physics(tendencies=True)
    inc = increments(case)
    _, window = _window(case)
    t = iau_terms(1.0 / window, inc, case["zz"], b.get("diag", "rho_edge"), b.get("state", "rho_zz", 1),
                  b.get("state", "theta_m", 1), b.get("state", "scalars", 1), zero)
    _set_phys(b, t)
    b.atm_timestep(dt, 1)
    b.shift_time_levels()
    _same(a[0], _state(b), "step 1")
    _set_phys(b, zero)
    b.atm_timestep(dt, 2)
    b.shift_time_levels()
    _same(got, _state(b), "the step after set_iau(False)")
    b.close()


@pytest.mark.parametrize("K", [27, 4, 80, 150])
def test_iau_shapes(K):
    """K = 27: (nCells + 1) K is odd, so the cell kernel takes one value per lane, and the edge
    kernel's last value is a single one; K = 4: the smallest column; K = 80 and 150: the 128-lane
    and 192-lane builds, which share the kernels' one source."""
    _equivalence(K, False, 2)


def _blocks_equal_one_block(case, part, nsteps):
    from mpas_dycore import Dycore, decomp
    dt, window = _window(case)
    one, ex = run_iau(case, nsteps)
    ex["dy"].close()
    full = dict(case, **increments(case))
    blocks = decomp.decompose(full, part)
    assert all("scalars_amb" in b.case and b.case["u_amb"].shape[0] == b.case["nEdges"] for b in blocks)
    dy = Dycore.from_blocks(blocks, device=0, moist_end=NS)
    dy.init_diagnostics(dt)
    dy.set_iau(True, window)
    n_glob = {"cell": case["nCells"], "edge": case["nEdges"]}
    for it in range(1, nsteps + 1):
        dy.atm_timestep(dt, it)
        dy.shift_time_levels()
        dy.synchronize()
        got = {n: decomp.gather_owned(blocks, [dy.get("state", n, 1, block=i) for i in range(len(blocks))], loc,
                                      n_glob[loc]) for n, loc in STATE}
        _same(got, one[it - 1], f"{len(blocks)} blocks, step {it}")
    dy.close()
    return blocks


def test_iau_four_blocks_equal_one_block():
    """Owned against halo ranges: the IAU terms on the owned elements only, the physics value (0)
    on the halo elements of the new arrays, no new exchange."""
    from mpas_dycore import decomp
    case = _case(26, True)
    _blocks_equal_one_block(case, decomp.partition_sfc(case["nCells"], 4), 4)


def test_iau_blocks_pair_across_the_owned_end():
    """K = 27 in blocks: where the owned range ends on an odd value, one 16-byte pair of the
    two-values-per-lane kernels holds an owned and a halo value.  The partition (contiguous ranges of
    the cell order, as partition_sfc makes them) is chosen so that a block has an odd nEdgesSolve (the
    edge kernel) and a block an even nCells + 1 with an odd nCellsSolve (the cell kernel's two-value
    form at an odd K); the blocks with an odd nCells + 1 take its one-value form."""
    case = _case(27, False)
    part = np.zeros(case["nCells"], dtype=np.int64)
    for i, c in enumerate((161, 322, 483)):
        part[c:] = i + 1
    blocks = _blocks_equal_one_block(case, part, 2)
    K = case["nVertLevels"]
    assert any((b.solve[1] * K) % 2 for b in blocks)
    assert any(((b.case["nCells"] + 1) * K) % 2 == 0 and (b.solve[0] * K) % 2 for b in blocks)
    assert any(((b.case["nCells"] + 1) * K) % 2 for b in blocks)


def test_iau_graph_branches():
    """Captured steps: every step replays a graph, and the states are the eager run's across the
    window's end.  The count of captures comes from the measurement hook mpas_dyc_get_profile
    (out[5], Dycore.graph_captures).  A step is captured once per buffer layout it starts from (two:
    the time-level parity) and IAU branch (two), never because itimestep changed: steps 1 and 2 capture
    the forced branch on either parity, step 3 replays, steps 4 and 5 capture the free branch on
    either parity -- the fifth step captures nothing again, it is the first free step of its parity --
    and from step 6 on nothing is captured."""
    case = _case(26, True)
    eager, ex = run_iau(case, 5, graph=False)
    ex["dy"].close()
    assert ex["graph"] == [False] * 5 and ex["captures"] == 0
    from mpas_dycore import Dycore
    dt, window = _window(case)
    dy = Dycore(dict(case, **increments(case)), device=0, moist_end=NS)
    dy.init_diagnostics(dt)
    dy.use_graph(True)
    dy.set_iau(True, window)
    caps = []
    for it in range(1, 7):
        dy.atm_timestep(dt, it)
        assert dy.graph_active(), f"step {it} ran eagerly"
        caps.append(dy.graph_captures())
        dy.shift_time_levels()
        if it <= 5:
            _same(_state(dy), eager[it - 1], f"graph, step {it}")
    dy.close()
    assert caps == [1, 2, 2, 3, 4, 4], caps


def test_first_set_field_completes_the_pool_of_its_block_only():
    """The tend_iau pool is allocated on demand, block by block: a first set of one of its fields
    makes the other increments of that block readable, as zeros; the other block's pool stays
    unallocated (MPAS_DYC_ESTATE on get) until set_iau(on), which completes every block's."""
    import ctypes as C
    from mpas_dycore import Dycore, decomp
    case = _case(27, False)
    blocks = decomp.decompose(case, decomp.partition_sfc(case["nCells"], 2))
    assert not any(n in b.case for b in blocks for n in ("u_amb", "theta_amb", "rho_amb", "scalars_amb"))
    dy = Dycore.from_blocks(blocks, device=0, moist_end=NS)
    names = ("u", "theta", "rho", "scalars")

    def rc_get(ib, n):
        buf = np.empty(dy.field_bytes("tend_iau", n, block=ib) // 8)
        assert buf.size > 0
        return dy.lib.mpas_dyc_get_block_field(dy.h, ib, b"tend_iau", n.encode(), 1, buf.ctypes.data_as(C.c_void_p),
                                               buf.nbytes)

    assert all(rc_get(ib, n) == -3 for ib in (0, 1) for n in names)   # MPAS_DYC_ESTATE: nothing set yet
    K = case["nVertLevels"]
    u1 = np.random.default_rng(11).standard_normal((blocks[1].case["nEdges"] + 1) * K)
    dy.set_raw("tend_iau", "u", u1, block=1)
    assert np.array_equal(dy.get_raw("tend_iau", "u", block=1), u1)
    for n, size in (("theta", K), ("rho", K), ("scalars", K * NS)):
        a = dy.get_raw("tend_iau", n, block=1)
        assert a.shape == ((blocks[1].case["nCells"] + 1) * size,) and not a.any(), n
    assert all(rc_get(0, n) == -3 for n in names)                     # block 0 is as it was
    dy.set_iau(True, _window(case)[1])
    for ib in (0, 1):
        for n in names:
            a = dy.get_raw("tend_iau", n, block=ib)
            if (ib, n) == (1, "u"):
                assert np.array_equal(a, u1)
            else:
                assert a.size and not a.any(), (ib, n)
    dy.close()
