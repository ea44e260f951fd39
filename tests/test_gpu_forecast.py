"""GPU: the step's optional parts together -- host physics tendencies, the incremental analysis update,
regional lateral boundary conditions, Kessler microphysics inside the step and the convective running
maxima after it -- on several blocks and with graph replay, as a regional forecast runs them.

Each part has its own file (test_gpu_physics.py, test_gpu_iau.py, test_gpu_lbc.py, test_gpu_lbc_decomp.py,
test_gpu_kessler.py, test_gpu_convective.py); none of those turns two device-side parts on at once.  The
case is mpas_dycore.cases.forecast_case (x1.642, qv / qc / qr, dt = 600 s; tests/test_forecast_case.py
asserts what it has to cover).  Two runners:

A (`run_a`) -- everything on the device: set_physics(tendencies), set_iau, set_microphysics("kessler"),
  set_diag_update, set_summary, and per step set_lbc, atm_timestep, shift_time_levels, diag_update.
B (`run_b`) -- the same forecast with every hook the host can own done by the host: one block, eager,
  IAU off, set_physics(tendencies, microphysics), LBCs on; before each step the physics + IAU sums by
  test_gpu_iau.iau_terms from B's own fields, after it mpas_dycore.kessler.driver on time level 2,
  finish_step, and mpas_dycore.convective.update for the running maxima.  Each of B's parts is pinned on
  its own: the physics path, the LBCs and a host microphysics ahead of the regional tail to the compiled
  reference (test_gpu_physics.py, test_gpu_lbc.py, test_gpu_dropin.py), iau_terms, kessler.driver and
  convective.update to the reference's sources or fixtures by their host tests.

The device's pow / exp are not the C library's, so A against B holds to the project's bounds (rel Linf
1e-10; 1e-9 on w and the mixing ratios, per species), not bit for bit; everything structural -- the
specified zone against the driving data, blocks against one block, graph against eager, a restart -- is
bit for bit, except updraft_helicity_max across blocks (its vertex sums run in each block's own order).
"""
import numpy as np
import pytest

from conftest import progress, rel_linf
# helpers of the sibling test files: pytest puts this directory on sys.path (as for conftest)
from test_forecast_case import partition
from test_gpu_iau import iau_terms
from test_gpu_restart import DIAG as RESTART_DIAG
from test_gpu_stress import rel_linf_species

pytestmark = pytest.mark.gpu

NS = 3
STATE = [("u", "edge"), ("w", "cell"), ("theta_m", "cell"), ("rho_zz", "cell"), ("scalars", "cell")]
ACC = [("diag_physics", "rainnc"), ("diag_physics", "rainncv"), ("diag_physics", "precipw"),
       ("diag_physics", "i_rainnc"), ("diag", "surface_pressure"), ("tend", "tend_sfc_pressure")]
MAXIMA = ("w_velocity_max", "wind_speed_level1_max", "updraft_helicity_max")
PHYS = ("tend_ru_physics", "tend_rtheta_physics", "tend_rho_physics")
REGIONAL = ("bdyMaskCell", "bdyMaskEdge", "specZoneMaskCell", "specZoneMaskEdge", "nearestRelaxationCell",
            "meshScalingRegionalCell", "meshScalingRegionalEdge")   # what cases.regional_lbc adds to a case
SUMMARY_KEYS = ("flags", "w_min", "w_max", "u_min", "u_max", "nan_w", "nan_u", "scalars")
TIGHT, LOOSE = 1e-10, 1e-9      # test_gpu_kessler.py / test_gpu_convective.py: u, theta_m, rho_zz, 2-D fields; w, scalars
ACTS = 1e-8                     # test_gpu_kessler.py: "the run with the scheme off differs by more than"
_CASES, _RUNS = {}, {}


def _forecast(K):
    from mpas_dycore.cases import forecast_case
    if K not in _CASES:
        _CASES[K] = forecast_case(K)
    return _CASES[K]


def _img(a):
    out = np.zeros((a.shape[0] + 1,) + a.shape[1:], dtype=a.dtype)
    out[:-1] = a
    return out


def _dtr(lbc, dt, it):
    """Seconds from the start of step ``it`` to the end of the LBC interval: set_lbc's argument."""
    return lbc["interval_end"] - (it - 1) * dt


def _set_lbc_pool(dy, case, lbc, blocks):
    from oracle import ref_runner
    for (name, tl), img in ref_runner.lbc_images(case, lbc).items():
        loc = "edge" if name in ("lbc_u", "lbc_ru") else "cell"
        for ib in range(dy.nblocks):
            dy.set_raw("lbc", name, img if blocks is None else _img(img[:-1][blocks[ib].glob[loc]]), tl, block=ib)


def run_a(K, nsteps, graph=True, nblocks=1, transport="copies", off=(), bucket=0.0, first=1, restart=None,
          fields_first=True, save_restart_at=None, output_calls_at=None):
    """Runner A.  off: hooks left out ("physics", "iau", "lbc", "kessler").  restart: the images of
    save_restart_at of an earlier run; the context starts from them (restart_diagnostics) at step ``first``,
    uploaded before (fields_first) or after the hooks are set.  output_calls_at: after that step the three
    output-time diagnostics run once.  Returns (per-step dicts of global element-major arrays, extra)."""
    from mpas_dycore import Dycore, decomp
    from mpas_dycore import fields as F
    case, lbc, inc, phys = _forecast(K)
    dt, window = float(case["dt"]), inc["window"]
    full = dict(case, **{n: inc[n] for n in F.IAU_FIELD})
    if "lbc" in off:  # set_lbc left off: the relaxation zone's masks stay, the specified zone goes (test_each_hook_acts)
        full.update(bdyMaskCell=np.minimum(case["bdyMaskCell"], 5), bdyMaskEdge=np.minimum(case["bdyMaskEdge"], 5),
                    specZoneMaskCell=case["specZoneMaskCell"] * 0.0, specZoneMaskEdge=case["specZoneMaskEdge"] * 0.0)
    if nblocks == 1:
        blocks = None
        dy = Dycore(full, device=0, moist_end=NS)
    else:
        blocks = decomp.decompose(full, partition(case, K))
        assert len(blocks) == nblocks and all("scalars_amb" in b.case for b in blocks)
        kw = {} if transport == "copies" else dict(comm_id=Dycore.comm_unique_id(), nranks=1, rank=0, rccl_local=True,
                                                   p2p=transport == "p2p")
        dy = Dycore.from_blocks(blocks, device=0, moist_end=NS, **kw)
        if transport != "copies":
            dy.set_overlap(transport == "rccl")
    n_glob = {"cell": case["nCells"], "edge": case["nEdges"]}

    def local(a, ib, loc):
        return _img(a if blocks is None else a[blocks[ib].glob[loc]])

    def gather(pool, name, loc):
        def get(ib):  # i_rainnc as fp64: gather_owned fills the elements no block owns with NaN
            a = dy.get(pool, name, 1, block=ib)
            return a.astype(np.float64) if a.dtype == np.int32 else a
        if blocks is None:
            return get(0)
        return decomp.gather_owned(blocks, [get(i) for i in range(nblocks)], loc, n_glob[loc])

    def hooks():
        if "physics" not in off:
            dy.set_physics(tendencies=True)
            for ib in range(nblocks):
                for n in PHYS:
                    dy.set_raw("tend_physics", n, local(phys[n], ib, "edge" if n == "tend_ru_physics" else "cell"), block=ib)
        if "iau" not in off:
            dy.set_iau(True, window)
        if "kessler" not in off:
            dy.set_microphysics("kessler", 2, 3, bucket)
        dy.set_diag_update()
        dy.set_summary(global_minmax_vel=True, global_minmax_sca=True)

    def upload_restart():
        for (pool, n), img in restart.items():
            dy.set_raw(pool, n, img, 1)

    if "lbc" not in off:
        _set_lbc_pool(dy, case, lbc, blocks)
    if restart is None:
        dy.init_diagnostics(dt)
        dy.use_graph(graph)
        hooks()
    else:
        assert blocks is None
        dy.use_graph(graph)
        if fields_first:
            upload_restart()
            hooks()
        else:
            hooks()
            upload_restart()
        dy.restart_diagnostics(dt)
    if output_calls_at is not None:
        dy.set_isobaric()
        dy.set_pv()
        dy.set_convective()
    extra = {"active": [], "captures": [], "summary": [], "blocks": blocks,
             "rtheta_base": gather("diag", "rtheta_base", "cell")}
    out = []
    for it in range(first, first + nsteps):
        if "physics" not in off:  # IAU adds to scalars_tend in place
            for ib in range(nblocks):
                dy.set_raw("tend", "scalars_tend", local(phys["scalars_tend"], ib, "cell"), block=ib)
        if "lbc" not in off:
            dy.set_lbc(True, _dtr(lbc, dt, it))
        dy.atm_timestep(dt, it)
        extra["active"].append(dy.graph_active())
        extra["captures"].append(dy.graph_captures())
        dy.shift_time_levels()
        dy.diag_update()
        dy.synchronize()
        s = {n: gather("state", n, loc) for n, loc in STATE}
        s["rtheta_p"] = gather("diag", "rtheta_p", "cell")
        if "kessler" not in off:
            s.update({n: gather(p, n, "cell")[:, 0] for p, n in ACC})
        s.update({n: gather("diag", n, "cell")[:, 0] for n in MAXIMA})
        out.append(s)
        sm = dy.summarize_timestep()
        extra["summary"].append({k: sm[k] for k in SUMMARY_KEYS})
        if it == save_restart_at:
            assert blocks is None
            r = {("state", n): dy.get_raw("state", n, 1) for n, _ in STATE}
            r.update({("diag", n): dy.get_raw("diag", n) for n in RESTART_DIAG + ("surface_pressure",) + MAXIMA})
            r[("tend", "rt_diabatic_tend")] = dy.get_raw("tend", "rt_diabatic_tend")
            r.update({("diag_physics", n): dy.get_raw("diag_physics", n) for n in ("rainnc", "rainncv", "i_rainnc", "precipw")})
            extra["restart"] = r
        if it == output_calls_at:
            dy.isobaric_diagnostics()
            dy.pv_diagnostics()
            dy.convective_diagnostics()
            dy.synchronize()
            assert dy.graph_captures() == extra["captures"][-1], "an output-time call captured or dropped a graph"
            for n, loc in STATE:
                assert np.array_equal(gather("state", n, loc), s[n]), f"{n} changed by the output-time calls"
    dy.close()
    return out, extra


def run_b(K, nsteps):
    """Runner B.  Returns (per-step dicts, extra): extra["kessler"] the scheme's loop counters,
    extra["pre_reset"] per step the specified zone's (theta_m, scalars) of time level 2 after the
    microphysics and before finish_step's reset."""
    from mpas_dycore import Dycore, convective, kessler as ks
    case, lbc, inc, phys = _forecast(K)
    dt, window = float(case["dt"]), inc["window"]
    n = case["nCells"]
    spec = np.asarray(case["bdyMaskCell"]) > 5
    dy = Dycore(case, device=0, moist_end=NS)
    _set_lbc_pool(dy, case, lbc, None)
    dy.init_diagnostics(dt)
    dy.set_physics(tendencies=True, microphysics=True)
    static = {"zz": np.asarray(case["zz"]), "zgrid": np.asarray(case["zgrid"]),
              "rtheta_base": dy.get("diag", "rtheta_base"), "exner_base": dy.get("diag", "exner_base"),
              "pressure_base": dy.get("diag", "pressure_base")}
    acc = {"rainnc": np.zeros(n), "i_rainnc": np.zeros(n, dtype=np.int32), "surface_pressure": np.zeros(n)}
    maxima = convective.zeros(case)
    out, extra = [], {"resplit": 0, "nfall0": 0, "pre_reset": []}
    for it in range(1, nsteps + 1):
        dy.synchronize()
        assert dy.iau_weight(dt, it) == 0.0  # IAU is off in B: the weight is the test's own
        wgt = 1.0 / window if it <= 3 else 0.0
        t = iau_terms(wgt, inc, case["zz"], dy.get("diag", "rho_edge"), dy.get("state", "rho_zz", 1),
                      dy.get("state", "theta_m", 1), dy.get("state", "scalars", 1), phys)
        for nm in PHYS:
            dy.set_raw("tend_physics", nm, _img(t[nm]))
        dy.set_raw("tend", "scalars_tend", _img(t["scalars_tend"]))
        dy.set_lbc(True, _dtr(lbc, dt, it))
        dy.atm_timestep(dt, it)
        dy.synchronize()
        f = dict(static, **acc, theta_m=dy.get("state", "theta_m", 2), rho_zz=dy.get("state", "rho_zz", 2),
                 scalars=dy.get("state", "scalars", 2), exner=dy.get("diag", "exner"))
        o = ks.driver(f, dt)
        extra["resplit"] += int(o["info"]["resplit"].sum())
        extra["nfall0"] = max(extra["nfall0"], int(o["info"]["nfall0"].max()))
        extra["pre_reset"].append((o["theta_m"][spec].copy(), o["scalars"][spec].copy()))
        acc = {k: o[k] for k in acc}
        dy.set_raw("state", "theta_m", _img(o["theta_m"]), 2)
        dy.set_raw("state", "scalars", _img(o["scalars"]), 2)
        for p, nm in (("diag", "rtheta_p"), ("diag", "exner"), ("diag", "pressure_p"), ("tend", "rt_diabatic_tend")):
            dy.set_raw(p, nm, _img(o[nm]))
        dy.finish_step(dt)
        dy.shift_time_levels()
        dy.synchronize()
        s = {nm: dy.get("state", nm, 1) for nm, _ in STATE}
        maxima = convective.update(case, s["w"], dy.get("diag", "vorticity"), dy.get("diag", "uReconstructZonal"),
                                   dy.get("diag", "uReconstructMeridional"), maxima, convective.ALL)
        s.update({nm: o[nm] for nm in ("rainnc", "precipw", "surface_pressure")})
        s.update(maxima)
        out.append(s)
    dy.close()
    return out, extra


def _a(K, nsteps, **kw):
    """A run of runner A, shared between the tests that need it (never modified by them)."""
    key = (K, nsteps) + tuple(sorted(kw.items()))
    if key not in _RUNS:
        _RUNS[key] = run_a(K, nsteps, **kw)
    return _RUNS[key]


def _full_a(K):
    """The whole forecast on one block with graph replay: 6 steps at K = 26 (the capture count), else 5."""
    return _a(K, 6 if K == 26 else 5)


def _b(K):
    if ("b", K) not in _RUNS:
        _RUNS[("b", K)] = run_b(K, 5)
    return _RUNS[("b", K)]


def _finite(s, what):
    for n, a in s.items():
        assert np.all(np.isfinite(a)), f"{what}: {n} is not finite"


def _same(got, want, names, what):
    for n in names:
        assert np.array_equal(got[n], want[n]), \
            f"{what}: {n} differs on {np.count_nonzero(got[n] != want[n])} values, max |diff| {np.nanmax(np.abs(got[n] - want[n])):.3e}"


@pytest.mark.parametrize("K", [26, 27, 80])
def test_device_hooks_equal_host_composed(K):
    """A (graph replay) against B after each of five steps.  K = 27: the pair layout's odd
    instantiation and IAU's one-value form; K = 80: the wide build, Kessler in two chunks.
    Bounds: u, theta_m, rho_zz 1e-10; w and each scalar species on its own 1e-9; rainnc, precipw,
    surface_pressure and the three running maxima 1e-10 after the last step.
    Measured on an MI355X (profiles/forecast_hooks_new_tests.log), worst of the five steps and the three K:
    u 3.4e-14, theta_m 7.5e-16, rho_zz 7.3e-16, w 2.3e-13 (K = 80; 4.5e-14 at 26 and 27), qv 2.0e-15,
    qc 2.8e-14, qr 2.2e-15; after step 5 rainnc 2.7e-16, precipw 5.3e-16, surface_pressure 8.6e-16,
    w_velocity_max 3.1e-14, wind_speed_level1_max 1.7e-14, updraft_helicity_max 1.1e-13: every one more
    than 400 times inside its bound."""
    a, ex = _full_a(K)
    b, bx = _b(K)
    assert all(ex["active"])
    worst = {}
    for it in range(5):
        _finite(a[it], f"K={K} A step {it + 1}")
        _finite(b[it], f"K={K} B step {it + 1}")
        errs = {n: rel_linf(a[it][n], b[it][n]) for n in ("u", "theta_m", "rho_zz", "w")}
        errs.update(dict(zip(("qv", "qc", "qr"), rel_linf_species(a[it]["scalars"], b[it]["scalars"]))))
        progress(f"forecast K={K} step {it + 1} A vs B rel Linf: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
        for n, e in errs.items():
            worst[n] = max(worst.get(n, 0.0), e)
            tol = TIGHT if n in ("u", "theta_m", "rho_zz") else LOOSE
            assert e <= tol, f"K={K} step {it + 1} {n}: rel Linf {e:.3e} > {tol:g}"
    last = {n: rel_linf(a[4][n], b[4][n]) for n in ("rainnc", "precipw", "surface_pressure") + MAXIMA}
    progress(f"forecast K={K} worst of 5 steps: " + ", ".join(f"{n} {e:.2e}" for n, e in worst.items()))
    progress(f"forecast K={K} after step 5: " + ", ".join(f"{n} {e:.2e}" for n, e in last.items()))
    for n, e in last.items():
        assert e <= TIGHT, f"K={K} {n} after step 5: rel Linf {e:.3e} > {TIGHT:g}"
    # what keeps the comparison from passing on trivia
    assert bx["resplit"] > 0 and bx["nfall0"] > 8, (bx["resplit"], bx["nfall0"])
    assert a[4]["rainnc"].max() > 0.0 and b[4]["rainnc"].max() > 0.0
    assert all(b[4][n].max() > 0.0 for n in MAXIMA)


def _driving(lbc, name, dtr, dt):
    """mpas_atm_get_bdy_state at the end of the step: state - (dtr - dt) * tend, in that order."""
    return lbc[f"lbc_{name}_s"] - (dtr - dt) * lbc[f"lbc_{name}_t"]


def _check_specified_zone(K, a, ex, what):
    case, lbc, _, _ = _forecast(K)
    dt = float(case["dt"])
    spec = np.asarray(case["bdyMaskCell"]) > 5
    for it in range(1, 6):
        dtr = _dtr(lbc, dt, it)
        rt, rho = _driving(lbc, "rtheta_m", dtr, dt), _driving(lbc, "rho_zz", dtr, dt)   # :6394-6433
        want = {"theta_m": rt / rho, "rtheta_p": rt - ex["rtheta_base"], "scalars": _driving(lbc, "scalars", dtr, dt)}
        for n, w in want.items():                                                           # :6632-6671
            g = a[it - 1][n]
            assert np.array_equal(g[spec], w[spec]), \
                f"{what} step {it}: {n} of the specified zone is not the driving value on {np.count_nonzero(g[spec] != w[spec])} values"


def test_specified_zone_holds_the_driving_values():
    """Kessler x LBC.  At the end of a step the owned specified cells are a pure function of the driving
    data (atm_bdy_reset_speczone_values, atm_bdy_set_scalars_work: the reset after the microphysics):
    theta_m, rtheta_p and the three scalars of A equal the expression evaluated in numpy bit for bit after
    every step, on one block (K = 26) and on 4 blocks over the one-sided transfer (K = 27); the same
    cells of a run without the microphysics are bit-identical, while the relaxation zone and the
    interior differ in theta_m by more than 1e-8; and in B the microphysics had changed these cells
    (cloud or rain present, values off the driving ones) before the reset put them back.
    Measured on an MI355X: theta_m with against without Kessler, rel Linf 4.7e-3 .. 5.1e-3 in the
    relaxation zone and 4.6e-3 .. 5.0e-3 in the interior over the five steps; the specified zone 0."""
    case, lbc, _, _ = _forecast(26)
    dt = float(case["dt"])
    mask = np.asarray(case["bdyMaskCell"])
    spec = mask > 5
    a, ex = _full_a(26)
    _check_specified_zone(26, a, ex, "one block")
    a4, ex4 = _a(27, 5, nblocks=4, transport="p2p", graph=True)
    _check_specified_zone(27, a4, ex4, "4 blocks, K=27")
    off, _ = _a(26, 5, off=("kessler",))
    for it in range(5):
        for n in ("theta_m", "rtheta_p", "scalars"):
            assert np.array_equal(off[it][n][spec], a[it][n][spec]), f"step {it + 1}: {n} of the specified zone"
        for zone, sel in (("relaxation", (mask > 0) & (mask <= 5)), ("interior", mask == 0)):
            d = rel_linf(off[it]["theta_m"][sel], a[it]["theta_m"][sel])
            progress(f"forecast step {it + 1} theta_m with / without Kessler, {zone} zone: rel Linf {d:.2e}")
            assert d > ACTS, f"step {it + 1}: Kessler does not act in the {zone} zone ({d:.3e})"
    # the reset had something to undo: B's microphysics left cloud or rain, and other values than the
    # driving ones, in the specified zone
    _, bx = _b(26)
    for it, (th, sc) in enumerate(bx["pre_reset"], start=1):
        dtr = _dtr(lbc, dt, it)
        assert np.any(sc[:, :, 1:] != 0.0), f"step {it}: no cloud or rain in the specified zone before the reset"
        assert np.any(sc != _driving(lbc, "scalars", dtr, dt)[spec]), f"step {it}: scalars already the driving ones"
        assert np.any(th != (_driving(lbc, "rtheta_m", dtr, dt) / _driving(lbc, "rho_zz", dtr, dt))[spec]), \
            f"step {it}: theta_m already the driving one"


@pytest.mark.parametrize("transport,K", [("copies", 26), ("rccl", 26), ("p2p", 26), ("p2p", 27)])
def test_blocks_equal_one_block(transport, K):
    """A on 4 blocks against A on one block after each of five steps: local copies eager, RCCL
    split-phase (send to self, set_overlap) under graph replay, the one-sided transfer under graph
    replay.  The prognostics, rtheta_p, the microphysics' fields and the w / wind-speed maxima bit for bit
    on owned elements; updraft_helicity_max to 1e-10 (test_gpu_convective.py's bound across blocks; measured
    there 1.8e-16, here on an MI355X 9.0e-17 .. 1.5e-16 at K = 26 on every transport and 3.7e-17 at K = 27);
    the step's summary equal."""
    one, ex1 = _full_a(K)
    graph = transport != "copies"
    got, ex = _a(K, 5, nblocks=4, transport=transport, graph=graph)
    assert ex["active"] == [graph] * 5, ex["active"]
    names = [n for n, _ in STATE] + ["rtheta_p"] + [n for _, n in ACC] + list(MAXIMA[:2])
    own_spec = [int((np.asarray(b.case["bdyMaskCell"])[:b.solve[0]] > 5).sum()) for b in ex["blocks"]]
    assert sum(1 for s in own_spec if s) >= 2 and 0 in own_spec, own_spec
    for it in range(5):
        _finite(got[it], f"{transport} K={K} step {it + 1}")
        _same(got[it], one[it], names, f"4 blocks ({transport}, K={K}) step {it + 1}")
        e = rel_linf(got[it][MAXIMA[2]], one[it][MAXIMA[2]])
        progress(f"forecast 4 blocks ({transport}, K={K}) step {it + 1}: updraft_helicity_max rel Linf {e:.2e}")
        assert e <= TIGHT, e
        assert ex["summary"][it] == ex1["summary"][it], (it + 1, ex["summary"][it], ex1["summary"][it])
    assert got[4]["rainnc"].max() > 0.0


def test_graph_captures_with_every_hook():
    """Six steps: replayed steps are the eager steps bit for bit, every step replays, and the capture
    count is the IAU test's [1, 2, 2, 3, 4, 4] -- one capture per time-level parity and IAU branch --
    unchanged by Kessler, the LBCs, the per-step set_lbc (a device scalar) and diag_update.  The three
    output-time calls after step 3 leave the count and the prognostics as they are (asserted in run_a)
    and the later steps bit for bit the eager ones."""
    names = [n for n, _ in STATE] + ["rtheta_p"] + [n for _, n in ACC] + list(MAXIMA)
    eager, exe = _a(26, 6, graph=False)
    assert exe["active"] == [False] * 6 and exe["captures"] == [0] * 6
    for what, (got, ex) in (("graph", _full_a(26)), ("graph + output calls", _a(26, 6, output_calls_at=3))):
        assert ex["active"] == [True] * 6, (what, ex["active"])
        assert ex["captures"] == [1, 2, 2, 3, 4, 4], (what, ex["captures"])
        for it in range(6):
            _same(got[it], eager[it], names, f"{what}, step {it + 1}")
            assert ex["summary"][it] == exe["summary"][it]


def test_restart_inside_the_window():
    """Five steps against two steps, a "restart file" and three more in a fresh context (step 3 still
    forced, 4 and 5 free): the prognostics, the accumulators and the running maxima after step 5 are the
    uninterrupted run's bit for bit.  The file holds test_gpu_restart.py's state and diag lists and, for
    the hooks, tend.rt_diabatic_tend (in the reference's restart stream), rainnc / rainncv / i_rainnc /
    precipw, surface_pressure and the three maxima, as raw images, uploaded once before the hooks are set
    and once after (d.diabatic is derived in both places).  config_bucket_rainnc is chosen from the
    bucket-free run's own rainnc so that i_rainnc increments in steps 3-5."""
    free, _ = _full_a(26)
    c = int(np.argmax(free[4]["rainnc"]))
    assert free[4]["rainnc"][c] > free[1]["rainnc"][c] > 0.0
    bucket = 0.5 * float(free[1]["rainnc"][c] + free[4]["rainnc"][c])
    want, ex = _a(26, 5, bucket=bucket, save_restart_at=2)
    assert np.any(want[4]["i_rainnc"] > want[1]["i_rainnc"]), "i_rainnc does not increment in steps 3-5"
    assert np.any(ex["restart"][("tend", "rt_diabatic_tend")] != 0.0)
    names = [n for n, _ in STATE] + ["rtheta_p"] + [n for _, n in ACC] + list(MAXIMA)
    for fields_first in (True, False):
        got, exr = run_a(26, 3, bucket=bucket, first=3, restart=ex["restart"], fields_first=fields_first)
        what = "fields before the hooks" if fields_first else "hooks before the fields"
        assert exr["captures"] == [1, 2, 3], (what, exr["captures"])   # forced, free, free on the other parity
        for it in range(3):
            _same(got[it], want[2 + it], names, f"restart ({what}), step {3 + it}")
            assert exr["summary"][it] == ex["summary"][2 + it]


def _kessler_valid_levels(case):
    """Levels on which the initial state keeps the saturation vapour pressure below half the pressure
    everywhere: where module_mp_kessler.F's qvs = ep_2 es / (p - es) means what it says."""
    from mpas_dycore import kessler as ks
    n, K = case["nCells"], case["nVertLevels"]
    zz, th = np.asarray(case["zz"]), np.asarray(case["theta"])
    qv = np.asarray(case["scalars"], dtype=np.float64).reshape(n, K, NS)[:, :, 0]
    pii = (zz * (ks.R_D / ks.P0) * (np.asarray(case["rho"]) / zz) * th * (1.0 + ks.R_V / ks.R_D * qv)) ** ks.RCV
    temp, pressure = pii * th, 1.0e5 * pii ** (1004.0 / 287.0)
    es = 1000.0 * ks.SVP1 * np.exp(ks.SVP2 * (temp - ks.SVPT0) / (temp - ks.SVP3))
    return np.all(es < 0.5 * pressure, axis=0), temp * (1.0 + ks.R_V / ks.R_D * qv) / pii


def test_each_hook_acts():
    """A with exactly one of the physics forcing, IAU, the LBCs and Kessler left off moves theta_m after
    four steps by more than 1e-8 relative to the full A: a hook that silently does nothing when another
    is on would pass every comparison above on both sides.  "LBCs off" leaves set_lbc out and, as
    test_gpu_lbc.py does for the same switch, caps the masks at 5: the relaxation zone stays, the specified
    zone, which nothing would drive, goes.

    A run that merely diverges would satisfy that, and two of these do leave the model's range, at the
    model top: the JW column reaches 45 km, where the initial state has T = 264 K at 2 hPa, so on the top
    three of the 26 levels es(T) exceeds the pressure (es / p = 1.0, 1.2, 1.3).  module_mp_kessler.F's
    qvs = ep_2 es / (p - es) is negative there, its saturation adjustment condenses cloud water that no
    vapour supplies (the host restatement, pinned to the compiled scheme, gives qc + 1.6e-3 and theta_m
    + 23 K at the top level in one call on the initial state) and the heating raises es further.  In the
    full A the physics' drying aloft times Rv/Rd theta in IAU's theta_m tendency (mpas_atm_iau.F:207-208)
    cools the top level by 17.6 K a step, which keeps es at or below p; without the physics forcing or
    without IAU that term is absent and the top level runs away (theta_m at most 1561, 1636, 2099, 10040 K
    after steps 1..4 without the forcing, 1560, 1628, 1978, 8955 K without IAU; the same eager, without the
    LBCs, and with Kessler, LBCs and nothing else; with Kessler off as well it stays at 1537 K).  That is
    the reference scheme on a column it was not made for, not the hooks.  So the hook must also be seen
    to act where nothing diverges: after step 1, with every level of every run within 100 K of the initial
    range, and after step 4 on the levels where the initial es stays below p / 2 (the lower 21), again
    within 100 K of the initial range.
    The 100 K are the reasoning's, not a measurement: the forcing, the increments and their cross term move
    theta_m by at most 53 K in four steps.
    Measured on an MI355X, rel Linf of theta_m against the full A after 4 steps / after step 1 / after 4
    steps on the lower 21 levels: without the physics forcing 5.8 / 2.8e-2 / 1.4e-2, without IAU 5.0 /
    2.7e-2 / 1.5e-2, without the LBCs 2.7e-2 / 8.9e-3 / 6.7e-3, without Kessler 5.0e-3 / 4.7e-3 / 7.5e-3;
    theta_m after step 1 at most 1561 K (initially 1537 K), after step 4 on the lower 21 levels 226 .. 1008 K
    (initially 227 .. 1000 K)."""
    case = _forecast(26)[0]
    valid, th0 = _kessler_valid_levels(case)
    assert valid.sum() == 21 and valid[:21].all()
    full, _ = _full_a(26)
    for hook in ("physics", "iau", "lbc", "kessler"):
        off, _ = _a(26, 5 if hook == "kessler" else 4, off=(hook,))
        _finite(off[3], f"without {hook}")
        d = rel_linf(off[3]["theta_m"], full[3]["theta_m"])
        d1 = rel_linf(off[0]["theta_m"], full[0]["theta_m"])
        dv = rel_linf(off[3]["theta_m"][:, valid], full[3]["theta_m"][:, valid])
        progress(f"forecast without {hook}: theta_m differs by rel Linf {d:.2e} after 4 steps, {d1:.2e} after step 1, "
                 f"{dv:.2e} after 4 steps on the levels with es < p / 2; its range after step 1 "
                 f"{off[0]['theta_m'].min():.1f} .. {off[0]['theta_m'].max():.1f} K, after step 4 on those levels "
                 f"{off[3]['theta_m'][:, valid].min():.1f} .. {off[3]['theta_m'][:, valid].max():.1f} K")
        assert d > ACTS, f"leaving {hook} out changes theta_m by {d:.3e} only"
        assert d1 > ACTS and dv > ACTS, f"leaving {hook} out acts only where the run diverges ({d1:.3e}, {dv:.3e})"
        for what, a, ref in (("step 1", off[0]["theta_m"], th0), ("step 4, es < p / 2", off[3]["theta_m"][:, valid], th0[:, valid])):
            assert ref.min() - 100.0 <= a.min() and a.max() <= ref.max() + 100.0, \
                f"without {hook}, {what}: theta_m {a.min():.1f} .. {a.max():.1f} K left the initial range {ref.min():.1f} .. {ref.max():.1f} K"


def test_microphysics_off_leaves_rt_diabatic_tend_to_the_host():
    """set_microphysics(None) after steps have run: tend.rt_diabatic_tend keeps the scheme's last values and
    the step goes on reading them -- the field is the host's to manage from then on, as on the
    host-microphysics path (include/mpas_dycore.h).  A host that zeroes it gets the step of a context that
    never had the scheme on."""
    from mpas_dycore import Dycore
    case = {n: a for n, a in _forecast(26)[0].items() if n not in REGIONAL}   # a global run: no LBCs here
    dt = float(case["dt"])

    def step(dy, it):
        dy.atm_timestep(dt, it)
        dy.shift_time_levels()
        dy.synchronize()
        return {n: dy.get("state", n, 1) for n, _ in STATE}

    dy = Dycore(case, device=0, moist_end=NS)
    dy.init_diagnostics(dt)
    dy.set_microphysics("kessler", 2, 3)
    step(dy, 1)
    left = dy.get("tend", "rt_diabatic_tend")
    restart = {("state", n): dy.get_raw("state", n, 1) for n, _ in STATE}
    restart.update({("diag", n): dy.get_raw("diag", n) for n in RESTART_DIAG})
    dy.set_microphysics(None)
    assert left.any() and np.array_equal(dy.get("tend", "rt_diabatic_tend"), left)
    kept = step(dy, 2)
    dy.close()
    # the same second step from the same fields in contexts that never had the scheme: with the field
    # put back it is the step above, with the field zero it is not
    for put_back in (True, False):
        c = Dycore(case, device=0, moist_end=NS)
        for (pool, n), img in restart.items():
            c.set_raw(pool, n, img, 1)
        if put_back:
            c.set_raw("tend", "rt_diabatic_tend", _img(left))
        c.restart_diagnostics(dt)
        got = step(c, 2)
        c.close()
        same = all(np.array_equal(got[n], kept[n]) for n, _ in STATE)
        assert same == put_back, f"rt_diabatic_tend {'put back' if put_back else 'zero'}: same step = {same}"
