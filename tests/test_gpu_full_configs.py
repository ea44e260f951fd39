"""GPU parity at BASELINE.json's full sizes: configs[2], [3] and [4] at their own meshes.

north_star bar: relative L-infinity <= 1e-10 on u / theta_m / rho_zz after 10 RK3 steps vs the
reference Fortran dycore on the same mesh and initial state (w and the mixing ratios <= 1e-9,
relative to their own maximum).  The oracle is the unmodified reference atm_srk3
(oracle/_ref/mpas_ref_harness, built from /root/reference by oracle/Makefile; it travels to the
box as a binary) run on the GPU box's host cores, 16 OpenMP threads.

  * configs[2]: x1.163842 x 56, dry JW, dt = 360 s, config_time_integration_order = 3:
    10 steps vs the reference; the same mesh as 8 MPAS blocks exchanging through RCCL
    (send/recv to self, split-phase) -- the 8-GPU decomposition on one device -- bitwise equal
    to the one-block run;
  * configs[3]: the same mesh, num_scalars = 6 (all moist species), monotone split transport,
    10 steps vs the reference;
  * configs[4]: the 60-3 km variable-resolution SCVT of 835586 cells (x20.835586's size and range:
    generators relaxed offline by tools/make_varres_mesh.py, triangulated on the box by
    mesh.varres_from_generators; pentagons, hexagons and heptagons, maxEdges = 7), 56 levels,
    config_time_integration_order = 3: 10 steps vs the reference, and 8 RCCL blocks (cells of very
    different sizes per block) bitwise equal to one block.

Cases are built on the box (about a minute at 163842, a few at 835586) and cached under
$MPAS_DYCORE_CACHE (default ~/.cache/mpas_dycore), where bench.py finds them too.
Progress lines go to the real stderr so a long run shows it is alive.
"""
import numpy as np
import pytest

from conftest import heartbeat, progress, rel_linf

pytestmark = [pytest.mark.gpu, pytest.mark.slow]

PROG = [("state", "u", "state.u.tl1", "edge"), ("state", "theta_m", "state.theta_m.tl1", "cell"),
        ("state", "rho_zz", "state.rho_zz.tl1", "cell"), ("state", "w", "state.w.tl1", "cell"),
        ("state", "scalars", "state.scalars.tl1", "cell")]
DUMP = ["state.u", "state.theta_m", "state.rho_zz", "state.w", "state.scalars"]
TOL = 1e-10          # u, theta_m, rho_zz (north_star)
TOL_LOOSE = 1e-9     # w and the mixing ratios


def _reference(case, nsteps, moist_end=1):
    from oracle import ref_runner
    if not ref_runner.available():
        pytest.skip("oracle/_ref not built")
    with heartbeat(f"reference: {nsteps} steps on {case['nCells']} cells"):
        res, times = ref_runner.run_reference(case, nsteps=nsteps, dt=float(case["dt"]), dump_steps=[nsteps],
                                              nthreads=16, moist_end=moist_end, dump_only=DUMP)
    progress(f"reference done, s/step {np.round(times, 2).tolist()}")
    return res[nsteps]


def _check(got, ref):
    errs = {key: rel_linf(got[key].reshape(ref[key].shape), ref[key]) for key in got}
    bad = {k: v for k, v in errs.items()
           if not v <= (TOL if k in ("state.u.tl1", "state.theta_m.tl1", "state.rho_zz.tl1") else TOL_LOOSE)}
    assert not bad, f"rel Linf above tolerance: {bad} (all: {errs})"
    progress(f"rel Linf vs reference {errs}")
    return errs


def _run(dy, dt, nsteps):
    dy.init_diagnostics(dt)
    dy.use_graph(True)
    for it in range(nsteps):
        dy.atm_timestep(dt, it + 1)
        dy.shift_time_levels()
    dy.synchronize()


def _single(case, nsteps, moist_end=1):
    from mpas_dycore import Dycore
    with heartbeat(f"GPU one block: {nsteps} steps"):
        dy = Dycore(case, device=0, moist_end=moist_end)
        _run(dy, float(case["dt"]), nsteps)
        out = {key: dy.get(pool, name, 1) for pool, name, key, _ in PROG}
        dy.close()
    return out


def _blocks_rccl(case, nblocks, nsteps, single, moist_end=1):
    """nblocks MPAS blocks on one device, every block-to-block halo message through RCCL (send to
    self), split-phase exchanges on: bitwise equal to the one-block run."""
    from mpas_dycore import Dycore, decomp
    with heartbeat(f"{nblocks}-block decomposition"):
        blocks = decomp.decompose(case, decomp.partition_sfc(case["nCells"], nblocks))
    dy = Dycore.from_blocks(blocks, device=0, comm_id=Dycore.comm_unique_id(), nranks=1, rank=0,
                            rccl_local=True, moist_end=moist_end)
    dy.set_overlap(True)
    _run(dy, float(case["dt"]), nsteps)
    n_glob = {"cell": case["nCells"], "edge": case["nEdges"]}
    for pool, name, key, loc in PROG:
        per = [dy.get(pool, name, 1, block=i) for i in range(len(blocks))]
        got = decomp.gather_owned(blocks, per, loc, n_glob[loc])
        assert np.array_equal(got, single[key]), f"{key}: {nblocks} RCCL blocks differ from one block"
    dy.close()
    progress(f"{nblocks} RCCL blocks bitwise equal to one block")


# ---------------------------------------------------------------- configs[2]: x1.163842 x 56 dry

@pytest.fixture(scope="module")
def dry163842():
    from mpas_dycore.cases import jw_case
    with heartbeat("building x1.163842 x 56 dry case (order 3)"):
        c = jw_case(163842, K=56, ns=1, order=3)
    assert c["config"]["config_time_integration_order"] == 3
    return c


@pytest.fixture(scope="module")
def dry163842_gpu(dry163842):
    return _single(dry163842, 10)


def test_configs2_x1_163842_L56_dry_10_steps_matches_reference(dry163842, dry163842_gpu):
    _check(dry163842_gpu, _reference(dry163842, 10))


def test_configs2_x1_163842_L56_eight_rccl_blocks_bitwise(dry163842, dry163842_gpu):
    _blocks_rccl(dry163842, 8, 10, dry163842_gpu)


def test_configs2_dropin_fortran_host_ms_per_dt(dry163842, dry163842_gpu):
    """The Fortran drop-in under the harness driver (mpas_atm_core.F's calls) at configs[2]: same
    bits as the Python host, and its ms/dt -- the wall time of steps 3..10, device wait included --
    within 10 % of the Python host's on the same case (no per-step copy-back: the state stays in
    HBM until atm_dycore_to_host)."""
    import time
    from mpas_dycore import Dycore
    from oracle import ref_runner
    if not ref_runner.available(ref_runner.DROPIN_HARNESS):
        pytest.skip("drop-in harness not built")
    c, n, dt = dry163842, 10, float(dry163842["dt"])
    with heartbeat("drop-in harness: 10 steps at 163842 x 56"):
        res, times, total = ref_runner.run_reference(c, nsteps=n, dt=dt, dump_steps=[n], nthreads=1,
                                                     dump_only=DUMP, binary=ref_runner.DROPIN_HARNESS,
                                                     with_total=True)
    for _, _, key, _ in PROG:
        a = res[n][key]
        assert np.array_equal(a, dry163842_gpu[key].reshape(a.shape)), f"{key}: drop-in differs from the Python host"
    # steps 3..n: the first launch of each time-level parity's graph loads its kernels
    ms_dropin = 1e3 * total["after2"] / (n - 2)
    dy = Dycore(c, device=0)
    dy.init_diagnostics(dt)
    dy.use_graph(True)
    for it in range(2):
        dy.atm_timestep(dt, it + 1)
        dy.shift_time_levels()
    dy.synchronize()
    t0 = time.perf_counter()
    for it in range(2, n):
        dy.atm_timestep(dt, it + 1)
        dy.shift_time_levels()
    dy.synchronize()
    ms_py = 1e3 * (time.perf_counter() - t0) / (n - 2)
    dy.close()
    progress(f"drop-in {ms_dropin:.2f} ms/dt, Python host {ms_py:.2f} ms/dt (host step calls {np.round(times, 4).tolist()})")
    assert ms_dropin <= 1.10 * ms_py, f"drop-in {ms_dropin:.2f} ms/dt vs Python host {ms_py:.2f}"


# ---------------------------------------------------------------- configs[3]: moist ns=6, monotone

def test_configs3_x1_163842_L56_moist_ns6_mono_10_steps_matches_reference():
    from mpas_dycore.cases import jw_case
    with heartbeat("building x1.163842 x 56 moist ns=6 case (order 3)"):
        c = jw_case(163842, K=56, ns=6, moist=True, order=3)
    assert c["config"]["config_monotonic"] and c["num_scalars"] == 6
    got = _single(c, 10, moist_end=6)
    _check(got, _reference(c, 10, moist_end=6))


# ---------------------------------------------------------------- configs[4]: var-res ~835586

@pytest.fixture(scope="module")
def varres835586():
    from mpas_dycore.cases import varres_case
    with heartbeat("building the 835586-cell 60-3 km variable-resolution case (order 3)"):
        c = varres_case(835586, ratio=20.0, K=56, ns=1, order=3)
    noc = np.asarray(c["nEdgesOnCell"])
    assert c["nCells"] == 835586 and c["maxEdges"] == 7 and (noc == 7).sum() > 0 and (noc == 5).sum() > 0
    assert 2.0e3 < c["dcEdge"].min() < 3.6e3 and 50e3 < c["dcEdge"].max() < 75e3, "not a 60-3 km mesh"
    assert c["config"]["config_time_integration_order"] == 3
    progress(f"x20.835586: dcEdge {c['dcEdge'].min() / 1e3:.2f}-{c['dcEdge'].max() / 1e3:.1f} km, "
             f"{int((noc == 5).sum())} pentagons, {int((noc == 7).sum())} heptagons, dt {c['dt']:g} s")
    return c


def test_configs4_varres_835586_L56_10_steps_matches_reference_and_8_blocks(varres835586):
    c = varres835586
    got = _single(c, 10)
    _check(got, _reference(c, 10))
    _blocks_rccl(c, 8, 10, got)
