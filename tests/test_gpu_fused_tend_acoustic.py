"""GPU: dyn_tend's last cell kernel and the stage's first acoustic cell phase in one launch
(k_dyn_cells3_acoustic_r, the default on one block) give the same bits as the two kernels
(MPAS_DYCORE_FUSE_TEND_ACOUSTIC=0): both call the same device functions, and the fused launch only
keeps in registers what the second kernel would load again.  Every case runs 3 steps with graph
replay and compares the state, the coupled diagnostics and the two tendencies the fused launch
stores only when something reads them later; Dycore.fused_tend_acoustic() tells "fused" from
"silently fell back"."""
import os

import numpy as np
import pytest

from conftest import physics_forcing

pytestmark = pytest.mark.gpu

STATE = ("u", "w", "theta_m", "rho_zz", "scalars")
DIAG = ("ru", "rw", "rtheta_p", "rho_p", "exner", "pressure_p", "wwAvg", "ruAvg")
TEND = ("w", "theta_m")
SWITCH = "MPAS_DYCORE_FUSE_TEND_ACOUSTIC"


def _img(a):
    out = np.zeros((a.shape[0] + 1,) + a.shape[1:])
    out[:-1] = a
    return out


def _create(case, fused, blocks=0):
    """A context created with the switch set (the library reads it then)."""
    from mpas_dycore import Dycore, decomp
    saved = os.environ.get(SWITCH)
    if fused:
        os.environ.pop(SWITCH, None)  # the default
    else:
        os.environ[SWITCH] = "0"
    try:
        if blocks:
            bl = decomp.decompose(case, decomp.partition_sfc(case["nCells"], blocks))
            return Dycore.from_blocks(bl, device=0, comm_id=Dycore.comm_unique_id(), nranks=1, rank=0,
                                      rccl_local=True, moist_end=case["num_scalars"])
        return Dycore(case, device=0, moist_end=case["num_scalars"])
    finally:
        if saved is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = saved


def _run(case, fused, dt=2880.0, physics=False, nsteps=3):
    dy = _create(case, fused)
    dy.init_diagnostics(dt)
    if physics:
        phys = physics_forcing(case)
        dy.set_physics(tendencies=True)
        for n in ("tend_ru_physics", "tend_rtheta_physics", "tend_rho_physics"):
            dy.set_raw("tend_physics", n, _img(phys[n]))
        kk = (np.arange(case["nVertLevels"]) + 0.5) / case["nVertLevels"]
        dy.set_raw("tend", "rt_diabatic_tend", _img(2e-5 * np.cos(case["latCell"][:, None]) * np.exp(-3 * kk)))
    dy.use_graph(True)
    for i in range(nsteps):
        if physics:
            dy.set_raw("tend", "scalars_tend", _img(phys["scalars_tend"]))
        dy.atm_timestep(dt, i + 1)
        dy.shift_time_levels()
    dy.synchronize()
    out = {"state." + n: dy.get("state", n, 1) for n in STATE}
    out.update({"diag." + n: dy.get("diag", n) for n in DIAG})
    out.update({"tend." + n: dy.get("tend", n) for n in TEND})
    stages, graph = dy.fused_tend_acoustic(), dy.graph_active()
    dy.close()
    return out, stages, graph


def _check(case, want_stages=(1, 2, 3), **kw):
    got, stages, graph = _run(case, True, **kw)
    ref, ref_stages, ref_graph = _run(case, False, **kw)
    assert stages == want_stages, f"fused stages {stages}"
    assert ref_stages == (), f"switch off, but fused stages {ref_stages}"
    assert graph and ref_graph
    for n in ref:
        assert np.all(np.isfinite(ref[n])), n
        assert np.array_equal(got[n], ref[n]), f"{n}: {int(np.count_nonzero(got[n] != ref[n]))} values differ"


def _jw(K=26, **config):
    from mpas_dycore.cases import jw_case
    case = jw_case(642, K=K, ns=1, order=3, cache=False)
    case["config"] = dict(case["config"], **config)
    return case


def test_flagship_stage_pattern():
    """Dry, order 3, 2 sub-steps: stages of 1 / 1 / 2 sub-steps, so all three forms run
    (rk 1 with recovery, rk 2 with recovery, rk 3 without)."""
    _check(_jw())


def test_moist(moist_case):
    """cqw != 1, three species (order 2, 2 sub-steps: 1 / 1 / 2 as well)."""
    _check(moist_case)


def test_variable_resolution(varres_case_small):
    """maxEdges = 7: pentagons with fewer edges than the record holds, and heptagons."""
    _check(varres_case_small, dt=float(varres_case_small["dt"]))


@pytest.mark.parametrize("K", [25, 63])
def test_level_counts(K):
    """An odd K, and K = 63, where w's level K is on lane 63 and every lane of the shifts is live."""
    _check(_jw(K=K))


# (namelist, dt, the stages that must report fused); dt keeps the acoustic sub-step at 480 s
@pytest.mark.parametrize("config,dt,stages", [
    # the dt's last stage has one sub-step: it stores the tendencies for the pool
    (dict(config_number_of_sub_steps=1), 1440.0, (1, 2, 3)),
    # rk 2 has two sub-steps: the form without recovery at rk 2
    (dict(config_number_of_sub_steps=4), 2880.0, (1, 2, 3)),
    (dict(config_time_integration_order=2, config_number_of_sub_steps=2), 2880.0, (1, 2, 3)),
    # rk 1 has two sub-steps: it keeps the two kernels
    (dict(config_time_integration_order=2, config_number_of_sub_steps=4), 2880.0, (2, 3)),
    (dict(config_dynamics_split_steps=1), 960.0, (1, 2, 3)),
    # del4 off
    (dict(config_horiz_mixing="2d_fixed", config_h_mom_eddy_visc4=0.0, config_h_theta_eddy_visc4=0.0), 2880.0, (1, 2, 3)),
], ids=["substeps1", "substeps4", "order2", "order2_substeps4", "split1", "del4_off"])
def test_namelist_variants(config, dt, stages):
    _check(_jw(**config), want_stages=stages, dt=dt)


def test_physics_tendencies(moist_case):
    """tend_rtheta_physics in the tendencies, rt_diabatic_tend in them and in the stage-3 recovery."""
    _check(moist_case, physics=True)


def test_blocks_are_not_fused(moist_case):
    dy = _create(moist_case, True, blocks=4)
    assert dy.fused_tend_acoustic() == ()
    dy.close()


def test_regional_is_not_fused():
    from mpas_dycore import Dycore
    from mpas_dycore.cases import jw_case, regional_lbc
    from oracle import ref_runner
    case, lbc = regional_lbc(jw_case(2562, K=26, ns=3, moist=True, cache=False))
    dy = Dycore(case, device=0, moist_end=case["num_scalars"])
    assert dy.fused_tend_acoustic() == (1, 2, 3)
    for (name, tl), img in ref_runner.lbc_images(case, lbc).items():
        dy.set_raw("lbc", name, img, tl)
    dy.set_lbc(True, lbc["interval_end"])
    assert dy.fused_tend_acoustic() == ()
    dy.close()
