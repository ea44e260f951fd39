"""GPU: the averaging of ruAvg / wwAvg over the dynamics substeps done by stage 3's last damping and
cell phase (k_divdamp_p<true>, the recovery of k_acoustic_cells_r<ME, true> /
k_dyn_cells3_acoustic_r<ME, false, true>; the default on one block with split transport) gives the
same bits as k_substep_finish_v (MPAS_DYCORE_FOLD_SUBSTEP_AVG=0): the same sum and product on the
value the kernel was about to store.  Every case runs 3 steps with graph replay and compares the
state, the two averages, their running sums and the coupled momenta; Dycore.folded_passes() tells
"folded" from "silently fell back"."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("u", "w", "theta_m", "rho_zz", "scalars")
DIAG = ("ruAvg", "wwAvg", "ruAvg_split", "wwAvg_split", "ru", "rw")
SWITCH = "MPAS_DYCORE_FOLD_SUBSTEP_AVG"
FOLD = "substep_avg"


def _create(case, folded, blocks=0):
    """A context created with the switch set (the library reads it then)."""
    from mpas_dycore import Dycore, decomp
    saved = os.environ.get(SWITCH)
    if folded:
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


def _run(case, folded, dt=2880.0, nsteps=3):
    dy = _create(case, folded)
    dy.init_diagnostics(dt)
    dy.use_graph(True)
    for i in range(nsteps):
        dy.atm_timestep(dt, i + 1)
        dy.shift_time_levels()
    dy.synchronize()
    out = {"state." + n: dy.get("state", n, 1) for n in STATE}
    out.update({"diag." + n: dy.get("diag", n) for n in DIAG})
    folds, graph = dy.folded_passes(), dy.graph_active()
    dy.close()
    return out, folds, graph


def _check(case, **kw):
    got, folds, graph = _run(case, True, **kw)
    ref, ref_folds, ref_graph = _run(case, False, **kw)
    assert FOLD in folds, f"folded passes {folds}"
    assert FOLD not in ref_folds, f"switch off, but folded passes {ref_folds}"
    assert graph and ref_graph
    for n in ref:
        assert np.all(np.isfinite(ref[n])), n
        assert np.array_equal(got[n], ref[n]), f"{n}: {int(np.count_nonzero(got[n] != ref[n]))} values differ"
    assert np.any(ref["diag.ruAvg_split"] != 0.0)


def _jw(K=26, **config):
    from mpas_dycore.cases import jw_case
    case = jw_case(642, K=K, ns=1, order=3, cache=False)
    case["config"] = dict(case["config"], **config)
    return case


def test_default_namelist():
    """Three dynamics substeps: a first, a middle and a last one."""
    _check(_jw())


# (namelist, dt); dt keeps the acoustic sub-step at 480 s
@pytest.mark.parametrize("config,dt", [
    (dict(config_dynamics_split_steps=1), 960.0),   # the first substep is the last one
    (dict(config_dynamics_split_steps=2), 1920.0),  # no middle substep
    # stage 3 has one sub-step: its recovery runs in the launch of the tendencies' last cell kernel
    (dict(config_number_of_sub_steps=1), 1440.0),
    (dict(config_number_of_sub_steps=4), 2880.0),
    (dict(config_time_integration_order=2, config_number_of_sub_steps=2), 2880.0),
], ids=["split1", "split2", "substeps1", "substeps4", "order2"])
def test_namelist_variants(config, dt):
    _check(_jw(**config), dt=dt)


@pytest.mark.parametrize("K", [25, 63])
def test_level_counts(K):
    """An odd K (the pair layout's last pair holds one level), and K = 63, where wwAvg's level K is
    on lane 63."""
    _check(_jw(K=K))


def test_moist(moist_case):
    _check(moist_case)


def test_variable_resolution(varres_case_small):
    """maxEdges = 7."""
    _check(varres_case_small, dt=float(varres_case_small["dt"]))


def test_blocks_are_not_folded(moist_case):
    dy = _create(moist_case, True, blocks=4)
    assert FOLD not in dy.folded_passes()
    dy.close()


def test_regional_is_not_folded():
    from mpas_dycore import Dycore
    from mpas_dycore.cases import jw_case, regional_lbc
    from oracle import ref_runner
    case, lbc = regional_lbc(jw_case(2562, K=26, ns=3, moist=True, cache=False))
    dy = Dycore(case, device=0, moist_end=case["num_scalars"])
    for (name, tl), img in ref_runner.lbc_images(case, lbc).items():
        dy.set_raw("lbc", name, img, tl)
    dy.set_lbc(True, lbc["interval_end"])
    assert FOLD not in dy.folded_passes()
    dy.close()
