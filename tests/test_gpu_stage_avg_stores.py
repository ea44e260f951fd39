"""GPU: the recoveries of stages 1 and 2 store no ruAvg / wwAvg (the default on one block with split
transport: the next stage forms ruAvg afresh from dts * tend_u and its sub-step 1 zeroes wwAvg
without reading it; the transport and the substep averaging read stage 3's) and the step gives the
same bits as with every stage storing them (MPAS_DYCORE_SKIP_STAGE_AVG=0).  Every case runs 3 steps
with graph replay and compares the state, the acoustic fields, the two averages with their running
sums and the coefficient arrays; Dycore.folded_passes() tells "skipped" from "stored as before"."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("u", "w", "theta_m", "rho_zz", "scalars")
DIAG = ("ru", "rw", "rw_p", "rho_pp", "rtheta_pp", "ruAvg", "wwAvg", "ruAvg_split", "wwAvg_split", "rtheta_p", "exner",
        "pressure_p", "coftz", "cofwz", "cofwr", "cofwt", "a_tri", "alpha_tri", "gamma_tri")
SWITCH = "MPAS_DYCORE_SKIP_STAGE_AVG"
FOLD = "stage_avg_stores"


def _create(case, skipped, blocks=0, env=None):
    """A context created with the switch (and any other variable of env) set: the library reads
    them then."""
    from mpas_dycore import Dycore, decomp
    want = dict(env or {})
    want[SWITCH] = None if skipped else "0"  # None: the default
    saved = {k: os.environ.get(k) for k in want}
    for k, v in want.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        if blocks:
            bl = decomp.decompose(case, decomp.partition_sfc(case["nCells"], blocks))
            return Dycore.from_blocks(bl, device=0, comm_id=Dycore.comm_unique_id(), nranks=1, rank=0,
                                      rccl_local=True, moist_end=case["num_scalars"])
        return Dycore(case, device=0, moist_end=case["num_scalars"])
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(case, skipped, dt=2880.0, nsteps=3, env=None):
    dy = _create(case, skipped, env=env)
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


def _check(case, want=True, **kw):
    got, folds, graph = _run(case, True, **kw)
    ref, ref_folds, ref_graph = _run(case, False, **kw)
    assert (FOLD in folds) == want, f"folded passes {folds}"
    assert FOLD not in ref_folds, f"switch off, but folded passes {ref_folds}"
    assert graph and ref_graph
    for n in ref:
        assert np.all(np.isfinite(ref[n])), n
        assert np.array_equal(got[n], ref[n]), f"{n}: {int(np.count_nonzero(got[n] != ref[n]))} values differ"
    assert np.any(ref["diag.ruAvg"] != 0.0) and np.any(ref["diag.wwAvg"] != 0.0)


def _jw(K=26, **config):
    from mpas_dycore.cases import jw_case
    case = jw_case(642, K=K, ns=1, order=3, cache=False)
    case["config"] = dict(case["config"], **config)
    return case


def test_default_namelist():
    """Order 3, three dynamics substeps: stage 1 of one sub-step (its recovery runs in the launch of
    the tendencies' last cell kernel), stage 2 of several."""
    _check(_jw())


@pytest.mark.parametrize("K", [25, 63])
def test_level_counts(K):
    """An odd K (the pair layout's last pair holds one level), and K = 63, where wwAvg's level K is
    on lane 63."""
    _check(_jw(K=K))


# (namelist, dt); dt keeps the acoustic sub-step at 480 s
@pytest.mark.parametrize("config,dt", [
    (dict(config_time_integration_order=2, config_number_of_sub_steps=2), 2880.0),
    (dict(config_time_integration_order=2, config_number_of_sub_steps=4), 2880.0),  # stage 1 of two sub-steps
    (dict(config_number_of_sub_steps=4), 2880.0),
    (dict(config_dynamics_split_steps=1), 960.0),
], ids=["order2_substeps2", "order2_substeps4", "order3_substeps4", "split1"])
def test_namelist_variants(config, dt):
    _check(_jw(**config), dt=dt)


def test_moist(moist_case):
    _check(moist_case)


def test_variable_resolution(varres_case_small):
    """maxEdges = 7."""
    _check(varres_case_small, dt=float(varres_case_small["dt"]))


def test_substep_finish_kernel_reads_stage3(moist_case):
    """MPAS_DYCORE_FOLD_SUBSTEP_AVG=0: k_substep_finish_v averages what stage 3 stored."""
    _check(moist_case, env={"MPAS_DYCORE_FOLD_SUBSTEP_AVG": "0"})


def test_transport_in_dynamics_keeps_the_stores(moist_case):
    """The scalar transport after stages 1 and 2 reads their ruAvg / wwAvg: stored, same bits."""
    case = dict(moist_case)
    case["config"] = dict(case["config"], config_split_dynamics_transport=False)
    _check(case, want=False)


def test_blocks_keep_the_stores(moist_case):
    dy = _create(moist_case, True, blocks=4)
    assert FOLD not in dy.folded_passes()
    dy.close()
