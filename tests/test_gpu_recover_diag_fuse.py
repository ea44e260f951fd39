"""GPU: the w recovery in the launch of the diagnostics' cell kernel (k_recover3_diag_cells_b after
k_diag_vertices_p; the default on one block with split transport) gives the same bits as the two
kernels in the reference's order (MPAS_DYCORE_FUSE_RECOVER_DIAG=0): the launch calls the device
functions the two kernels call, and k_diag_vertices_p reads nothing the recovery writes.  Every case
runs 3 steps with graph replay and compares the state and what the two kernels and their readers
write; Dycore.folded_passes() tells "fused" from "silently fell back"."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("u", "w", "theta_m", "rho_zz", "scalars")
DIAG = ("h_divergence", "ke", "pv_edge", "divergence", "ru", "rw")
SWITCH = "MPAS_DYCORE_FUSE_RECOVER_DIAG"
FOLD = "recover_diag"


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


def _run(case, fused, dt=2880.0, nsteps=3):
    dy = _create(case, fused)
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


def _jw(K=26, **config):
    from mpas_dycore.cases import jw_case
    case = jw_case(642, K=K, ns=1, order=3, cache=False)
    case["config"] = dict(case["config"], **config)
    return case


def test_default_namelist():
    """Stages 1 and 2 with the next stage's h_divergence in the recovery, stage 3 without."""
    _check(_jw())


@pytest.mark.parametrize("K", [25, 63])
def test_level_counts(K):
    """An odd K, and K = 63, where w's level K is on lane 63 of the recovery's shifts."""
    _check(_jw(K=K))


def test_order2():
    _check(_jw(config_time_integration_order=2, config_number_of_sub_steps=2))


def test_moist(moist_case):
    _check(moist_case)


def test_variable_resolution(varres_case_small):
    """maxEdges = 7: pentagons with fewer edges than the record holds, and heptagons."""
    _check(varres_case_small, dt=float(varres_case_small["dt"]))


def test_transport_in_dynamics_keeps_the_kernels(moist_case):
    """The scalar transport runs between the recovery and the diagnostics: not fused, same bits."""
    case = dict(moist_case)
    case["config"] = dict(case["config"], config_split_dynamics_transport=False)
    _check(case, want=False)


def test_blocks_are_not_fused(moist_case):
    dy = _create(moist_case, True, blocks=4)
    assert FOLD not in dy.folded_passes()
    dy.close()
