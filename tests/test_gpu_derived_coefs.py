"""GPU: the acoustic cell phases form cofwr, a_tri and gamma_tri in registers, by the device
functions the coefficient kernels call, and the coefficient calls but the dt's last do not store
the three (the default) -- the same bits as with every call storing and every cell phase loading
them (MPAS_DYCORE_DERIVE_COEFS=0).  Every case runs 3 steps with graph replay and compares the
state, the acoustic fields and, after the step, the seven coefficient arrays (the pool keeps the
last call's); Dycore.folded_passes() tells "derived" from "loaded as before"."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("u", "w", "theta_m", "rho_zz", "scalars")
COEFS = ("coftz", "cofwz", "cofwr", "cofwt", "a_tri", "alpha_tri", "gamma_tri")
ACOUSTIC = ("ru_p", "rw_p", "rho_pp", "rtheta_pp", "ruAvg", "wwAvg")
DIAG = ("ru", "rw", "rw_p", "rho_pp", "rtheta_pp", "ruAvg", "wwAvg", "ruAvg_split", "wwAvg_split", "rtheta_p", "exner",
        "pressure_p") + COEFS
SWITCH = "MPAS_DYCORE_DERIVE_COEFS"
FOLD = "derived_coefs"


def _create(case, derived, blocks=0):
    """A context created with the switch set (the library reads it then)."""
    from mpas_dycore import Dycore, decomp
    saved = os.environ.get(SWITCH)
    if derived:
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


def _fields(dy, blocks=0):
    out = {}
    for b in range(max(blocks, 1)):
        out.update({f"{b}.state.{n}": dy.get("state", n, 1, block=b) for n in STATE})
        out.update({f"{b}.diag.{n}": dy.get("diag", n, block=b) for n in DIAG})
    return out


def _steps(dy, dt, nsteps, lbc=None):
    for i in range(nsteps):
        if lbc is not None:
            dy.set_lbc(True, lbc["interval_end"] - i * dt)
        dy.atm_timestep(dt, i + 1)
        dy.shift_time_levels()
    dy.synchronize()


def _run(case, derived, dt=2880.0, nsteps=3, blocks=0, lbc=None, images=None):
    dy = _create(case, derived, blocks)
    for (name, tl), img in (images or {}).items():
        dy.set_raw("lbc", name, img, tl)
    dy.init_diagnostics(dt)
    dy.use_graph(True)
    before = dy.folded_passes()
    _steps(dy, dt, nsteps, lbc)
    out = _fields(dy, blocks)
    folds, graph = dy.folded_passes(), dy.graph_active()
    dy.close()
    return out, before, folds, graph


def _equal(got, ref):
    for n in ref:
        assert np.all(np.isfinite(ref[n])), n
        assert np.array_equal(got[n], ref[n]), f"{n}: {int(np.count_nonzero(got[n] != ref[n]))} values differ"


def _check(case, **kw):
    got, before, folds, graph = _run(case, True, **kw)
    ref, _, ref_folds, ref_graph = _run(case, False, **kw)
    assert FOLD not in before, f"no coefficient call yet, but folded passes {before}"
    assert FOLD in folds, f"folded passes {folds}"
    assert FOLD not in ref_folds, f"switch off, but folded passes {ref_folds}"
    if kw.get("lbc") is None:  # a regional step's boundary time changes from step to step
        assert graph and ref_graph
    _equal(got, ref)
    assert np.any(ref["0.diag.cofwr"] != 0.0) and np.any(ref["0.diag.gamma_tri"] != 0.0)


def _jw(K=26, **config):
    from mpas_dycore.cases import jw_case
    case = jw_case(642, K=K, ns=1, order=3, cache=False)
    case["config"] = dict(case["config"], **config)
    return case


@pytest.mark.parametrize("K", [26, 25, 63])
def test_level_counts(K):
    """The default namelist (order 3, three dynamics substeps) at an even K, an odd K (the coefficient
    kernel's last pair holds one level) and K = 63, where level K sits on lane 63 of the shifts."""
    _check(_jw(K=K))


# (namelist, dt); dt keeps the acoustic sub-step at 480 s
@pytest.mark.parametrize("config,dt", [
    # order 2: the dt's last coefficient call is the last substep's start
    (dict(config_time_integration_order=2, config_number_of_sub_steps=2), 2880.0),
    (dict(config_time_integration_order=2, config_number_of_sub_steps=4), 2880.0),
    (dict(config_number_of_sub_steps=4), 2880.0),
    # one dynamics substep: at order 2 the dt's only coefficient call stores everything
    (dict(config_dynamics_split_steps=1), 960.0),
    (dict(config_dynamics_split_steps=1, config_time_integration_order=2, config_number_of_sub_steps=2), 960.0),
], ids=["order2_substeps2", "order2_substeps4", "order3_substeps4", "split1", "split1_order2"])
def test_namelist_variants(config, dt):
    _check(_jw(**config), dt=dt)


def test_moist(moist_case):
    """cqw != 1."""
    _check(moist_case)


def test_variable_resolution(varres_case_small):
    """maxEdges = 7."""
    _check(varres_case_small, dt=float(varres_case_small["dt"]))


def test_blocks(moist_case):
    """4 blocks exchanging through RCCL: every block's cell phases derive, the same bits per block."""
    _check(moist_case, blocks=4)


def test_regional():
    """LBC run: the relaxation zone solves with derived coefficients, the specified zone uses none."""
    from mpas_dycore.cases import jw_case, regional_lbc
    from oracle import ref_runner
    case, lbc = regional_lbc(jw_case(2562, K=26, ns=3, moist=True, cache=False))
    _check(case, dt=float(case["dt"]), lbc=lbc, images=ref_runner.lbc_images(case, lbc))


def _acoustic(dy):
    return {n: dy.get("diag", n) for n in ACOUSTIC}


def test_acoustic_step_with_another_dts(moist_case):
    """After 2 steps, mpas_dyc_time_acoustic_step with a sub-step that is not the step's: the derived
    coefficients take the dtseps of the last coefficient call, as the stored ones did."""
    dt = 2880.0
    cfg = moist_case["config"]
    dts = dt / cfg["config_dynamics_split_steps"] / cfg["config_number_of_sub_steps"]
    res = []
    for derived in (True, False):
        dy = _create(moist_case, derived)
        dy.init_diagnostics(dt)
        dy.use_graph(True)
        _steps(dy, dt, 2)
        assert (FOLD in dy.folded_passes()) == derived
        dy.time_acoustic_step(0.625 * dts, 2, 3)
        res.append(_acoustic(dy))
        dy.close()
    _equal(*res)
    assert np.any(res[1]["rw_p"] != 0.0)


def test_foreign_coefficient_arrays_are_loaded(moist_case):
    """A fresh context given another context's coefficient arrays by set_raw has made no coefficient
    call of its own: its cell phases load the arrays, until a step has run."""
    dt = 2880.0
    cfg = moist_case["config"]
    dts = dt / cfg["config_dynamics_split_steps"] / cfg["config_number_of_sub_steps"]
    donor = _create(moist_case, False)
    donor.init_diagnostics(dt)
    _steps(donor, dt, 1)
    images = {n: donor.get_raw("diag", n) for n in COEFS + ("cofrz",) + ACOUSTIC}
    donor.close()
    res = []
    for derived in (True, False):
        dy = _create(moist_case, derived)
        dy.init_diagnostics(dt)
        for n, img in images.items():
            dy.set_raw("diag", n, img)
        assert FOLD not in dy.folded_passes()
        dy.time_acoustic_step(dts, 2, 3)
        res.append(_acoustic(dy))
        assert FOLD not in dy.folded_passes()
        if derived:
            dy.use_graph(True)
            _steps(dy, dt, 1)
            assert FOLD in dy.folded_passes()
            dy.set_raw("diag", "alpha_tri", images["alpha_tri"])
            assert FOLD not in dy.folded_passes()
        dy.close()
    _equal(*res)
    assert np.any(res[1]["rw_p"] != 0.0)
