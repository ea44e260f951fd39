"""GPU: stage 1's edge kernel with k_dyn_edges_rk1b_b's work folded in (k_dyn_edges_p<true, NE2,
true, ODD, true> after k_dyn_delsq_vc_p: the del4 term of tend_u_euler, the Rayleigh term, the final
tend_u and the pack of its exchange; the default in the pair layout) gives the same bits as the
separate kernel (MPAS_DYCORE_FOLD_RK1_EDGES=0): the same expressions on the tend_u, u and rho_edge
the kernel already holds.  Every case runs 3 steps with graph replay and compares the state, tend_u,
tend_u_euler and ru; Dycore.folded_passes() tells "folded" from "silently fell back"."""
import os

import numpy as np
import pytest

from conftest import physics_forcing

pytestmark = pytest.mark.gpu

STATE = ("u", "w", "theta_m", "rho_zz", "scalars")
DIAG = ("ru",)
TEND = ("u", "u_euler")
SWITCH = "MPAS_DYCORE_FOLD_RK1_EDGES"
FOLD = "rk1_edges"


def _img(a):
    out = np.zeros((a.shape[0] + 1,) + a.shape[1:])
    out[:-1] = a
    return out


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


def _run(case, folded, dt=2880.0, physics=False, nsteps=3, blocks=0):
    dy = _create(case, folded, blocks)
    dy.init_diagnostics(dt)
    if physics:
        phys = physics_forcing(case)
        dy.set_physics(tendencies=True)
        for n in ("tend_ru_physics", "tend_rtheta_physics", "tend_rho_physics"):
            dy.set_raw("tend_physics", n, _img(phys[n]))
    dy.use_graph(True)
    for i in range(nsteps):
        if physics:
            dy.set_raw("tend", "scalars_tend", _img(phys["scalars_tend"]))
        dy.atm_timestep(dt, i + 1)
        dy.shift_time_levels()
    dy.synchronize()
    out = {}
    for b in range(max(blocks, 1)):
        out.update({f"{b}.state.{n}": dy.get("state", n, 1, block=b) for n in STATE})
        out.update({f"{b}.diag.{n}": dy.get("diag", n, block=b) for n in DIAG})
        out.update({f"{b}.tend.{n}": dy.get("tend", n, block=b) for n in TEND})
    folds, graph = dy.folded_passes(), dy.graph_active()
    dy.close()
    return out, folds, graph


def _check(case, want_fold=True, **kw):
    got, folds, graph = _run(case, True, **kw)
    ref, ref_folds, ref_graph = _run(case, False, **kw)
    assert (FOLD in folds) == want_fold, f"folded passes {folds}"
    assert FOLD not in ref_folds, f"switch off, but folded passes {ref_folds}"
    assert graph == ref_graph and (graph or kw.get("blocks"))
    for n in ref:
        assert np.all(np.isfinite(ref[n])), n
        assert np.array_equal(got[n], ref[n]), f"{n}: {int(np.count_nonzero(got[n] != ref[n]))} values differ"
    assert np.any(ref["0.tend.u_euler"] != 0.0)


def _jw(K=26, **config):
    from mpas_dycore.cases import jw_case
    case = jw_case(642, K=K, ns=1, order=3, cache=False)
    case["config"] = dict(case["config"], **config)
    return case


def test_default_namelist():
    _check(_jw())


def test_odd_level_count():
    """K = 25: the pair layout's last pair holds one level."""
    _check(_jw(K=25))


def test_variable_resolution(varres_case_small):
    """maxEdges = 7: the form with 12 TRiSK neighbours."""
    _check(varres_case_small, dt=float(varres_case_small["dt"]))


@pytest.mark.parametrize("config", [
    # del4 off: only the final sum is left
    dict(config_horiz_mixing="2d_fixed", config_h_mom_eddy_visc4=0.0, config_h_theta_eddy_visc4=0.0),
    dict(config_rayleigh_damp_u=True, config_number_rayleigh_damp_u_levels=5,
         config_rayleigh_damp_u_timescale_days=2.0),
], ids=["del4_off", "rayleigh"])
def test_namelist_variants(config):
    _check(_jw(**config))


def test_physics_tendencies(moist_case):
    """tend_ru_physics in the final sum."""
    _check(moist_case, physics=True)


def test_blocks_pack_the_exchange(moist_case):
    """4 blocks: the folded kernel packs the final tend_u into the send buffer of its exchange."""
    _check(moist_case, blocks=4)


def test_vertical_mixing_keeps_the_kernel():
    """The vertical mixing of u stays in k_dyn_edges_rk1b_b: the fold reports off, and the switch
    changes nothing."""
    _check(_jw(config_horiz_mixing="2d_fixed", config_h_mom_eddy_visc2=2.0e5, config_h_mom_eddy_visc4=4.0e15,
               config_h_theta_eddy_visc2=1.0e5, config_h_theta_eddy_visc4=2.0e15, config_v_mom_eddy_visc2=5.0,
               config_v_theta_eddy_visc2=5.0), want_fold=False)
