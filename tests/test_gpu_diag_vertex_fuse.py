"""GPU: the diagnostics' cell kernel forming vorticity, ke_vertex and pv_vertex of its own vertices
from u at the cell's edges and spokes (diag_cells_vtx_col; the default on one block whose mesh
passes the record's checks) gives the same bits as k_diag_vertices_p followed by the cell kernel
that gathers what it stored (MPAS_DYCORE_FUSE_DIAG_VERTICES=0): both evaluate diag_vertex_vals on
the same three values in edgesOnVertex order.  Every case runs init_diagnostics and 3 steps with
graph replay and compares the state and what the diagnostics and their readers write;
Dycore.folded_passes() tells "fused" from "silently fell back"."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("u", "w", "theta_m", "rho_zz", "scalars")
DIAG = ("ke", "pv_cell", "pv_vertex", "vorticity", "divergence", "pv_edge", "rho_edge", "v", "gradPVt", "gradPVn",
        "h_divergence", "ru", "rw")
SWITCH = "MPAS_DYCORE_FUSE_DIAG_VERTICES"
FOLD = "diag_vertices"


def _create(case, fused, blocks=0, env=None):
    """A context created with the switch (and env, further switches) set: the library reads them then."""
    from mpas_dycore import Dycore, decomp
    want = dict(env or {})
    want[SWITCH] = None if fused else "0"  # None: the default
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


def _run(case, fused, dt=2880.0, nsteps=3, env=None):
    dy = _create(case, fused, env=env)
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


def _same(got, ref):
    for n in ref:
        assert np.all(np.isfinite(ref[n])), n
        assert np.array_equal(got[n], ref[n]), f"{n}: {int(np.count_nonzero(got[n] != ref[n]))} values differ"


def _check(case, want=True, **kw):
    got, folds, graph = _run(case, True, **kw)
    ref, ref_folds, ref_graph = _run(case, False, **kw)
    assert (FOLD in folds) == want, f"folded passes {folds}"
    assert FOLD not in ref_folds, f"switch off, but folded passes {ref_folds}"
    assert graph and ref_graph
    _same(got, ref)


def _jw(K=26, **config):
    from mpas_dycore.cases import jw_case
    case = jw_case(642, K=K, ns=1, order=3, cache=False)
    case["config"] = dict(case["config"], **config)
    return case


def test_default_namelist():
    _check(_jw())


def test_after_init_diagnostics():
    """The model-init call (the plain cell-kernel form), which stores vorticity and divergence."""
    out = []
    for fused in (True, False):
        dy = _create(_jw(), fused)
        dy.init_diagnostics(2880.0)
        dy.synchronize()
        assert (FOLD in dy.folded_passes()) == fused
        out.append({"diag." + n: dy.get("diag", n) for n in DIAG})
        dy.close()
    _same(out[0], out[1])


@pytest.mark.parametrize("K", [25, 63])
def test_level_counts(K):
    """An odd K, and K = 63, the last level count of the one-wavefront column."""
    _check(_jw(K=K))


def test_order2():
    _check(_jw(config_time_integration_order=2, config_number_of_sub_steps=2))


def test_moist(moist_case):
    _check(moist_case)


def test_variable_resolution(varres_case_small):
    """maxEdges = 7: pentagons' masked slots, the wrap of slot 0 at 5, 6 and 7 edges, heptagons, and
    the spoke at each of the three places of edgesOnVertex."""
    _check(varres_case_small, dt=float(varres_case_small["dt"]))


def test_without_the_recovery_in_the_launch():
    """MPAS_DYCORE_FUSE_RECOVER_DIAG=0: every call runs the plain cell-kernel form, vertices still fused."""
    _check(_jw(), env={"MPAS_DYCORE_FUSE_RECOVER_DIAG": "0"})


def test_transport_in_dynamics(moist_case):
    """The scalar transport runs between the recovery and the diagnostics: the plain cell-kernel form."""
    case = dict(moist_case)
    case["config"] = dict(case["config"], config_split_dynamics_transport=False)
    _check(case)


def test_rolled_vertex_slots_keep_the_vertex_kernel():
    """verticesOnCell and kiteForCell rolled by one slot within each cell's nEdgesOnCell entries: slot i
    no longer touches edges i and i-1, the record's check fails, and the context runs the vertex kernel."""
    case = _jw()
    ne = np.asarray(case["nEdgesOnCell"])
    for n in ("verticesOnCell", "kiteForCell"):
        a = np.array(case[n])
        for c in range(a.shape[0]):
            a[c, :ne[c]] = np.roll(a[c, :ne[c]], 1)
        case[n] = a
    _check(case, want=False)


def test_blocks_are_not_fused(moist_case):
    dy = _create(moist_case, True, blocks=4)
    assert FOLD not in dy.folded_passes()
    dy.close()
