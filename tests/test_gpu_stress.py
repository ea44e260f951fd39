"""GPU parity where the smooth JW case is blind: active limiter, mixing cap, namelist scalars.

The other GPU tests run the JW state with smooth Gaussian tracer blobs and compare `scalars`
with one maximum over the whole array (qv, 1.6e-2).  There the monotone limiter changes the
tracer species by 1e-7 of their own maxima after 3 steps, kdiff never reaches its cap, and seven
namelist scalars keep their defaults.  Here:

  * mpas_dycore.cases.stress_case (top-hat and noise tracers, config_smagorinsky_coef = 1;
    tests/test_stress_case.py asserts on the reference alone that 61 % of kdiff sits at the cap
    and that the limiter moves the species by 9e-2 and 1.8e-1 of their own maxima) runs 3 steps
    against the reference dycore, each species measured against its own maximum
    (rel_linf_species).  The bar is 1e-11 for every field and species: the project's 3-step
    x1.642 bar (tests/test_gpu_configs.py).  The reference's own sensitivity to one-ulp changes
    of its inputs on this state is 5.0e-14 (u), 5.9e-16 (theta_m), 3.6e-16 (rho_zz), 1.2e-12 (w)
    and 7e-15 (a species' own norm), so the bar stands 8x above that floor for w and more than
    1000x for the rest.  With the limiter's effect at 1e-1 of a species' maximum, an error above
    1e-10 of that effect (in the flux rescale, the bounds or the scale_arr exchange) breaks the
    bar; on the smooth blobs even removing the limiter cost only 2e-8 of the compared norm.
  * the kernel families, the mono / cells / delsq switches, 4 RCCL-local blocks and graph replay
    give the same bits on that state, where the scale factors are below 1;
  * diag.kdiff itself matches the reference, with the same share of entries at the cap;
  * each of config_coef_3rd_order, config_apvm_upwinding, config_del4u_div_factor,
    config_visc4_2dsmag, config_smagorinsky_coef, config_epssm and config_smdiv takes a
    non-default value on the smooth moist case, 3 steps against the reference, same bar.

Every measured error is printed through conftest.progress (one MI355X run is kept in
profiles/stress_parity_gpu.log: on the stress case u <= 9.8e-14, w <= 1.0e-12, every species
<= 2.1e-14 of its own maximum; kdiff within 3.4e-14 with the reference's share at the cap).
"""
import os

import numpy as np
import pytest

from conftest import progress, rel_linf

pytestmark = pytest.mark.gpu

DT = 2880.0
NSTEPS = 3
BAR = 1e-11
PROGNOSTICS = ("u", "theta_m", "rho_zz", "w", "scalars")


def rel_linf_species(got, ref):
    """Per species: max|got - ref| over that species alone, divided by its own max|ref| (the
    absolute difference for a species that is identically zero in the reference)."""
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    return [rel_linf(got[..., s], ref[..., s]) for s in range(ref.shape[-1])]


def _need_ref():
    from oracle import ref_runner
    if not ref_runner.available():
        pytest.skip("oracle/_ref not built")
    return ref_runner


_CASES: dict = {}
_REFS: dict = {}
_RUNS: dict = {}


def _stress(K, ns):
    from mpas_dycore.cases import stress_case
    if (K, ns) not in _CASES:
        _CASES[K, ns] = stress_case(K, ns)
    return _CASES[K, ns]


def _stress_ref(K, ns, steps=(NSTEPS,)):
    """The reference's dumps of the stress case, computed once per (K, ns, steps)."""
    key = (K, ns, tuple(steps))
    if key not in _REFS:
        res, _ = _need_ref().run_reference(_stress(K, ns), nsteps=max(steps), dt=DT, dump_steps=list(steps),
                                           nthreads=4, moist_end=ns)
        _REFS[key] = res
    return _REFS[key]


def _run(case, env=None, blocks=0, graph=True, nsteps=NSTEPS, moist_end=None, diag=()):
    """nsteps steps on the GPU with the environment variables env set while the context is created
    (the library reads its switches then); blocks > 0: that many blocks on the device, exchanging
    through RCCL.  Returns the five prognostics (and the diag fields asked for)."""
    from mpas_dycore import Dycore, decomp
    env = dict(env or {})
    moist_end = case["num_scalars"] if moist_end is None else moist_end
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        if blocks:
            bl = decomp.decompose(case, decomp.partition_sfc(case["nCells"], blocks))
            dy = Dycore.from_blocks(bl, device=0, comm_id=Dycore.comm_unique_id(), nranks=1, rank=0,
                                    rccl_local=True, moist_end=moist_end)
        else:
            dy = Dycore(case, device=0, moist_end=moist_end)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v
    dy.init_diagnostics(DT)
    dy.use_graph(graph)
    for i in range(nsteps):
        dy.atm_timestep(DT, i + 1)
        dy.shift_time_levels()
    dy.synchronize()
    if graph and not blocks:
        assert dy.graph_active()
    if blocks:
        n_glob = {"cell": case["nCells"], "edge": case["nEdges"]}
        out = {n: decomp.gather_owned(bl, [dy.get("state", n, 1, block=i) for i in range(len(bl))],
                                      "edge" if n == "u" else "cell", n_glob["edge" if n == "u" else "cell"])
               for n in PROGNOSTICS}
    else:
        out = {n: dy.get("state", n, 1) for n in PROGNOSTICS}
        out.update({n: dy.get("diag", n) for n in diag})
    dy.close()
    return out


def _default_run(K, ns):
    """The default switches on the stress case (graph replay), computed once and left unchanged."""
    if (K, ns) not in _RUNS:
        _RUNS[K, ns] = _run(_stress(K, ns))
    return _RUNS[K, ns]


def _errors(got, ref):
    """{field or species: error} of a GPU run against a reference dump, each against its own maximum."""
    errs = {n: rel_linf(got[n].reshape(ref[f"state.{n}.tl1"].shape), ref[f"state.{n}.tl1"])
            for n in ("u", "theta_m", "rho_zz", "w")}
    for s, e in enumerate(rel_linf_species(got["scalars"], ref["state.scalars.tl1"])):
        errs[f"scalars[{s}]"] = e
    return errs


def _fmt(errs):
    return " ".join(f"{k}={v:.2e}" for k, v in errs.items())


# ---------------------------------------------------------------- parity with the reference

@pytest.mark.parametrize("K,ns", [(26, 3), (55, 3), (80, 3), (150, 3), (55, 6)])
def test_stress_case_matches_reference(K, ns):
    """3 graph-replayed steps of the stress case against the reference dycore: u, theta_m, rho_zz,
    w and every species against its own maximum, all <= 1e-11."""
    ref = _stress_ref(K, ns)[NSTEPS]
    got = _default_run(K, ns)
    errs = _errors(got, ref)
    progress(f"stress parity K={K} ns={ns} steps={NSTEPS}: {_fmt(errs)}")
    sc = got["scalars"].reshape(ref["state.scalars.tl1"].shape)
    assert sc.min() >= 0.0  # the limiter and the clip leave no negative mixing ratio
    if ns == 6:
        assert not sc[..., 5].any()  # a species that is identically zero stays so
    assert np.isfinite(list(errs.values())).all()
    bad = {k: v for k, v in errs.items() if not v <= BAR}
    assert not bad, f"K={K} ns={ns}: {bad} (all {errs})"


# ---------------------------------------------------------------- bitwise equalities

SWITCHES = [{"MPAS_DYCORE_KERNELS": "general"}, {"MPAS_DYCORE_KERNELS": "batched"}, {"MPAS_DYCORE_MONO_PAIRS": "0"},
            {"MPAS_DYCORE_MONO_FUSE": "0"}, {"MPAS_DYCORE_CELLS1_PAIR": "0"}, {"MPAS_DYCORE_CELLS2_PAIR": "0"},
            {"MPAS_DYCORE_DELSQ_PAIR": "0"}]
BITWISE = [(K, ns, env) for K, ns in ((26, 3), (55, 6)) for env in SWITCHES] + \
          [(80, 3, env) for env in SWITCHES[:2]]


def _env_id(env):
    return ",".join(f"{k[len('MPAS_DYCORE_'):]}={v}" for k, v in env.items())


@pytest.mark.parametrize("K,ns,env", BITWISE, ids=[f"K{K}-ns{ns}-{_env_id(env)}" for K, ns, env in BITWISE])
def test_stress_case_switch_equals_default_bitwise(K, ns, env):
    """The kernel families and the pair / fuse switches evaluate the same expressions in the same
    order: equal bits with scale factors below 1 and kdiff at its cap."""
    ref = _default_run(K, ns)
    got = _run(_stress(K, ns), env)
    for n in PROGNOSTICS:
        assert np.array_equal(got[n], ref[n]), f"{_env_id(env)}: {n} max diff {np.abs(got[n] - ref[n]).max():.3e}"


@pytest.mark.parametrize("K,ns", [(26, 3), (55, 6)])
def test_stress_case_four_blocks_equal_one(K, ns):
    """4 blocks exchanging through RCCL equal one block bit for bit: the scale_arr exchange carries
    factors below 1 here."""
    ref = _default_run(K, ns)
    got = _run(_stress(K, ns), blocks=4)
    for n in PROGNOSTICS:
        assert np.array_equal(got[n], ref[n]), f"{n} max diff {np.abs(got[n] - ref[n]).max():.3e}"


def test_stress_case_graph_equals_eager():
    ref = _default_run(26, 3)
    got = _run(_stress(26, 3), graph=False)
    for n in PROGNOSTICS:
        assert np.array_equal(got[n], ref[n]), n


# ---------------------------------------------------------------- kdiff at the cap

@pytest.mark.parametrize("family", ["general", "batched", "pair"])
def test_stress_case_kdiff_matches_reference(family):
    """diag.kdiff after step 1 at K = 26: the same share of entries at the cap 0.01 len_disp^2 / dt
    as the reference, and rel Linf <= 1e-11."""
    case = _stress(26, 3)
    ref = _stress_ref(26, 3, steps=(1,))[1]["diag.kdiff"]
    got = _run(case, {"MPAS_DYCORE_KERNELS": family}, nsteps=1, diag=("kdiff",))["kdiff"].reshape(ref.shape)
    cap = 0.01 * case["config"]["config_len_disp"] ** 2 / DT
    share_ref = float(np.mean(ref >= cap * (1.0 - 1e-12)))
    share_got = float(np.mean(got >= cap * (1.0 - 1e-12)))
    err = rel_linf(got, ref)
    progress(f"stress kdiff K=26 step 1 {family}: at cap gpu {share_got:.4f} ref {share_ref:.4f}, rel Linf {err:.2e}")
    assert 0.3 <= share_ref <= 0.9
    assert share_got == share_ref
    assert err <= BAR


# ---------------------------------------------------------------- namelist scalars

NAMELIST = [("config_smagorinsky_coef", 0.5), ("config_coef_3rd_order", 0.0), ("config_coef_3rd_order", 1.0),
            ("config_apvm_upwinding", 0.0), ("config_apvm_upwinding", 1.0), ("config_del4u_div_factor", 1.0),
            ("config_visc4_2dsmag", 0.2), ("config_visc4_2dsmag", 0.0), ("config_epssm", 0.3), ("config_smdiv", 0.3),
            ("config_smdiv", 0.0)]
ON_GENERAL = ("config_coef_3rd_order", "config_epssm", "config_del4u_div_factor")
NAMELIST_RUNS = [(n, v, "default") for n, v in NAMELIST] + [(n, v, "general") for n, v in NAMELIST if n in ON_GENERAL]


def _smooth_case(**config):
    """The smooth moist JW case (x1.642, K = 26, ns = 3) with namelist options set through
    build_case: model_init folds config_coef_3rd_order into adv_coefs_3rd and zb3_cell."""
    from mpas_dycore import cases
    from mpas_dycore.init_atm import build_case
    cfg = dict(config_len_disp=cases.jw_len_disp(3), config_dt=cases.jw_dt(3), config_time_integration_order=2)
    cfg.update(config)
    return build_case(cases._mesh(3, 20), K=26, ns=3, moist=True, config=cfg)


@pytest.fixture(scope="module")
def smooth_default_ref():
    res, _ = _need_ref().run_reference(_smooth_case(), nsteps=NSTEPS, dt=DT, dump_steps=[NSTEPS], nthreads=4,
                                       moist_end=3)
    return res[NSTEPS]


_NAMELIST_REFS: dict = {}


@pytest.mark.parametrize("name,value,family", NAMELIST_RUNS, ids=[f"{n}={v}-{f}" for n, v, f in NAMELIST_RUNS])
def test_namelist_scalar_matches_reference(name, value, family, smooth_default_ref):
    """One namelist scalar off its default on the smooth moist case: the reference trajectory moves
    (so the option is consumed), and the GPU follows it to 1e-11 per field and per species."""
    case = _smooth_case(**{name: value})
    if (name, value) not in _NAMELIST_REFS:
        res, _ = _need_ref().run_reference(case, nsteps=NSTEPS, dt=DT, dump_steps=[NSTEPS], nthreads=4, moist_end=3)
        _NAMELIST_REFS[name, value] = res[NSTEPS]
    ref = _NAMELIST_REFS[name, value]
    moved = rel_linf(ref["state.u.tl1"], smooth_default_ref["state.u.tl1"])
    assert moved > 1e-9, f"{name}={value}: the option did not change the reference trajectory ({moved:.2e})"
    got = _run(case, {} if family == "default" else {"MPAS_DYCORE_KERNELS": family}, moist_end=3)
    errs = _errors(got, ref)
    progress(f"namelist {name}={value} {family}: u moves by {moved:.1e}; {_fmt(errs)}")
    assert np.isfinite(list(errs.values())).all()
    bad = {k: v for k, v in errs.items() if not v <= BAR}
    assert not bad, f"{name}={value} ({family}): {bad} (all {errs})"
