"""The stress case (mpas_dycore.cases.stress_case) really loads the paths it is meant to load.

Asserted on the reference dycore alone (oracle/_ref), after 3 steps of 2880 s on x1.642 with
moist_end = ns: most of kdiff sits at the Smagorinsky cap 0.01 len_disp^2 / dt, the monotone
limiter changes the top-hat and noise species by more than 1e-6 of their own maxima in a large
share of entries, and the unlimited scheme undershoots zero, so the limiter and the final clip at
zero have real negatives to remove.  tests/test_gpu_stress.py compares the GPU with the
reference on this state; these conditions are what gives that comparison its teeth.
"""
import numpy as np
import pytest

DT = 2880.0
NSTEPS = 3
CASES = [(26, 3), (55, 3), (80, 3), (150, 3), (55, 6)]
UNLIMITED = dict(config_monotonic=False, config_positive_definite=False)


def limiter_share(lim, unl, s):
    """Share of species s's entries that the limiter moves by more than 1e-6 of the species' maximum."""
    a, b = lim[..., s], unl[..., s]
    return float(np.mean(np.abs(a - b) > 1e-6 * np.max(np.abs(a))))


@pytest.mark.parametrize("K,ns", CASES)
def test_stress_case_loads_limiter_and_cap(K, ns):
    from mpas_dycore.cases import stress_case
    from oracle import ref_runner
    if not ref_runner.available():
        pytest.skip("oracle/_ref not built")
    case = stress_case(K, ns)
    assert case["dt"] == DT and case["config"]["config_smagorinsky_coef"] == 1.0
    ini = np.asarray(case["scalars"]).reshape(case["nCells"], K, ns)
    assert np.count_nonzero(ini[..., 1]) > 0 and set(np.unique(ini[..., 1])) == {0.0, 1e-3}
    zeros = float(np.mean(ini[..., 2] == 0.0))
    assert 0.45 < zeros < 0.55 and ini[..., 2].min() == 0.0

    res, _ = ref_runner.run_reference(case, nsteps=NSTEPS, dt=DT, dump_steps=[NSTEPS], nthreads=4, moist_end=ns)
    lim = res[NSTEPS]
    for key, a in lim.items():
        if isinstance(a, np.ndarray):
            assert np.isfinite(a).all(), f"K={K} ns={ns}: {key} not finite"

    cfg = case["config"]
    cap = 0.01 * cfg["config_len_disp"] ** 2 / DT
    kd = lim["diag.kdiff"]
    assert kd.shape == (case["nCells"], K)
    at_cap = float(np.mean(kd >= cap * (1.0 - 1e-12)))
    assert kd.max() <= cap * (1.0 + 1e-12)
    assert 0.3 <= at_cap <= 0.9, f"K={K} ns={ns}: share of kdiff at the cap {at_cap:.3f}"

    ucase = stress_case(K, ns, **UNLIMITED)
    assert np.array_equal(ucase["scalars"], case["scalars"])
    ures, _ = ref_runner.run_reference(ucase, nsteps=NSTEPS, dt=DT, dump_steps=[NSTEPS], nthreads=4, moist_end=ns)
    sl, su = lim["state.scalars.tl1"], ures[NSTEPS]["state.scalars.tl1"]
    assert sl.shape == su.shape == (case["nCells"], K, ns)
    assert sl.min() >= 0.0  # the limited run stays non-negative
    hats, noises = ((1, 3), (2, 4)) if ns == 6 else ((1,), (2,))
    shares = {s: limiter_share(sl, su, s) for s in hats + noises}
    mins = {s: float(su[..., s].min()) for s in hats}
    print(f"K={K} ns={ns}: kdiff at cap {at_cap:.3f}, limiter shares {shares}, unlimited minima {mins}")
    for s in hats:
        assert shares[s] >= 0.10, f"K={K} ns={ns}: species {s} limiter share {shares[s]:.3f}"
        assert mins[s] < -1e-5 * (1.0 if s == 1 else 0.5), f"K={K} ns={ns}: species {s} unlimited minimum {mins[s]:.2e}"
    for s in noises:
        assert shares[s] >= 0.90, f"K={K} ns={ns}: species {s} limiter share {shares[s]:.3f}"
    if ns == 6:
        # a species that is identically zero stays exactly zero, limited or not
        assert not sl[..., 5].any() and not su[..., 5].any()
