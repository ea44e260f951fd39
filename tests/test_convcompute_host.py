"""The host restatement of the output-time convective diagnostics (mpas_dycore.convcompute) against the
compiled reference.

tests/golden/convective_columns.npz (tools/make_convective_golden.py) holds synthetic MPAS-level columns and
what the reference's own convective_diagnostics.F (the loops of convective_diagnostics_compute and getcape,
compiled with the oracle's flags) computed from them.  The restatement is the yardstick of the device kernels
on states the fixture does not cover (tests/test_gpu_convcompute.py), so it is pinned here:
* bit for bit on all twelve written outputs of every set, cape and cin included: both sides call the C
  library's exp / log / pow in the same order;
* the fixture exercises what it must, and every column of it is stable: its discrete decisions (source
  level, iterations of every sub-step, branch of every level, how the ascent ended) do not move when every
  exp / log / pow result is shifted by +4 or -4 ulp;
* such a shift moves cape and cin by at most 1e-10 (rel Linf over a set) -- which is what makes the GPU
  tests' bound attainable for any library within that envelope;
* the synthetic soundings the GPU tests use have at most 2 % borderline columns;
* the bounded-work deviation: a column whose pressure goes up and down ends by the sub-step cap.
"""
import os
import sys

import numpy as np
import pytest

from conftest import rel_linf

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

from mpas_dycore import convcompute as cc  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convective_columns.npz")
KS = (4, 26, 64, 150)
SHIFT_BOUND = 1e-10
NSOLVE = 130                # the owned cells of the GPU tests


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


_RUNS = {}


def _classified(golden, K):
    if K not in _RUNS:
        cols, ref = cc.fixture_columns(golden, f"K{K}")
        _RUNS[K] = (cols, ref) + cc.classify(cols)
    return _RUNS[K]


@pytest.mark.parametrize("K", KS)
def test_restatement_has_the_reference_bits(golden, K):
    cols, ref, host, _, _ = _classified(golden, K)
    assert cols["theta_m"].shape == (40, K) and cols["zgrid"].shape == (40, K + 1)
    for name in cc.WRITTEN:
        assert np.array_equal(host[name], ref[name]), \
            f"K={K} {name}: rel Linf {rel_linf(host[name], ref[name]):.3e} (host libm helper loaded: {cc.host_libm_loaded()})"


def test_no_convergence_set(golden):
    """The columns the generator found that trip getcape's `i > 100` exit (extreme moisture): the reference
    returns cape and cin as accumulated so far, and so does the restatement, bit for bit."""
    cols, ref = cc.fixture_columns(golden, "noconv")
    host = cc.compute(cols)
    assert np.all(host["info"]["end"] == cc.END_NOCONV)
    assert host["info"]["iters"].max() == 101
    for name in cc.WRITTEN:
        assert np.array_equal(host[name], ref[name]), name


@pytest.mark.parametrize("K", KS)
def test_fixture_coverage(golden, K):
    from make_convective_golden import check_coverage, coverage
    cols, ref, host, _, _ = _classified(golden, K)
    cov = coverage(host, cols)
    print(f"K={K}: {cov}")
    check_coverage(cov, K)
    info = host["info"]
    # the items of the list, spelled out
    assert np.any((ref["cape"] > 100.0) & (ref["cin"] > 0.0)) and np.any(ref["cape"] == 0.0)
    assert np.any(info["kmax"] > 0) and np.any(info["p1"] < 50000.0)
    assert np.any(info["end"] == cc.END_100HPA) and np.any(info["end"] == cc.END_TOP)
    assert np.any(info["branch"] == cc.FIRST_POSITIVE) and np.any(info["branch"] == cc.FIRST_NEGATIVE)
    zp = info["zp"]
    assert np.any(zp[:, 0] > 1000.0) and np.any(zp[:, 0] <= 1000.0) and np.any(zp[:, -1] >= 6000.0)
    if K == 4:
        assert np.any(zp[:, -1] < 6000.0)           # the kz = min(kz, n - 1) clamp from above
    assert np.any(info["shear_raw"] < 1.0e-4) and np.any(info["srh_raw"] < 0.0)
    if K == 150:
        dp = (cols["pressure_p"] + cols["pressure_base"])
        dp = dp[:, :-1] - dp[:, 1:]
        assert np.any(np.any(dp < 100.0, axis=1) & np.any(dp > 1000.0, axis=1))     # nloop = 1 next to thick layers


@pytest.mark.parametrize("K", KS)
def test_fixture_columns_are_stable_and_the_shift_is_small(golden, K):
    _, _, host, stable, others = _classified(golden, K)
    assert stable.all(), f"K={K}: borderline fixture columns {np.flatnonzero(~stable)}"
    for ulp, o in zip((4, -4), others):
        for name in ("cape", "cin"):
            err = rel_linf(o[name], host[name])
            print(f"K={K} ulp {ulp:+d}: {name} rel Linf {err:.3e} (max |value| {np.max(np.abs(host[name])):.4g})")
            assert err <= SHIFT_BOUND, (K, ulp, name, err)


@pytest.mark.parametrize("K", KS)
def test_synthetic_fields_are_mostly_stable(K):
    from mpas_dycore.cases import jw_case
    case = jw_case(642, K=K, ns=3, moist=True, cache=False)
    f = cc.synthetic_fields(case, K)
    assert all(f[name].shape[0] == case["nCells"] for name in cc.INPUTS)
    again = cc.synthetic_fields(case, K)
    assert all(np.array_equal(f[name], again[name]) for name in cc.INPUTS)
    for name in cc.INPUTS:
        assert np.array_equal(f[name].astype(np.float32).astype(np.float64), f[name]), name
    base, stable, _ = cc.classify({name: f[name][:NSOLVE] for name in cc.INPUTS})
    borderline = int(np.count_nonzero(~stable))
    print(f"K={K}: {borderline} borderline of {NSOLVE}; cape > 100 J/kg on {np.count_nonzero(base['cape'] > 100.0)}, "
          f"sub-steps max {base['info']['nsub'].max()} mean {base['info']['nsub'].mean():.0f}, iterations per column mean "
          f"{base['info']['iters'].sum(axis=1).mean():.0f}")
    assert borderline <= 0.02 * NSOLVE
    if K >= 26:
        assert np.any(base["cape"] > 100.0)


def test_substep_cap():
    """A K = 26 column whose pressure alternates between 1000 and 10 hPa: 991 sub-steps for every second
    level, so the ascent ends by the cap of 8192 + K sub-steps, with finite cape and cin."""
    f = cc.alternating_column(26)
    host = cc.compute(f)
    info = host["info"]
    assert info["end"][0] == cc.END_CAP and info["nsub"][0] == cc.SUBSTEP_CAP + 26
    assert np.isfinite(host["cape"][0]) and np.isfinite(host["cin"][0]) and host["cape"][0] >= 0.0 and host["cin"][0] >= 0.0
    for name in cc.WRITTEN:
        assert np.all(np.isfinite(host[name])), name


def test_written_by_quirks():
    surface = {"uzonal_surface", "umeridional_surface", "temperature_surface", "dewpoint_surface"}
    assert cc.written_by(0) == ()
    for bit in (cc.LCL, cc.LFC, cc.UZONAL_SURFACE, cc.DEWPOINT_SURFACE):
        assert set(cc.written_by(bit)) == surface
    assert set(cc.written_by(cc.CAPE)) == set(cc.written_by(cc.CIN)) == surface | {"cape", "cin"}
    assert set(cc.written_by(cc.SRH_0_3KM)) == surface | {"srh_0_3km"}
    assert set(cc.written_by(cc.UMERIDIONAL_6KM)) == surface | {"umeridional_6km"}
    assert set(cc.written_by(cc.ALL)) == set(cc.WRITTEN)
