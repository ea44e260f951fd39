"""The host restatement of the isobaric diagnostics (mpas_dycore.isobaric) against the compiled reference.

tests/golden/isobaric_columns.npz (tools/make_isobaric_golden.py) holds synthetic MPAS-level columns and what
the reference's own isobaric_diagnostics.F, compiled with the oracle's flags, computed from them.  The
restatement is the yardstick of the device kernel on states the fixture does not cover
(tests/test_gpu_isobaric.py), so it is pinned here:
* bit for bit on everything without a transcendental function, and, with the host C-library helper loaded
  (csrc/libmpas_host.so: same library, same order), on the rest too; without the helper the rest is
  bounded by 1e-13 relative, and the measured difference is printed;
* the fixture exercises what it must (every branch on at least 3 columns for every K, no column skipped)
  and keeps every comparison whose operand passed through log / exp / pow apart by a relative 1e-9;
* the per-column rule equals the loop transcription of interp_tofixed_pressure, with its kupper / kount
  bookkeeping, on the fixture's columns taken as one batch.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

from mpas_dycore import isobaric as iso  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "isobaric_columns.npz")
KS = (4, 26, 63, 64, 150)
SOFT_BOUND = 1e-13


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


_RUNS = {}


def _run(golden, tag):
    if tag not in _RUNS:
        c, ref = iso.fixture_columns(golden, tag)
        host = iso.cells(iso.fixture_cells(c))
        vert = iso.vertices(c["pressure_p_img"], c["pressure_base_img"], c["vorticity"], c["cellsOnVertex"],
                            c["kiteAreasOnVertex"], c["areaTriangle"])
        _RUNS[tag] = (c, ref, host, vert)
    return _RUNS[tag]


def _soft(name, info):
    """The values of an output that pass through log / exp / pow."""
    group = name.rsplit("_", 1)[0]
    if group == "dewpoint" or name == "mslp":
        return None                        # all of them
    if group in ("height", "w"):
        return info["iface"]["uses_top"][:, iso.HPA.index(int(name.rsplit("_", 1)[1][:-3]))]
    if name == "z_isobaric":
        return info["z_isobaric"]["uses_top"]
    return False


@pytest.mark.parametrize("tag", [f"K{K}" for K in KS] + ["fail"])
def test_restatement_against_compiled_reference(golden, tag):
    c, ref, host, vert = _run(golden, tag)
    assert set(ref) == set(iso.CELL_FIELDS + iso.VERTEX_FIELDS)
    worst = 0.0
    for name, r in ref.items():
        h = vert[name] if name in iso.VERTEX_FIELDS else host[name]
        assert h.shape == r.shape and np.all(np.isfinite(r)), name
        soft = _soft(name, host["info"])
        if soft is False or iso.host_libm_loaded():
            assert np.array_equal(h, r), f"{tag} {name}: not the reference's bits"
            continue
        m = np.ones(r.shape, dtype=bool) if soft is None else soft
        assert np.array_equal(h[~m], r[~m]), f"{tag} {name}: arithmetic-only values differ"
        if m.any():
            err = float(np.max(np.abs(h[m] - r[m])) / max(np.max(np.abs(r[m])), 1e-300))
            worst = max(worst, err)
            assert err <= SOFT_BOUND, f"{tag} {name}: rel Linf {err:.3e} > {SOFT_BOUND:g}"
    print(f"{tag}: host C library {'loaded: all bit for bit' if iso.host_libm_loaded() else f'not loaded: worst {worst:.3e}'}")
    if tag == "fail":
        assert host["info"]["slp"]["fail"].sum() == 3 and not ref["mslp"].any()
    else:
        assert ref["mslp"].min() > 5.0e4 and not host["info"]["slp"]["fail"].any()


@pytest.mark.parametrize("K", KS)
def test_fixture_coverage_and_margins(golden, K):
    import make_isobaric_golden as gen
    c, ref, host, vert = _run(golden, f"K{K}")
    n = c["theta_m"].shape[0]
    assert n >= 32 and c["vorticity"].shape[0] >= 32 and c["theta_m"].shape[1] == K
    cov = gen.coverage(host, vert)
    gen.check_coverage(cov, K)
    assert len(cov) == 19
    m = gen.margins(host)
    assert m.shape == (n,) and m.min() >= gen.MIN_MARGIN, m.min()          # every column, none excluded
    # the exact equalities hold no transcendental: they occur on the mass levels, whose pressure is
    # (pressure_p + pressure_base) / 100, on at least 3 columns each built from pressure_p = 0 and a
    # pressure_base exact in hPa; no target equals the top interface's pressure2(K + 1)
    info = host["info"]["mass"]
    exact = ~c["pressure_p"].any(axis=1) & ~(c["pressure_base"] % 100.0).any(axis=1)
    assert np.count_nonzero(exact & np.any(info["equal_lower"], axis=1)) >= 3
    assert np.count_nonzero(exact & np.any(info["branch"] == iso.EQUAL_TOP, axis=1)) >= 3
    for which in ("iface", "z_isobaric"):
        assert not np.any(host["info"][which]["branch"] == iso.EQUAL_TOP), which
    # strictly monotone columns, the only ones the per-column rule is guaranteed for
    p = iso.pressure(c["pressure_p"], c["pressure_base"])
    assert np.all(np.diff(p, axis=1) < 0) and np.all(np.diff(iso.pressure2(p, c["zgrid"]), axis=1) < 0)
    assert np.all(np.diff(vert["info"]["pressure_v"], axis=1) < 0)
    # the inputs are numbers float32 holds exactly
    for name in iso.FIXTURE_CELL_IN:
        assert golden[f"{name}_K{K}"].dtype == np.float32, name


def test_committed_file_is_small():
    assert os.path.getsize(GOLDEN) < (1 << 20)


@pytest.mark.parametrize("K", KS)
def test_per_column_rule_against_loop_transcription(golden, K):
    """interp() against interp_tofixed_pressure's own loops on the whole batch: mass levels in hPa and in
    Pa (t_isobaric), interfaces in hPa and in Pa (z_isobaric), and the vertices."""
    c, ref, host, vert = _run(golden, f"K{K}")
    p = iso.pressure(c["pressure_p"], c["pressure_base"])
    p2 = iso.pressure2(p, c["zgrid"])
    temperature = iso.thermo(p, c["theta_m"], c["qv"], c["exner"])[0]
    hpa = [float(x) for x in iso.HPA]
    for what, pres, field, targets in (("mass", p, c["uzonal"], hpa), ("t_isobaric", p * 100.0, temperature, list(iso.T_ISO_LEVELS)),
                                       ("iface", p2, c["w"], hpa), ("z_isobaric", p2 * 100.0, c["zgrid"], list(iso.Z_ISO_LEVELS)),
                                       ("vertex", vert["info"]["pressure_v"], c["vorticity"], hpa)):
        rule, _ = iso.interp(pres, field, targets)
        n = pres.shape[0]
        loops = iso.interp_reference_loops(pres[:, ::-1], field[:, ::-1], np.tile(np.array(targets), (n, 1)))
        assert np.array_equal(rule, loops), (K, what)
