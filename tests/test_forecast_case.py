"""CPU: mpas_dycore.cases.forecast_case, the case of tests/test_gpu_forecast.py, on its own.

The GPU tests compare runs with each other; what they cover depends on the case populating every
boundary zone, on a 4-block split that puts specified cells in some blocks and none in others, on the
pair kernels' straddling sizes at K = 27, and on forcing that is non-zero in every zone.  These are
asserted here, without a GPU.
"""
import numpy as np
import pytest

import conftest

ZONE_COUNTS = {0: 479, 1: 40, 2: 34, 3: 30, 4: 26, 5: 18, 6: 12, 7: 3}   # x1.642, interior_deg = 120
HAND_PARTITION = (161, 322, 483)   # test_gpu_iau.py::test_iau_blocks_pair_across_the_owned_end
_MEMO = {}


def _forecast(K):
    from mpas_dycore.cases import forecast_case
    if K not in _MEMO:
        _MEMO[K] = forecast_case(K)
    return _MEMO[K]


def partition(case, K):
    """The 4-block split the GPU tests use at this K: the SFC split, or where that gives no block an
    odd nCellsSolve K and no block an odd nEdgesSolve K at an odd K, the IAU test's hand partition."""
    from mpas_dycore import decomp
    part = decomp.partition_sfc(case["nCells"], 4)
    if K % 2:
        blocks = decomp.decompose(case, part)
        if not (any((b.solve[0] * K) % 2 for b in blocks) and any((b.solve[1] * K) % 2 for b in blocks)):
            part = np.zeros(case["nCells"], dtype=np.int32)
            for i, c in enumerate(HAND_PARTITION):
                part[c:] = i + 1
    return part


@pytest.mark.parametrize("K", [26, 27, 80])
def test_forecast_case_covers_every_zone_and_splits(K):
    from mpas_dycore import decomp
    from mpas_dycore.cases import FORECAST_DT
    case, lbc, inc, phys = _forecast(K)
    assert case["nVertLevels"] == K and case["num_scalars"] == 3 and case["dt"] == FORECAST_DT == 600.0
    assert inc["window"] == 2.5 * case["dt"]
    mask = np.asarray(case["bdyMaskCell"])
    counts = {m: int((mask == m).sum()) for m in range(8)}
    assert counts == ZONE_COUNTS and min(counts.values()) > 0, counts
    spec = mask > 5
    near = np.asarray(case["nearestRelaxationCell"])
    assert np.all(near[spec] >= 0) and np.all(mask[near[spec]] == 5), "a specified cell lacks a relaxation cell"
    # the driving scalars were taken after the seeding: they hold cloud and rain
    assert lbc["lbc_scalars_s"][:, :, 1].max() > 0.0 and lbc["lbc_scalars_s"][:, :, 2].max() > 0.0
    part = partition(case, K)
    blocks = decomp.decompose(case, part)
    own_spec = []
    for b in blocks:
        n = b.solve[0]
        m = np.asarray(b.case["bdyMaskCell"])[:n]
        assert np.array_equal(m, mask[b.glob["cell"][:n]])
        loc = np.asarray(b.case["nearestRelaxationCell"])[:n][m > 5]
        assert np.all(loc >= 0) and np.all(loc < b.case["nCells"]), f"block {b.part}: nearest cell outside the block"
        assert np.array_equal(b.glob["cell"][loc], near[b.glob["cell"][:n]][m > 5])
        own_spec.append(int((m > 5).sum()))
    assert sum(own_spec) == int(spec.sum())
    assert sum(1 for s in own_spec if s > 0) >= 2 and sum(1 for s in own_spec if s == 0) >= 1, own_spec
    if K == 27:
        assert any((b.solve[0] * K) % 2 for b in blocks), [b.solve for b in blocks]
        assert any((b.solve[1] * K) % 2 for b in blocks), [b.solve for b in blocks]
    if np.array_equal(part, decomp.partition_sfc(case["nCells"], 4)):
        assert [b.solve[0] for b in blocks] == [161, 160, 161, 160]
        assert [b.solve[1] for b in blocks] == [538, 472, 487, 423]
    # forcing and increments act in the interior, the relaxation zone and the specified zone
    coe = np.asarray(case["cellsOnEdge"])
    emask = np.asarray(case["bdyMaskEdge"])
    assert np.array_equal(emask, np.minimum(mask[coe[:, 0]], mask[coe[:, 1]]))
    for zone, cz, ez in (("interior", mask == 0, emask == 0), ("relaxation", (mask > 0) & (mask <= 5),
                                                                 (emask > 0) & (emask <= 5)),
                         ("specified", spec, emask > 5)):
        assert cz.any() and ez.any(), zone
        for n in ("theta_amb", "rho_amb", "scalars_amb"):
            assert np.any(inc[n][cz] != 0.0), (zone, n)
        for s in range(3):
            assert np.any(inc["scalars_amb"][cz][:, :, s] != 0.0), (zone, s)
            assert np.any(phys["scalars_tend"][cz][:, :, s] != 0.0), (zone, s)
        assert np.any(inc["u_amb"][ez] != 0.0) and np.any(phys["tend_ru_physics"][ez] != 0.0), zone
        for n in ("tend_rtheta_physics", "tend_rho_physics"):
            assert np.any(phys[n][cz] != 0.0), (zone, n)


def test_forecast_case_is_built_from_the_suites_parts():
    """The pieces are the ones the single-hook tests use: the suite's physics forcing bit for bit, the
    seeded species of the Kessler tests, the IAU increments on the final case."""
    from mpas_dycore.cases import iau_increments, jw_case, physics_forcing, seed_cloud_and_rain
    case, lbc, inc, phys = _forecast(26)
    want = conftest.physics_forcing(case, scale=0.1)
    assert set(want) == set(phys)
    for n in want:
        assert np.array_equal(phys[n], want[n]), n
    for scale in (1.0, 0.1):
        a, b = physics_forcing(case, scale), conftest.physics_forcing(case, scale)
        assert all(np.array_equal(a[n], b[n]) for n in b)
    seeded = seed_cloud_and_rain(jw_case(642, 26, ns=3, moist=True, cache=False))
    assert np.array_equal(case["scalars"], seeded["scalars"])
    sc = np.asarray(seeded["scalars"]).reshape(case["nCells"], 26, 3)
    assert sc[:, :, 1].max() == 1.0e-3 and sc[:, :, 2].max() > 2.0e-3 and np.all(sc[1::10][:, :, 1:] == 0.0)
    for n, a in iau_increments(case).items():
        assert np.array_equal(inc[n], a), n
