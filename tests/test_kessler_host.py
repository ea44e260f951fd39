"""The host restatement of the Kessler microphysics (mpas_dycore.kessler) against the compiled reference.

tests/golden/kessler_columns.npz (tools/make_kessler_golden.py) holds 64 synthetic columns for each K in
{4, 26, 63, 64, 150} and what the reference's own module_mp_kessler.F, compiled with the oracle's
Fortran flags, made of them.  The restatement is the yardstick of the device kernel
(tests/test_gpu_kessler.py), so it is pinned here: the scheme against the compiled reference, the
interstitial against a loop transcription of the Fortran, and the fixture's branch coverage and nint
margins re-checked on the committed file.  No column is skipped anywhere.
"""
import math
import os

import numpy as np
import pytest

from mpas_dycore import kessler as ks

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kessler_columns.npz")
KS = (4, 26, 63, 64, 150)
OUT = ("t", "qv", "qc", "qr", "rainnc", "rainncv")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def host(golden):
    """kessler() on every K's columns, computed once."""
    out = {}
    for K in KS:
        cols, ref, dt = ks.fixture_columns(golden, K)
        out[K] = (ks.kessler(dt=dt, **{n: cols[n] for n in ("t", "qv", "qc", "qr", "rho", "pii", "z", "dz8w")}), ref)
    return out


def test_fixture_shape(golden):
    assert tuple(golden["K"]) == KS
    assert os.path.getsize(GOLDEN) < 1 << 20
    for K in KS:
        cols, ref, dt = ks.fixture_columns(golden, K)
        assert cols["t"].shape == (64, K) and cols["zgrid"].shape == (64, K + 1) and dt > 0.0
        assert all(ref[n].shape == (64, K) for n in OUT[:4]) and ref["rainnc"].shape == (64,)
        assert np.all(cols["dz8w"] > 0.0)


@pytest.mark.parametrize("K", KS)
def test_kessler_matches_compiled_reference(host, K):
    """Bit for bit: the same C library, the same operand order (measured when the fixture was made:
    rel Linf 0.0 on t, qv, qc, qr, rainnc, rainncv for every K; amdflang -O2 calls the scalar pow / exp)."""
    got, ref = host[K]
    for n in OUT:
        d = float(np.max(np.abs(got[n] - ref[n])))
        print(f"K={K} {n}: max abs diff {d:.3e}")
        assert np.array_equal(got[n], ref[n]), f"K={K} {n}: max abs diff {d:.3e}"
    # rain reached the ground somewhere, and the last split step's rainncv is not the whole of it
    assert ref["rainnc"].max() > 0.0 and np.any(ref["rainncv"] < ref["rainnc"])


@pytest.mark.parametrize("K", KS)
def test_fixture_exercises_the_branches(host, K):
    """What the generator asserts, on the committed file: every branch of the sweep on >= 5 % of the
    cell-levels, a re-split on >= 10 % of the columns, nfall from 1 to more than 8, and every nint
    margin >= 1e-6 (a last-bit difference in pow cannot change a column's nfall)."""
    info = host[K][0]["info"]
    for n in ("cond", "ern1", "ern2", "ern3", "exhaust"):
        assert info[n].shape == (64, K)
        assert np.mean(info[n]) >= 0.05, f"{n}: {np.mean(info[n]):.3f}"
    assert np.mean(info["resplit"]) >= 0.10
    assert info["nfall0"].min() == 1 and info["nfall0"].max() > 8
    assert len(info["margin"]) == 64
    assert min(m.min() for m in info["margin"]) >= 1.0e-6


def _mpas_columns(golden, K=4, ns=3):
    """An MPAS-level state whose microphysics_from_MPAS is (close to) the fixture's K = 4 columns."""
    cols, _, dt = ks.fixture_columns(golden, K)
    n = cols["t"].shape[0]
    rng = np.random.default_rng(7)
    zz = 0.9 + 0.1 * rng.random((n, K))
    scalars = np.zeros((n, K, ns))
    scalars[:, :, 0], scalars[:, :, 1], scalars[:, :, 2] = cols["qv"], cols["qc"], cols["qr"]
    scalars[::7, 0, 0] = -1.0e-6        # a negative qv: max(0, qv) in the theta conversion
    f = {"zz": zz, "rho_zz": cols["rho"] / zz, "exner": cols["pii"], "zgrid": cols["zgrid"], "scalars": scalars,
         "theta_m": cols["t"] * (1.0 + ks.R_V / ks.R_D * np.maximum(0.0, scalars[:, :, 0]))}
    f["rtheta_base"] = 0.97 * f["rho_zz"] * f["theta_m"]
    f["exner_base"] = 0.99 * cols["pii"]
    f["pressure_base"] = 1.0e5 * cols["pii"] ** (ks.CP / ks.R_D)
    f["rainnc"] = 3.0 * rng.random(n)
    f["i_rainnc"] = rng.integers(0, 3, n).astype(np.int32)
    f["surface_pressure"] = 1.0e5 + 100.0 * rng.random(n)
    return f, dt


def test_interstitial_matches_loop_transcription(golden):
    """from_mpas / precip_to_mpas / to_mpas against the Fortran's loops written out one cell and level at a
    time (mpas_atmphys_interface.F:541-559, 694-737; mpas_atmphys_driver_microphysics.F:533-559), K = 4,
    with the bucket on so that some cells move rain into i_rainnc."""
    f, dt = _mpas_columns(golden)
    n, K = f["theta_m"].shape
    bucket = 2.5
    a = ks.from_mpas(f["theta_m"], f["scalars"], f["rho_zz"], f["zz"], f["exner"], f["zgrid"])
    for i in range(n):
        for k in range(K):
            qv = f["scalars"][i, k, 0]
            assert a["rho"][i, k] == f["zz"][i, k] * f["rho_zz"][i, k]
            assert a["t"][i, k] == f["theta_m"][i, k] / (1.0 + ks.R_V / ks.R_D * max(0.0, qv))
            assert a["pii"][i, k] == f["exner"][i, k] and a["z"][i, k] == f["zgrid"][i, k]
            assert a["dz8w"][i, k] == f["zgrid"][i, k + 1] - f["zgrid"][i, k]
            assert (a["qv"][i, k], a["qc"][i, k], a["qr"][i, k]) == tuple(f["scalars"][i, k, :3])
    out = ks.driver(f, dt, bucket_rainnc=bucket)
    kz = ks.kessler(a["t"], a["qv"], a["qc"], a["qr"], a["rho"], a["pii"], a["z"], a["dz8w"], dt)
    moved = 0
    for i in range(n):
        precipw = 0.0
        for k in range(K):
            rho_a = a["rho"][i, k] / (1.0 + kz["qv"][i, k])
            precipw = precipw + kz["qv"][i, k] * rho_a * a["dz8w"][i, k]
        assert out["precipw"][i] == precipw
        assert out["rainncv"][i] == kz["rainnc"][i]
        rainnc, ir = f["rainnc"][i] + kz["rainnc"][i], f["i_rainnc"][i]
        if rainnc > bucket:
            ir, rainnc, moved = ir + 1, rainnc - bucket, moved + 1
        assert out["rainnc"][i] == rainnc and out["i_rainnc"][i] == ir
        for k in range(K):
            assert tuple(out["scalars"][i, k]) == (kz["qv"][i, k], kz["qc"][i, k], kz["qr"][i, k])
            tm = kz["t"][i, k] * (1. + ks.R_V / ks.R_D * kz["qv"][i, k])
            assert out["theta_m"][i, k] == tm
            assert out["rt_diabatic_tend"][i, k] == (tm - f["theta_m"][i, k]) / dt
            rtp = f["rho_zz"][i, k] * tm - f["rtheta_base"][i, k]
            assert out["rtheta_p"][i, k] == rtp
            ex = math.pow(f["zz"][i, k] * (ks.R_D / ks.P0) * (rtp + f["rtheta_base"][i, k]), ks.RCV)
            assert out["exner"][i, k] == ex
            assert out["pressure_p"][i, k] == f["zz"][i, k] * ks.R_D * (
                ex * rtp + (ex - f["exner_base"][i, k]) * f["rtheta_base"][i, k])
        zg = f["zgrid"][i]
        tem1, tem2 = zg[1] - zg[0], zg[2] - zg[1]
        rho1 = f["rho_zz"][i, 0] * f["zz"][i, 0] * (1. + kz["qv"][i, 0])
        rho2 = f["rho_zz"][i, 1] * f["zz"][i, 1] * (1. + kz["qv"][i, 1])
        sp = 0.5 * ks.GRAVITY * (zg[1] - zg[0]) * (rho1 - 0.5 * (rho2 - rho1) * tem1 / (tem1 + tem2))
        sp = sp + out["pressure_p"][i, 0] + f["pressure_base"][i, 0]
        assert out["surface_pressure"][i] == sp
        assert out["tend_sfc_pressure"][i] == (sp - f["surface_pressure"][i]) / dt
    assert 0 < moved < n
    # without the bucket nothing moves
    nb = ks.driver(f, dt)
    assert np.array_equal(nb["i_rainnc"], f["i_rainnc"]) and np.array_equal(nb["rainnc"], f["rainnc"] + kz["rainnc"])


def test_second_call_accumulates(golden):
    """rainnc accumulates over calls, rainncv is the call's own."""
    f, dt = _mpas_columns(golden)
    o1 = ks.driver(f, dt)
    g = dict(f, **{n: o1[n] for n in ("theta_m", "scalars", "exner", "rainnc", "i_rainnc", "surface_pressure")})
    o2 = ks.driver(g, dt)
    assert np.array_equal(o2["rainnc"], o1["rainnc"] + o2["rainncv"])
    assert not np.array_equal(o2["rainncv"], o1["rainncv"])
