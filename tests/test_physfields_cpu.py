"""Config keys of the physical-space export and the skewness / flatness profiles of
TurbulenceStatistics (no GPU)."""
import numpy as np
import pytest

from channel_gpu_amd import require_core
from channel_gpu_amd.models.statistics import MOMENT_ROWS, TurbulenceStatistics
from channel_gpu_amd.utils.config import default_config


def test_config_keys_defaults_and_round_trip():
    C = require_core()
    c = C.Config()
    assert (c.fields_every, c.fields_planes, c.fields, c.moments_every) == (0, "", "u,v,w", 0)
    c = default_config(NX=32, NY=33, NZ=17, fields_every=5, fields_planes="4, 16", fields="u,wz", moments_every=7)
    d = C.Config.from_string(c.to_string())
    assert (d.fields_every, d.fields_planes, d.fields, d.moments_every) == (5, "4, 16", "u,wz", 7)
    e = C.Config.from_string("NX = 32; NY = 33; NZ = 17; fields_every = 3; fields = \"v\"; moments_every = 2;"
                             " fields_planes = \"0,32\";")
    assert (e.fields_every, e.fields_planes, e.fields, e.moments_every) == (3, "0,32", "v", 2)


@pytest.mark.parametrize("bad", [dict(fields="u,q"), dict(fields_planes="40"), dict(fields_every=-1),
                                 dict(moments_every=-1), dict(fields="")])
def test_config_rejects(bad):
    with pytest.raises(RuntimeError):
        default_config(NX=32, NY=33, NZ=17, **bad)


def _stats(n=9):
    y = -np.cos(np.pi * np.arange(n) / (n - 1))
    st = TurbulenceStatistics(y, 1e-3)
    U = 1 - y ** 2
    ms = np.stack([0.5 + 0 * y, 0.2 + 0 * y, 0.3 + 0 * y, -0.1 * y])
    st.add(U, ms.ravel(), 0.05, 0.05, 1.0)
    return st, y


def test_profiles_without_moments_unchanged():
    st, _ = _stats()
    assert set(st.profiles()) == {"y", "yplus", "Uplus", "urms", "vrms", "wrms", "uvplus"}


def test_skewness_flatness_profiles(tmp_path):
    st, y = _stats()
    n = y.size
    m2 = np.stack([0.5 + 0.1 * y ** 2, 0.2 + 0 * y, 0.3 + 0.05 * y ** 2])
    m2[:, [0, -1]] = 0.0  # the walls
    m = np.zeros((len(MOMENT_ROWS), n))
    m[1:4] = m2
    m[8:11] = 3 * m2 ** 2  # Gaussian: flatness 3, skewness 0 for u and w
    sv = 0.4 * y           # an antisymmetric v skewness
    m[6] = sv * m2[1] ** 1.5
    # two samples whose average is m: the moments are averaged before the ratios are formed
    st.add_moments(0.5 * m)
    st.add_moments(1.5 * m)
    p = st.profiles()
    h = (n + 1) // 2
    inner = slice(1, h)
    for q in "uvw":
        assert p["flat_" + q].shape == (h,)
        assert np.allclose(p["flat_" + q][inner], 3.0)
        assert p["flat_" + q][0] == 0.0 and p["skew_" + q][0] == 0.0
    assert np.allclose(p["skew_u"], 0.0) and np.allclose(p["skew_w"], 0.0)
    # folded with -1: the lower half's values survive (a +1 fold would cancel them)
    assert np.allclose(p["skew_v"][inner], sv[:h][inner])
    out = tmp_path / "prof.dat"
    st.write(str(out))
    assert np.loadtxt(out).shape == (h, 13)
    assert "skew_u skew_v skew_w flat_u flat_v flat_w" in out.read_text().splitlines()[1]
