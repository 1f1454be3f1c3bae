"""The NumPy reference of the per-plane histograms (channel_gpu_amd.reference.pdfs), the folding and
averaging of TurbulenceStatistics.add_histograms / pdfs, and the pdf_* config keys."""
import numpy as np
import pytest

from channel_gpu_amd.models.statistics import TurbulenceStatistics
from channel_gpu_amd.reference import pdfs as rp

NAMES = list(rp.HIST_NAMES)


def _fields(seed=3, npl=4, nx=24, nz=20, nhf=6):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((nhf, npl, nx, nz)) * np.linspace(0.5, 2.0, nhf)[:, None, None, None]
    f[0] += 1.0 + 0.3 * f[1]  # u about a mean, correlated with v
    return f


def _plane_stats(f):
    return f.mean(axis=(2, 3)), f.std(axis=(2, 3))


def test_totals_and_marginals():
    f = _fields()
    mean, rms = _plane_stats(f)
    for nb, nj in ((32, 16), (32, 32), (12, 4), (128, 64)):
        r = rp.histograms(list(f), mean, 2.5 * rms, nb, nj)
        assert r["hist"].shape == (6, 4, nb + 2) and r["joint"].shape == (4, nj + 2, nj + 2)
        assert r["hist"].dtype == np.uint64 and r["joint"].dtype == np.uint64
        assert (r["hist"].sum(axis=2) == 24 * 20).all() and (r["joint"].sum(axis=(1, 2)) == 24 * 20).all()
        assert r["hist"][:, :, 0].sum() > 0 and r["hist"][:, :, -1].sum() > 0  # 2.5 sigma: both tails leave the range
        assert np.array_equal(r["joint"].sum(axis=2), rp.rebin(r["hist"][0], nb, nj))
        assert np.array_equal(r["joint"].sum(axis=1), rp.rebin(r["hist"][1], nb, nj))


def test_bin_rule_edges():
    nb = 8
    c, hw = 0.5, 2.0
    sc = nb / (2 * hw)
    x = np.array([c, c - hw, c - hw - 1e-12, np.nextafter(c + hw, -np.inf), c + hw, 1e300, -1e300, np.nan,
                  c + 0.5 * hw, c - 1e-12])
    b = rp.bin_index(x, c, sc, nb)
    # the centre opens bin nb/2 + 1; the range is [c - h, c + h)
    assert list(b) == [nb // 2 + 1, 1, 0, nb, nb + 1, nb + 1, 0, 0, 3 * nb // 4 + 1, nb // 2]
    assert list(rp.joint_index(np.array([0, 1, 2, 3, 8, 9]), 8, 4)) == [0, 1, 1, 2, 4, 5]
    with pytest.raises(ValueError):
        rp.histograms([np.zeros((1, 4, 4))] * 3, np.zeros((3, 1)), np.ones((3, 1)), 7, 7)
    with pytest.raises(ValueError):
        rp.histograms([np.zeros((1, 4, 4))] * 3, np.zeros((3, 1)), np.ones((3, 1)), 8, 3)


def test_near_edge_count_and_moves():
    nb, c, sc = 4, 0.0, 2.0  # edges at -1, -0.5, 0, 0.5, 1
    x = np.array([-0.5 + 1e-7, 0.25, 0.5 - 1e-7, 0.9999999, 3.0, -0.2])
    assert rp.near_edge_count(x, c, sc, nb, 1e-6) == 3
    assert rp.near_edge_count(x, c, sc, nb, 1e-9) == 0
    # a perturbation below delta moves only near-edge samples, each by at most one bin
    rng = np.random.default_rng(5)
    x = rng.standard_normal(4000)
    y = x + rng.uniform(-1e-3, 1e-3, x.size)
    hx = np.bincount(rp.bin_index(x, 0.0, 16 / 6.0, 16), minlength=18)
    hy = np.bincount(rp.bin_index(y, 0.0, 16 / 6.0, 16), minlength=18)
    assert 0 < rp.moves(hy, hx) <= rp.near_edge_count(x, 0.0, 16 / 6.0, 16, 1e-3)
    assert rp.moves(hx, hx) == 0


def test_quadrants():
    f = _fields(nhf=3)
    mean, rms = _plane_stats(f)
    U = mean[0] + 0.01  # (not the bin centre: the quadrants have their own mean)
    q = rp.histograms(list(f), mean, 4 * rms, 32, 16, U=U)["quad"]
    du, v = f[0] - U[:, None, None], f[1]
    assert np.allclose(q[:4].sum(axis=0), (du * v).mean(axis=(1, 2)), rtol=0, atol=1e-14)
    assert np.allclose(q[4:].sum(axis=0), 1.0, rtol=0, atol=1e-14)
    assert (q[0] > 0).all() and (q[2] > 0).all() and (q[1] < 0).all() and (q[3] < 0).all()
    assert np.allclose(q[4], np.mean((du >= 0) & (v >= 0), axis=(1, 2)))
    assert list(rp.quadrant(np.array([1.0, -1.0, -1.0, 1.0, 0.0]), np.array([1.0, 1.0, -1.0, -1.0, 0.0]))) == [0, 1, 2, 3, 0]


def test_moments_from_the_histogram():
    """Mean and variance recomputed from a 128-bin, 8-sigma histogram agree with the direct ones to the bin width."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((1, 64, 64)) * 0.7 + 0.2
    mean, rms = x.mean(), x.std()
    nb = 128
    hw = 8 * rms
    h = rp.histograms([x, x, x], np.full((3, 1), mean), np.full((3, 1), hw), nb, 64)["hist"][0, 0]
    assert h[0] == 0 and h[-1] == 0
    width = 2 * hw / nb
    centres = mean + ((np.arange(nb) + 0.5) - nb / 2) * width
    p = h[1:-1] / h.sum()
    m1 = (p * centres).sum()
    m2 = np.sqrt((p * (centres - m1) ** 2).sum())
    assert abs(m1 - mean) < width and abs(m2 - rms) < width


def _sample(f, planes, centre, halfwidth, nb=16, nj=8):
    r = rp.histograms(list(f), centre, halfwidth, nb, nj)
    return {"planes": planes, "names": NAMES[:len(f)], "centre": centre, "halfwidth": halfwidth, **r}


def _stats(n=9):
    y = np.tanh(2.0 * (np.arange(n) * 2.0 / (n - 1) - 1.0)) / np.tanh(2.0)
    st = TurbulenceStatistics(y, 1e-3)
    st.add(np.zeros(n), np.zeros(4 * n), 0.05, 0.05, 0.0)
    return st


def test_statistics_fold_reverses_odd_fields():
    n = 9
    planes = [1, 3, 7, 4]  # 1 and 7 are mirrors; 3 stands alone; 4 is the centre plane
    # samples at k / 64 + 1 / 256: none on a bin edge (multiples of 3 / 8) or an axis, nor is its reflection
    f = np.round(_fields(seed=8, npl=4) * 64) / 64 + 1.0 / 256
    f[:, 2] = f[:, 0] * np.array([1, -1, 1, -1, 1, -1])[:, None, None]  # plane 7 = the reflection of plane 1
    centre, halfwidth = np.zeros((6, 4)), np.full((6, 4), 3.0)
    h = _sample(f, planes, centre, halfwidth, nb=16, nj=8)
    st = _stats(n)
    st.add_histograms(h)
    p = st.pdfs()
    assert list(p["planes"]) == [1, 3, 4]
    nb = 16
    for k, name in enumerate(NAMES):
        lo, hi = h["hist"][k, 0].astype(float), h["hist"][k, 2].astype(float)
        if name in rp.ODD_FIELDS:
            assert np.array_equal(hi, lo[::-1])  # the reflected plane's histogram is the reverse
        else:
            assert np.array_equal(hi, lo)
        # folded: twice the lower plane's counts, so the density is the lower plane's own
        assert np.allclose(p["pdf"][name][0], lo[1:-1] / lo.sum() / (2.0 / nb), rtol=0, atol=1e-15)
        assert np.allclose(p["pdf"][name][1], h["hist"][k, 1][1:-1] / 480.0 / (2.0 / nb), rtol=0, atol=1e-15)
        assert np.allclose(p["pdf"][name].sum(axis=1) * (2.0 / nb) + p["out_of_range"][name], 1.0, rtol=0, atol=1e-14)
        assert np.allclose(p["bin_centres"][name], (np.arange(nb) + 0.5) / 8 - 1)
    assert np.array_equal(h["joint"][2], h["joint"][0][:, ::-1])
    assert np.allclose(p["jpdf_uv"][0], h["joint"][0][1:-1, 1:-1] / 480.0 / (2.0 / 8) ** 2, rtol=0, atol=1e-13)
    # quadrants: Q1 <-> Q4, Q2 <-> Q3 and the sign of u'v under the reflection
    q = h["quad"]
    assert np.allclose(q[[3, 2, 1, 0], 2], -q[:4, 0], rtol=0, atol=1e-15) and np.allclose(q[4:][[3, 2, 1, 0], 2], q[4:, 0])
    assert np.allclose(p["quadrant_fraction"][:, 0], q[4:, 0]) and np.allclose(p["quadrant_uv_plus"][:, 0], q[:4, 0] / 0.05 ** 2)
    assert np.allclose(p["quadrant_fraction"].sum(axis=0), 1.0)
    assert p["y_plus"].shape == (3,) and (np.diff(p["y_plus"]) > 0).all()


def test_statistics_averages_and_freezes():
    f1, f2 = _fields(seed=1, npl=2), _fields(seed=2, npl=2)
    centre, halfwidth = np.zeros((6, 2)), np.full((6, 2), 4.0)
    st = _stats()
    with pytest.raises(ValueError, match="no histogram samples"):
        st.pdfs()
    assert st.pdf_frozen() is None
    a, b = _sample(f1, [2, 3], centre, halfwidth), _sample(f2, [2, 3], centre, halfwidth)
    st.add_histograms(a)
    st.add_histograms(b)
    assert st.nh == 2
    c, hw = st.pdf_frozen()
    assert np.array_equal(c, centre) and np.array_equal(hw, halfwidth)
    p = st.pdfs()
    tot = (a["hist"][1, 0] + b["hist"][1, 0]).astype(float)
    assert np.allclose(p["pdf"]["v"][0], tot[1:-1] / 960.0 / (2.0 / 16), rtol=0, atol=1e-15)
    assert np.allclose(p["quadrant_uv_plus"][:, 1] * 0.05 ** 2, 0.5 * (a["quad"][:4, 1] + b["quad"][:4, 1]))
    for key, other in (("centre", centre + 1e-9), ("halfwidth", halfwidth * (1 + 1e-12))):
        bad = dict(b)
        bad[key] = other
        with pytest.raises(ValueError, match="frozen"):
            st.add_histograms(bad)
    with pytest.raises(ValueError, match="other planes"):
        st.add_histograms(_sample(f2, [2, 4], centre, halfwidth))
    assert st.nh == 2


def test_config_keys(native):
    c = native.Config()
    assert (c.pdf_every, c.pdf_planes, c.pdf_bins, c.pdf_joint_bins, c.pdf_span, c.pdf_vorticity) == (0, "", 128, 64, 8.0, 0)
    text = 'application:\n{\n NX = 32; NY = 33; NZ = 17;\n pdf_every = 5; pdf_planes = "4, 16,28"; pdf_bins = 64;\n' \
           ' pdf_joint_bins = 16; pdf_span = 6.5; pdf_vorticity = 1;\n};\n'
    c = native.Config.from_string(text)
    assert (c.pdf_every, c.pdf_planes, c.pdf_bins, c.pdf_joint_bins, c.pdf_span, c.pdf_vorticity) == (5, "4, 16,28", 64, 16, 6.5, 1)
    c2 = native.Config.from_string(c.to_string())
    for k in ("pdf_every", "pdf_planes", "pdf_bins", "pdf_joint_bins", "pdf_span", "pdf_vorticity"):
        assert getattr(c2, k) == getattr(c, k), k
    for bad, what in (("pdf_every=-1", "cadences"), ("pdf_planes=\"4,33\"", "pdf_planes"), ("pdf_planes=\"4,x\"", "pdf_planes"),
                      ("pdf_bins=63", "pdf_bins"), ("pdf_bins=0", "pdf_bins"), ("pdf_bins=512", "pdf_bins"),
                      ("pdf_joint_bins=24", "pdf_joint_bins"), ("pdf_joint_bins=0", "pdf_joint_bins"),
                      ("pdf_span=0", "pdf_span"), ("pdf_span=-2.0", "pdf_span"), ("pdf_vorticity=2", "pdf_vorticity")):
        with pytest.raises(RuntimeError, match=what):
            native.Config.from_string(text, [bad])
