"""Per-plane histograms, the joint (u, v) histogram and the quadrant sums of the export stage
(Solver.plane_histograms) against the NumPy reference (channel_gpu_amd.reference.pdfs), binned from the
solver's own physical_fields() and from the oracle's fields.

Two histograms of perturbed samples are compared by the number of adjacent-bin moves between them,
sum_k |cum_got(k) - cum_ref(k)|, which may not exceed A, the number of reference samples within delta of a
bin edge (a sample perturbed by less than delta moves by at most one bin); the joint histograms by
sum |J_got - J_ref| <= 2 (A_u + A_v).  A comparison is only made where A is at most 1 % of the samples."""
import json

import numpy as np
import pytest

from channel_gpu_amd.reference import pdfs as rp
from channel_gpu_amd.utils.config import default_config
from test_physfields_gpu import NAMES, _solver, _stepping_solver, _tol

pytestmark = pytest.mark.gpu

MID = list(range(6, 27))  # the planes of the 33-plane grids away from the walls, where v and omega_y vanish


def _ulp(precision):
    return 2.0 ** -52 if precision == "fp64" else 2.0 ** -23


def _hist(s, planes, centre=None, halfwidth=None, **kw):
    flat = lambda a: [] if a is None else [float(v) for v in np.asarray(a, float).reshape(-1)]  # noqa: E731
    return s.plane_histograms(planes, centre=flat(centre), halfwidth=flat(halfwidth), **kw)


def _check_marginals(h):
    nb, nj = h["nbins"], h["njoint"]
    assert np.array_equal(h["joint"].sum(axis=2), rp.rebin(h["hist"][0], nb, nj))
    assert np.array_equal(h["joint"].sum(axis=1), rp.rebin(h["hist"][1], nb, nj))


def _compare(h, fields, names, deltas, cap=0.01):
    """h: the solver's histograms of planes h["planes"]; fields[name] (np, NX, Nzp): the reference samples;
    deltas[name] (np,): the perturbation allowed for per plane.  Returns the reference."""
    nb, nj = h["nbins"], h["njoint"]
    hn = list(h["names"])
    nsamp = fields[names[0]][0].size
    assert (h["hist"].sum(axis=2) == nsamp).all() and (h["joint"].sum(axis=(1, 2)) == nsamp).all()
    A = {}
    worst = 0
    for n in names:
        f = hn.index(n)
        for i in range(len(h["planes"])):
            c, sc = h["centre"][f, i], nb / (2.0 * h["halfwidth"][f, i])
            ref = np.bincount(rp.bin_index(fields[n][i], c, sc, nb).ravel(), minlength=nb + 2)
            a = rp.near_edge_count(fields[n][i], c, sc, nb, deltas[n][i])
            A[n, i] = a
            assert a <= cap * nsamp, f"{n} plane {h['planes'][i]}: {a} of {nsamp} samples within delta of an edge"
            d = rp.moves(h["hist"][f, i], ref)
            worst = max(worst, d)
            assert d <= a, f"{n} plane {h['planes'][i]}: {d} bin moves, {a} allowed"
    print(f"1-D histograms of {names}: at most {worst} moves, allowance at most {max(A.values())} of {nsamp}")
    if "u" in names and "v" in names:
        ref = rp.histograms([fields["u"], fields["v"]], h["centre"][:2], h["halfwidth"][:2], nb, nj)
        for i in range(len(h["planes"])):
            d = int(np.abs(h["joint"][i].astype(np.int64) - ref["joint"][i].astype(np.int64)).sum())
            assert d <= 2 * (A["u", i] + A["v", i]), f"joint plane {h['planes'][i]}: {d}"
    return A


def _own(s, h, names, precision):
    """The solver's own fields of the same planes and 4 ulp of the storage precision x the plane's max |x|."""
    f = s.physical_fields(list(h["planes"]), names)
    deltas = {n: 4 * _ulp(precision) * np.abs(f[n]).max(axis=(1, 2)) for n in names}
    return f, deltas


# ---- 1. against the solver's own physical_fields() -------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_own_fields_all_six(native, precision):
    """32 x 33 x 17: several rows per wave."""
    s, _, _ = _solver(native, 32, 33, 17, precision)
    h = _hist(s, MID, nbins=32, njoint=16, span=4.0, vorticity=True)
    assert list(h["names"]) == NAMES and h["hist"].shape == (6, 21, 34) and h["joint"].shape == (21, 18, 18)
    assert h["hist"].dtype == np.uint64 and h["joint"].dtype == np.uint64
    f, deltas = _own(s, h, NAMES, precision)
    _compare(h, f, NAMES, deltas)
    _check_marginals(h)


def test_own_fields_radix3(native):
    """48 x 33 x 25: radix-3 rows; 48 rows per plane against the block's row count."""
    s, _, _ = _solver(native, 48, 33, 25, "fp32")
    h = _hist(s, MID, nbins=32, njoint=16, span=4.0)
    assert list(h["names"]) == ["u", "v", "w"]
    f, deltas = _own(s, h, ["u", "v", "w"], "fp32")
    _compare(h, f, ["u", "v", "w"], deltas)
    _check_marginals(h)


# ---- 2. against the oracle's fields -----------------------------------------------------------------
@pytest.mark.parametrize("NX,NZ,precision", [(32, 17, "fp64"), (32, 17, "fp32"), (48, 25, "fp32")])
def test_oracle_fields(native, NX, NZ, precision):
    s, ph, U = _solver(native, NX, 33, NZ, precision)
    six = NX == 32
    names = NAMES if six else NAMES[:3]
    h = _hist(s, MID, nbins=32, njoint=16, span=4.0, vorticity=six)
    tol = _tol(precision)
    fields = {n: ph[i][MID] for i, n in enumerate(NAMES) if n in names}
    deltas = {n: np.full(len(MID), tol * np.abs(ph[NAMES.index(n)]).max()) for n in names}
    _compare(h, fields, names, deltas)
    _check_marginals(h)
    # quadrants: u' = u - U(y)
    nsamp = fields["u"][0].size
    ref = rp.histograms([fields["u"], fields["v"]], h["centre"][:2], h["halfwidth"][:2], 32, 16, U=U[MID])["quad"]
    m = np.asarray(s.plane_moments())
    for i, y in enumerate(MID):
        S, Sr = h["quad"][:4, i], ref[:4, i]
        scale = np.abs(Sr).max()
        err = np.abs(S - Sr).max() / scale
        near = rp.near_axis_count(fields["u"][i] - U[y], fields["v"][i], deltas["u"][i], deltas["v"][i])
        dn = np.abs(np.rint(h["quad"][4:, i] * nsamp) - np.rint(ref[4:, i] * nsamp)).max()
        print(f"plane {y}: quadrant sums rel. error {err:.2e} (tol {tol:.0e}); counts differ by {dn:.0f}, {near} near an axis; "
              f"sum - <u'v> {abs(S.sum() - m[4, y]) / scale:.2e}")
        assert err <= tol
        assert dn <= near
        assert abs(h["quad"][4:, i].sum() - 1.0) < 1e-12
        assert abs(S.sum() - m[4, y]) <= tol * scale


# ---- 3. long rows -------------------------------------------------------------------------------------
@pytest.mark.parametrize("NZ", [513, 1025])
def test_long_rows(native, NZ):
    """Nzp = 1024 (one wave per row) and 2048 (two waves per row)."""
    s, _, _ = _solver(native, 16, 17, NZ, "fp32")
    h = _hist(s, [4, 8, 12], nbins=32, njoint=16, span=4.0, vorticity=True)
    f, deltas = _own(s, h, ["u", "wz"], "fp32")
    _compare(h, f, ["u", "wz"], deltas)
    _check_marginals(h)


# ---- 4. blocked layout ------------------------------------------------------------------------------
def test_blocked_layout(native):
    s, _, _ = _solver(native, 16, 385, 9, "fp32")
    assert s.spec_kzb() == 8
    for planes in ([191], [6, 7, 8, 9]):
        h = _hist(s, planes, nbins=32, njoint=16, span=4.0, vorticity=True)
        f, deltas = _own(s, h, ["u", "w", "wz"], "fp32")
        _compare(h, f, ["u", "w", "wz"], deltas)
        _check_marginals(h)


# ---- 5. combine mode --------------------------------------------------------------------------------
def test_combine_mode(native, monkeypatch):
    monkeypatch.setenv("CHANNEL_COMBINE", "1")
    s, _, _ = _solver(native, 32, 33, 17, "fp64")
    assert s.combine()
    h = _hist(s, MID, nbins=32, njoint=16, span=4.0, vorticity=True)
    f, deltas = _own(s, h, NAMES, "fp64")
    _compare(h, f, NAMES, deltas)
    _check_marginals(h)


# ---- 6. wall shear ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_wall_shear(native, precision):
    """omega_z and omega_x at the wall planes are the wall shear stresses over the viscosity."""
    s, _, _ = _solver(native, 32, 33, 17, precision)
    h = _hist(s, [0, 32], nbins=32, njoint=16, span=4.0, vorticity=True)
    f, deltas = _own(s, h, ["wx", "wz"], precision)
    _compare(h, f, ["wx", "wz"], deltas)
    assert (h["hist"].sum(axis=2) == 32 * 32).all()
    # the default centre of omega_z is -D1 U: the plane mean of the exported field
    mean = f["wz"].mean(axis=(1, 2))
    err = np.abs(h["centre"][5] - mean).max() / np.abs(f["wz"]).max()
    print(f"centre of wz against the plane mean: {err:.2e}")
    assert err < _tol(precision)
    assert (h["centre"][1:5] == 0).all() and (h["halfwidth"] > 0).all()


# ---- 7. explicit inputs -------------------------------------------------------------------------------
def test_explicit_centre_and_halfwidth(native):
    s, _, _ = _solver(native, 32, 33, 17, "fp32")
    planes = [8, 16, 25]
    f = s.physical_fields(planes, ["u", "v", "w"])
    centre = np.array([[0.9, 1.2, 1.0], [0.01, 0.0, -0.01], [0.0, 0.02, 0.0]])
    # u: a quarter of the plane's spread, so that samples leave the range on both sides
    spread = np.array([f[n].max(axis=(1, 2)) - f[n].min(axis=(1, 2)) for n in ("u", "v", "w")])
    halfwidth = np.array([0.25, 2.0, 2.0])[:, None] * spread
    h = _hist(s, planes, centre, halfwidth, nbins=64, njoint=8, span=3.0)
    assert np.array_equal(h["centre"], centre) and np.array_equal(h["halfwidth"], halfwidth)
    deltas = {n: 4 * _ulp("fp32") * np.abs(f[n]).max(axis=(1, 2)) for n in ("u", "v", "w")}
    _compare(h, f, ["u", "v", "w"], deltas)
    _check_marginals(h)
    for i in range(3):
        x = f["u"][i]
        under = np.count_nonzero(x < centre[0, i] - halfwidth[0, i])
        over = np.count_nonzero(x >= centre[0, i] + halfwidth[0, i])
        assert under + over > 0
        near = rp.near_edge_count(x, centre[0, i], 64 / (2 * halfwidth[0, i]), 64, deltas["u"][i])
        assert abs(int(h["hist"][0, i, 0]) - under) <= near and abs(int(h["hist"][0, i, -1]) - over) <= near
        assert h["joint"][i, 0].sum() == h["hist"][0, i, 0] and h["joint"][i, -1].sum() == h["hist"][0, i, -1]


# ---- 8. repeatability ---------------------------------------------------------------------------------
def test_two_calls_are_bitwise_equal(native):
    s, _, _ = _solver(native, 48, 33, 25, "fp32")
    a = _hist(s, list(range(33)), vorticity=True)
    b = _hist(s, list(range(33)), vorticity=True)
    assert a["hist"].shape == (6, 33, 130) and a["joint"].shape == (33, 66, 66)
    assert np.array_equal(a["hist"], b["hist"]) and np.array_equal(a["joint"], b["joint"])
    assert np.array_equal(a["centre"], b["centre"]) and np.array_equal(a["halfwidth"], b["halfwidth"])
    _check_marginals(a)


def test_histograms_do_not_disturb_the_run(native):
    a, _ = _stepping_solver(native)
    for _ in range(4):
        a.step(False)
    b, _ = _stepping_solver(native)
    for _ in range(2):
        b.step(False)
    _hist(b, list(range(33)), vorticity=True)
    for _ in range(2):
        b.step(False)
    assert a.graph_active() and b.graph_active()
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    La, Lb = a.log(), b.log()
    assert La.dt == Lb.dt and La.time == Lb.time


# ---- 9. files -----------------------------------------------------------------------------------------
def test_files(native, tmp_path):
    cfg = default_config(NX=32, NY=33, NZ=17, Re=1000.0, precision="fp32", ic="random", ic_amplitude=0.2,
                         stats_every=0, log_every=0, symmetry_every=0, path=str(tmp_path) + "/",
                         pdf_every=2, pdf_planes="4,16", pdf_bins=64, pdf_joint_bins=32, pdf_span=5.0, pdf_vorticity=1)
    s = native.Solver(cfg, 0, 1, 0, b"")
    s.init_ic()
    s.run(4, False)
    for step in (2, 4):
        a = np.load(tmp_path / f"PDF_{step:08d}.npy")
        j = np.load(tmp_path / f"JPDF_UV_{step:08d}.npy")
        q = np.load(tmp_path / f"QUAD_{step:08d}.npy")
        assert a.shape == (6, 2, 66) and a.dtype == np.dtype("<u8")
        assert j.shape == (2, 34, 34) and j.dtype == np.dtype("<u8")
        assert q.shape == (8, 2) and q.dtype == np.dtype("<f8")
        assert (a.sum(axis=2) == 32 * 32).all() and (j.sum(axis=(1, 2)) == 32 * 32).all()
    side = json.loads((tmp_path / "PDF_00000004.json").read_text())
    assert side["planes"] == [4, 16] and side["step"] == 4 and side["names"] == NAMES
    assert side["nbins"] == 64 and side["njoint"] == 32 and side["span"] == 5.0 and side["Re"] == 1000.0
    assert len(side["y"]) == 2 and side["time"] > 0
    centre, halfwidth = np.array(side["centre"]), np.array(side["halfwidth"])
    assert centre.shape == (6, 2) and halfwidth.shape == (6, 2) and (halfwidth > 0).all()
    now = _hist(s, [4, 16], centre, halfwidth, nbins=64, njoint=32, vorticity=True)
    assert np.array_equal(a, now["hist"]) and np.array_equal(j, now["joint"])
    assert np.abs(q - now["quad"]).max() <= 1e-12 * np.abs(q).max()


# ---- 10. refusals -------------------------------------------------------------------------------------
def test_refusals(native, monkeypatch):
    s, _, _ = _solver(native, 32, 33, 17, "fp32")
    with pytest.raises(RuntimeError, match="plane 33"):
        _hist(s, [33])
    with pytest.raises(RuntimeError, match="nbins"):
        _hist(s, [4], nbins=33)
    with pytest.raises(RuntimeError, match="njoint"):
        _hist(s, [4], nbins=32, njoint=12)
    with pytest.raises(RuntimeError, match="span"):
        _hist(s, [4], span=0.0)
    with pytest.raises(RuntimeError, match="halfwidth must be positive"):
        _hist(s, [4], np.zeros((3, 1)), np.array([[1.0], [0.0], [1.0]]))
    with pytest.raises(RuntimeError, match="shape"):
        _hist(s, [4, 5], np.zeros((3, 1)), np.ones((3, 1)))
    # a one-rank communicator (the P > 1 pipeline): the export is refused
    monkeypatch.setenv("CHANNEL_FORCE_COMM", "1")
    from channel_gpu_amd.models.channel import ChannelFlow

    c = ChannelFlow(NX=32, NY=33, NZ=17, Re=400.0, precision="fp32", ic="zero", stats_every=0, log_every=0,
                    symmetry_every=0)
    assert c.solver.comm_kind() != "none"
    with pytest.raises(RuntimeError, match="single-rank"):
        c.plane_histograms([4])


def test_channelflow_and_statistics(native):
    """The Python layers: the dict of ChannelFlow.plane_histograms and two frozen samples summed into PDFs."""
    from channel_gpu_amd.models.channel import ChannelFlow

    c = ChannelFlow(NX=32, NY=33, NZ=17, Re=1000.0, precision="fp32", ic="random", ic_amplitude=0.2, stats_every=2,
                    log_every=0, symmetry_every=0, dt_fixed=1e-3)
    c.initialize()
    st = c.sample_statistics(4, every=2, pdfs=True, pdf_planes=[4, 10, 22, 28], pdf_bins=32, pdf_span=4.0, pdf_vorticity=True)
    assert st.nh == 2
    h = c.plane_histograms([4, 28], nbins=32, njoint=32, span=4.0)
    assert h["edges"].shape == (33,) and h["edges"][0] == -1 and h["edges"][-1] == 1 and np.array_equal(h["y"], c.y[[4, 28]])
    p = st.pdfs()
    assert list(p["planes"]) == [4, 10] and p["pdf"]["wz"].shape == (2, 32) and p["jpdf_uv"].shape == (2, 32, 32)
    for n in NAMES:
        total = p["pdf"][n].sum(axis=1) * (2.0 / 32) + p["out_of_range"][n]
        assert np.abs(total - 1).max() < 1e-12
    assert np.abs(p["quadrant_fraction"].sum(axis=0) - 1).max() < 1e-12
