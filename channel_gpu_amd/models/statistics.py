"""Time-averaged turbulence statistics of the channel in wall units.

The reference only appends instantaneous profiles to text files (MEANPROFILE.dat every step,
URMS/VRMS/WRMS/RSTRSS.dat every 10 steps: meanUevol.c:489-560, statistics.cu:161-243) and leaves
averaging and wall scaling to the user.  This accumulator takes the same quantities the solver
reduces on the device — U(y), the plane mean squares <u'u'>, <v'v'>, <w'w'>, <u'v'> (Parseval
plane sums, all ranks reduced) and the wall friction velocities — and produces the standard
wall-unit profiles folded over the two channel halves: U+(y+), u'+, v'+, w'+ r.m.s., -<u'v'>+,
plus the scalar checks of a statistically steady Re_tau~180 channel (Re_tau, U+_c, the u'+ peak
and its y+).  Optionally it also averages the one-point central moments of the physical-space
export (``Solver.plane_moments``) into skewness and flatness profiles of u, v, w, and the
velocity-gradient sums (``Solver.gradient_sums``) and triple products (``Solver.transport_moments``)
into vorticity r.m.s. profiles and the budgets of k and of the Reynolds stresses, and the pressure
moments of the y-line Poisson solve (``Solver.pressure_moments``) into the pressure r.m.s., the
pressure-velocity correlations and the pressure-diffusion terms of those budgets, and the Parseval
sums of the spectral static pressure (``Solver.pressure_strain``) into the pressure-strain terms, with
which the uu, vv, ww and uv budgets close component by component.  The one-dimensional spectra at
every plane (``Solver.plane_spectra``) are averaged into wall-unit spectra, premultiplied spectra and
two-point correlations (``spectra``).  The per-plane histograms (``Solver.plane_histograms``) are summed
into PDFs, the joint PDF of (u', v) and the quadrant split of -u'v' (``pdfs``).  The spectral budget rows
(``Solver.spectral_budgets``) are averaged into the terms of the uu, vv, ww and uv budgets per (y, k)
(``spectral_budgets``).  The cross-spectra of every plane against a few reference planes
(``Solver.plane_cross_spectra``) are averaged into correlation maps around those planes, wall-normal
correlation coefficients and linear coherence spectra (``cross_correlations``).
"""
from __future__ import annotations

import json

import numpy as np


# rows of Solver.plane_moments()
MOMENT_ROWS = ("u", "uu", "vv", "ww", "uv", "uuu", "vvv", "www", "uuuu", "vvvv", "wwww")
# rows of Solver.gradient_sums() and Solver.transport_moments()
GRADIENT_ROWS = ("wxwx", "wywy", "wzwz", "guu", "gvv", "gww", "guv")
TRANSPORT_ROWS = ("uuv", "wwv", "uvv")
BUDGET_STRESSES = ("k", "uu", "vv", "ww", "uv")
BUDGET_TERMS = ("prod", "eps", "visc", "turb", "resid")
# rows of Solver.pressure_moments(): plane means of p'p', p'u', p'v, p'w
PRESSURE_ROWS = ("pp", "pu", "pv", "pw")
PRESSURE_TERMS = ("pdiff_k", "pdiff_vv", "pdiff_uv")
# rows of Solver.pressure_strain(): 2 <p' du'/dx>, 2 <p' dv/dy>, 2 <p' dw/dz>, <p' (du'/dy + dv/dx)>,
# <p'u'>, <p'v> and the retained-band part of <p'p'>
PSTRAIN_ROWS = ("ps_uu", "ps_vv", "ps_ww", "ps_uv", "pu", "pv", "pp_band")
PSTRAIN_TERMS = ("pstrain_uu", "pstrain_vv", "pstrain_ww", "pstrain_uv")
# rows of Solver.plane_spectra(): |u|^2, |v|^2, |w|^2, Re(u v*), |omega_x|^2, |omega_y|^2, |omega_z|^2,
# |p'|^2 per |kx| and per kz at every plane
SPECTRA_ROWS = ("uu", "vv", "ww", "uv", "wxwx", "wywy", "wzwz", "pp")
# rows of Solver.spectral_budgets() per |kx| and per kz at every plane (reference/spectral_budgets.py)
SBUDGET_ROWS = ("n_uu", "n_vv", "n_ww", "n_uv", "g_uu", "g_vv", "g_ww", "g_uv", "gs_uu", "gs_vv", "gs_ww", "gs_uv",
                "gu", "gv", "ps_uu", "ps_vv", "ps_ww", "ps_uv", "pu", "pv")
SBUDGET_STRESSES = ("uu", "vv", "ww", "uv")
SBUDGET_TERMS = ("production", "nonlinear", "pressure_strain", "pressure_diffusion", "viscous_diffusion", "dissipation",
                 "residual")


class TurbulenceStatistics:
    def __init__(self, y: np.ndarray, nu: float, stretch: float = 2.0):
        self.y = np.asarray(y, float)
        self.nu = float(nu)
        self.stretch = float(stretch)  # of the tanh grid (the budgets' compact D1, D2)
        self.reset()

    def reset(self):
        n = self.y.size
        self.n = 0
        self.U = np.zeros(n)
        self.ms = np.zeros((4, n))  # uu, vv, ww, uv
        self.tau = 0.0              # mean wall shear velocity squared (both walls)
        self.t0 = None
        self.t1 = None
        self.nm = 0
        self.mom = np.zeros((len(MOMENT_ROWS), n))
        self.nb = 0
        self.grad = np.zeros((len(GRADIENT_ROWS), n))
        self.triple = np.zeros((len(TRANSPORT_ROWS), n))
        self.vvv = np.zeros(n)
        self.npr = 0
        self.pres = np.zeros((len(PRESSURE_ROWS), n))
        self.nps = 0
        self.pstr = np.zeros((len(PSTRAIN_ROWS), n))
        self.nsp = 0
        self.ekx = self.ekz = self.kx = self.kz = None
        self.nxz = (0, 0)
        self.nsb = 0
        self.sb_kx = self.sb_kz = self.sb_ekx = self.sb_ekz = self.sb_k = None
        self.ncs = 0
        self.cs_kx = self.cs_kz = self.cs_ekx = self.cs_ekz = self.cs_k = self.cs_refs = self.cs_rows = None
        self.cs_nxz = (0, 0)
        self.nh = 0
        self.hist = self.joint = self.quad = None
        self.h_planes = self.h_names = self.h_centre = self.h_halfwidth = None

    def add_histograms(self, h: dict):
        """One sample of the per-plane histograms (the dict of ``ChannelFlow.plane_histograms``: planes,
        names, hist, joint, quad, centre, halfwidth).  The first sample's centre and half-width are
        frozen (``pdf_frozen``): counts only add on the same bins, so a later sample binned otherwise
        is refused."""
        hist, joint = np.asarray(h["hist"], np.uint64), np.asarray(h["joint"], np.uint64)
        quad = np.asarray(h["quad"], float)
        centre, halfwidth = np.asarray(h["centre"], float), np.asarray(h["halfwidth"], float)
        planes, names = [int(j) for j in h["planes"]], [str(s) for s in h["names"]]
        if hist.shape[:2] != (len(names), len(planes)) or joint.shape[0] != len(planes) or quad.shape != (8, len(planes)):
            raise ValueError(f"histograms of shape {hist.shape}, {joint.shape}, {quad.shape} for {len(names)} fields, {len(planes)} planes")
        if self.nh == 0:
            self.hist, self.joint, self.quad = np.zeros_like(hist), np.zeros_like(joint), np.zeros_like(quad)
            self.h_planes, self.h_names = planes, names
            self.h_centre, self.h_halfwidth = centre.copy(), halfwidth.copy()
        elif (planes != self.h_planes or names != self.h_names or hist.shape != self.hist.shape
              or joint.shape != self.joint.shape):
            raise ValueError("histograms of other planes, fields or bin counts than the first sample's")
        elif not (np.array_equal(centre, self.h_centre) and np.array_equal(halfwidth, self.h_halfwidth)):
            raise ValueError("histograms binned with another centre or halfwidth than the frozen ones of the first sample")
        self.hist += hist
        self.joint += joint
        self.quad += quad
        self.nh += 1

    def pdf_frozen(self):
        """(centre, halfwidth) of the first histogram sample, each (nhf, np), or None before it."""
        return None if self.nh == 0 else (self.h_centre, self.h_halfwidth)

    def pdfs(self) -> dict:
        """Summed histograms folded onto the lower half.  Two-dimensional, so kept out of ``profiles``:

          planes, y_plus        [h]       the lower-half plane of every row and its wall distance
          bin_centres[name]     [nb]      in units of the frozen half-width, from the frozen centre
          pdf[name]             [h, nb]   density in those units; integrates to 1 - out_of_range[name]
          out_of_range[name]    [h]       fraction of samples in the under- and overflow bins
          jpdf_uv               [h, nj, nj]  joint density of (u', v) in the same units (axes u, v)
          quadrant_fraction     [4, h]    share of samples in Q1 .. Q4
          quadrant_uv_plus      [4, h]    their contributions to <u'v>+ (the sum over the four is <u'v>+)

        A plane j and its mirror NY - 1 - j are folded when both were sampled, a single one stands
        alone.  The upper half is reflected (y -> -y): the bins of v, omega_x, omega_z and the v axis of
        the joint histogram are reversed, which is exact because the bins are symmetric about the
        centre, Q1 <-> Q4 and Q2 <-> Q3 are swapped and u'v changes sign."""
        if self.nh == 0 or self.n == 0:
            raise ValueError("no histogram samples")
        from ..reference.pdfs import ODD_FIELDS

        n = self.y.size
        ut, nu = self.utau(), self.nu
        pos = {j: i for i, j in enumerate(self.h_planes)}
        rows = sorted({min(j, n - 1 - j) for j in self.h_planes})
        nb, nj = self.hist.shape[2] - 2, self.joint.shape[1] - 2
        hist = np.zeros((len(self.h_names), len(rows), nb + 2))
        joint = np.zeros((len(rows), nj + 2, nj + 2))
        quad = np.zeros((8, len(rows)))
        swap = [3, 2, 1, 0]
        for r, j in enumerate(rows):
            parts = 0
            if j in pos:
                i = pos[j]
                hist[:, r] += self.hist[:, i]
                joint[r] += self.joint[i]
                quad[:, r] += self.quad[:, i]
                parts += 1
            if n - 1 - j != j and n - 1 - j in pos:
                i = pos[n - 1 - j]
                for f, name in enumerate(self.h_names):
                    hist[f, r] += self.hist[f, i][::-1] if name in ODD_FIELDS else self.hist[f, i]
                joint[r] += self.joint[i][:, ::-1]
                quad[:4, r] -= self.quad[swap, i]
                quad[4:, r] += self.quad[4:][swap, i]
                parts += 1
            quad[:, r] /= parts * self.nh
        out = {"planes": np.array(rows), "y_plus": (1.0 + self.y[rows]) * ut / nu, "pdf": {}, "bin_centres": {},
               "out_of_range": {}}
        for f, name in enumerate(self.h_names):
            tot = hist[f].sum(-1, keepdims=True)
            out["pdf"][name] = hist[f][:, 1:-1] / tot / (2.0 / nb)
            out["out_of_range"][name] = (hist[f][:, 0] + hist[f][:, -1]) / tot[:, 0]
            out["bin_centres"][name] = (np.arange(nb) + 0.5) * (2.0 / nb) - 1.0
        out["jpdf_uv"] = joint[:, 1:-1, 1:-1] / joint.sum((1, 2))[:, None, None] / (2.0 / nj) ** 2
        out["quadrant_fraction"] = quad[4:]
        out["quadrant_uv_plus"] = quad[:4] / ut ** 2
        return out

    def add_spectra(self, ekx, ekz, kx, kz, nx: int | None = None, nz: int | None = None):
        """One sample of the 1-D spectra at every plane (``Solver.plane_spectra``): ``ekx`` [8, NY, nkx]
        by |kx| and ``ekz`` [8, NY, nkz] by kz (``SPECTRA_ROWS``) with their wavenumbers in solver
        units.  ``nx``, ``nz``: the physical grid of the two-point correlations (default: twice the
        highest wavenumber index, the smallest grid that holds the bins)."""
        ekx, ekz = np.asarray(ekx, float), np.asarray(ekz, float)
        n = self.y.size
        if ekx.shape[:2] != (len(SPECTRA_ROWS), n) or ekz.shape[:2] != (len(SPECTRA_ROWS), n):
            raise ValueError(f"spectra of shape {ekx.shape}, {ekz.shape}: expected ({len(SPECTRA_ROWS)}, {n}, nk)")
        if self.nsp == 0:
            self.ekx, self.ekz = np.zeros_like(ekx), np.zeros_like(ekz)
            self.kx, self.kz = np.asarray(kx, float).copy(), np.asarray(kz, float).copy()
            self.nxz = (int(nx) if nx else 2 * (ekx.shape[2] - 1), int(nz) if nz else 2 * (ekz.shape[2] - 1))
        self.ekx += ekx
        self.ekz += ekz
        self.nsp += 1

    def spectra(self) -> dict:
        """Averaged 1-D spectra folded onto the lower half, in wall units.  The result is
        two-dimensional (y, k), so it is kept out of ``profiles``:

          y_plus                       [h]      from the nearest wall
          kx_plus, kz_plus             [nk]     k nu / u_tau
          lambda_x_plus, lambda_z_plus [nk]     2 pi / k+ (inf at k = 0)
          E_kx[row], E_kz[row]         [h, nk]  energy per wavenumber bin (the sum over k is the plane
                                                mean of the product): velocity rows in u_tau^2, vorticity
                                                rows in u_tau^4 / nu^2, pp in u_tau^4; uv is folded
                                                antisymmetrically like ``uvplus`` (but keeps its sign)
          premult_kx[row], premult_kz[row]      k Phi(k) with the density Phi = E / dk: (k / dk) E
          R_x[row], R_z[row]           [h, n/2 + 1]  two-point correlation coefficients of the
                                                auto-spectra rows at 0 .. n/2 grid intervals
          r_x_plus, r_z_plus           [n/2 + 1]  those separations"""
        if self.nsp == 0 or self.n == 0:
            raise ValueError("no spectra samples")
        from ..reference.spectra import AUTO_ROWS, correlations

        n = self.y.size
        ut, nu = self.utau(), self.nu
        h = (n + 1) // 2
        lo = np.arange(h)
        hi = n - 1 - lo
        unit = {"uu": ut ** 2, "vv": ut ** 2, "ww": ut ** 2, "uv": ut ** 2, "wxwx": ut ** 4 / nu ** 2,
                "wywy": ut ** 4 / nu ** 2, "wzwz": ut ** 4 / nu ** 2, "pp": ut ** 4}
        out = {"y_plus": (1.0 + self.y[lo]) * ut / nu, "E_kx": {}, "E_kz": {}, "premult_kx": {}, "premult_kz": {},
               "R_x": {}, "R_z": {}}
        for d, k, e, nn in (("x", self.kx, self.ekx / self.nsp, self.nxz[0]), ("z", self.kz, self.ekz / self.nsp, self.nxz[1])):
            out[f"k{d}_plus"] = k * nu / ut
            with np.errstate(divide="ignore"):
                out[f"lambda_{d}_plus"] = 2.0 * np.pi / out[f"k{d}_plus"]
            idx = k / k[1] if k.size > 1 else np.zeros_like(k)
            out[f"r_{d}_plus"] = np.arange(nn // 2 + 1) * (2.0 * np.pi / k[1] / nn if k.size > 1 else 0.0) * ut / nu
            for q, row in enumerate(SPECTRA_ROWS):
                a = 0.5 * (e[q][lo] + (-1.0 if row == "uv" else 1.0) * e[q][hi]) / unit[row]
                out[f"E_k{d}"][row] = a
                out[f"premult_k{d}"][row] = idx * a
                if row in AUTO_ROWS:
                    out[f"R_{d}"][row] = correlations(a, nn)
        return out

    def add_spectral_budgets(self, bkx, bkz, ekx, ekz, kx, kz):
        """One sample of the spectral budget rows (``Solver.spectral_budgets``): ``bkx`` [20, NY, nkx] by
        |kx| and ``bkz`` [20, NY, nkz] by kz (``SBUDGET_ROWS``), with the stress spectra uu, vv, ww, uv of
        the same state, ``ekx`` [4, NY, nkx] and ``ekz`` [4, NY, nkz] (rows 0..3 of
        ``Solver.plane_spectra``), and the wavenumbers in solver units."""
        n = self.y.size
        bkx, bkz, ekx, ekz = (np.asarray(a, float) for a in (bkx, bkz, ekx, ekz))
        if bkx.shape[:2] != (len(SBUDGET_ROWS), n) or bkz.shape[:2] != (len(SBUDGET_ROWS), n):
            raise ValueError(f"budget rows of shape {bkx.shape}, {bkz.shape}: expected ({len(SBUDGET_ROWS)}, {n}, nk)")
        if ekx.shape != (4, n, bkx.shape[2]) or ekz.shape != (4, n, bkz.shape[2]):
            raise ValueError(f"stress spectra of shape {ekx.shape}, {ekz.shape}: expected (4, {n}, nk) with the rows' nk")
        if self.nsb == 0:
            self.sb_kx, self.sb_kz = np.zeros_like(bkx), np.zeros_like(bkz)
            self.sb_ekx, self.sb_ekz = np.zeros_like(ekx), np.zeros_like(ekz)
            self.sb_k = (np.asarray(kx, float).copy(), np.asarray(kz, float).copy())
        self.sb_kx += bkx
        self.sb_kz += bkz
        self.sb_ekx += ekx
        self.sb_ekz += ekz
        self.nsb += 1

    def spectral_budgets(self) -> dict:
        """Averaged terms of the uu, vv, ww and uv budgets per (y, k), folded onto the lower half, in wall
        units (u_tau^4 / nu per wavenumber bin).  Two-dimensional, so kept out of ``profiles``:

          y_plus                              [h]      from the nearest wall
          kx_plus, kz_plus                    [nk]     k nu / u_tau
          lambda_x_plus, lambda_z_plus        [nk]     2 pi / k+ (inf at k = 0)
          terms_kx[stress][term], terms_kz..  [h, nk]  ``SBUDGET_TERMS`` of ``SBUDGET_STRESSES``
          premult_kx[stress][term], premult_kz..       (k / dk) times the term, as ``spectra`` does

        production -2 U' E_uv (uu), -U' E_vv (uv); nonlinear: turbulent transport plus inter-scale transfer;
        pressure_strain; pressure_diffusion -2 D1 pv (vv), -D1 pu (uv); viscous_diffusion nu D2 E;
        dissipation -2 nu g; residual: minus their sum, the unsteadiness of the finite average.  Summed over
        k the terms are those of ``budgets`` and ``pressure_terms``.  U is the average of ``add``; every term
        of uu, vv, ww is folded symmetrically and every term of uv antisymmetrically, like ``profiles``."""
        if self.nsb == 0 or self.n == 0:
            raise ValueError("no spectral budget samples")
        from ..reference.spectral_budgets import budget_terms

        ops = self._ops()
        n = self.y.size
        ut, nu = self.utau(), self.nu
        U = self.U / self.n
        h = (n + 1) // 2
        lo = np.arange(h)
        hi = n - 1 - lo
        sc = nu / ut ** 4
        out = {"y_plus": (1.0 + self.y[lo]) * ut / nu, "terms_kx": {}, "terms_kz": {}, "premult_kx": {}, "premult_kz": {}}
        for d, k, rows, e in (("x", self.sb_k[0], self.sb_kx / self.nsb, self.sb_ekx / self.nsb),
                              ("z", self.sb_k[1], self.sb_kz / self.nsb, self.sb_ekz / self.nsb)):
            out[f"k{d}_plus"] = k * nu / ut
            with np.errstate(divide="ignore"):
                out[f"lambda_{d}_plus"] = 2.0 * np.pi / out[f"k{d}_plus"]
            idx = k / k[1] if k.size > 1 else np.zeros_like(k)
            for s, terms in budget_terms(ops, nu, U, rows, e).items():
                terms["residual"] = -sum(terms.values())
                sign = -1.0 if s == "uv" else 1.0
                folded = {t: sc * 0.5 * (a[lo] + sign * a[hi]) for t, a in terms.items()}
                out[f"terms_k{d}"][s] = folded
                out[f"premult_k{d}"][s] = {t: idx * a for t, a in folded.items()}
        return out

    def add_cross_spectra(self, ckx, ckz, ref_planes, rows, ekx, ekz, kx, kz, nx: int | None = None, nz: int | None = None):
        """One sample of the cross-spectra against reference planes (``Solver.plane_cross_spectra``):
        ``ckx`` [4, nref, NY, nkx] and ``ckz`` [4, nref, NY, nkz], complex, of the planes ``ref_planes`` and
        the row names ``rows``, with the spectra of the same state for the normalisation, ``ekx``
        [8, NY, nkx] and ``ekz`` [8, NY, nkz] (``Solver.plane_spectra``), and the wavenumbers in solver
        units.  ``nx``, ``nz``: the physical grid of the correlation maps (default: twice the highest
        wavenumber index).  Every sample has the planes and rows of the first."""
        ckx, ckz = np.asarray(ckx, complex), np.asarray(ckz, complex)
        ekx, ekz = np.asarray(ekx, float), np.asarray(ekz, float)
        refs, rows = [int(j) for j in ref_planes], [str(r) for r in rows]
        n = self.y.size
        if ckx.shape[:3] != (4, len(refs), n) or ckz.shape[:3] != (4, len(refs), n) or len(rows) != 4:
            raise ValueError(f"cross-spectra of shape {ckx.shape}, {ckz.shape}: expected (4, {len(refs)}, {n}, nk)")
        if ekx.shape != (len(SPECTRA_ROWS), n, ckx.shape[3]) or ekz.shape != (len(SPECTRA_ROWS), n, ckz.shape[3]):
            raise ValueError(f"spectra of shape {ekx.shape}, {ekz.shape}: expected ({len(SPECTRA_ROWS)}, {n}, nk) with the rows' nk")
        if self.ncs == 0:
            self.cs_kx, self.cs_kz = np.zeros_like(ckx), np.zeros_like(ckz)
            self.cs_ekx, self.cs_ekz = np.zeros_like(ekx), np.zeros_like(ekz)
            self.cs_refs, self.cs_rows = refs, rows
            self.cs_k = (np.asarray(kx, float).copy(), np.asarray(kz, float).copy())
            self.cs_nxz = (int(nx) if nx else 2 * (ckx.shape[3] - 1), int(nz) if nz else 2 * (ckz.shape[3] - 1))
        elif refs != self.cs_refs or rows != self.cs_rows or ckx.shape != self.cs_kx.shape or ckz.shape != self.cs_kz.shape:
            raise ValueError("cross-spectra of other reference planes, rows or sizes than the first sample's")
        self.cs_kx += ckx
        self.cs_kz += ckz
        self.cs_ekx += ekx
        self.cs_ekz += ekz
        self.ncs += 1

    def cross_correlations(self) -> dict:
        """Two-point correlations across planes from the averaged cross-spectra.  Three-dimensional, so
        kept out of ``profiles``:

          ref_planes, ref_y_plus         [nref']         the reference planes after folding and their wall distance
          y_plus                         [NY]            of every plane, from the reference plane's wall
          r_x_plus, r_z_plus             [NX], [NZp]     the signed separations -n/2 .. n/2 - 1 grid intervals
          R_x[row], R_z[row]             [nref', NY, n]  <a'(x + r, y) b'(x, y_r)> / sqrt(<a'a'>(y) <b'b'>(y_r))
          R_y[row]                       [nref', NY]     the same at zero separation
          coherence_kx[row], coherence_kz[row]  [nref', NY, nk]  |C|^2 / (E_a(y) E_b(y_r)) per wavenumber bin

        all 0 where the denominator is 0 (the walls).  A reference plane j and its mirror NY - 1 - j are
        folded when both were sampled, a single one stands alone, as in ``pdfs``.  The upper one is
        reflected (y -> NY - 1 - y); v, omega_x and omega_z are odd under the reflection, so the rows uv,
        u_wz and w_wx change sign.  The variances and spectra of the denominators are folded alike."""
        if self.ncs == 0 or self.n == 0:
            raise ValueError("no cross-spectra samples")
        from ..reference.cross_spectra import ODD_ROWS, ROW_FACTORS, cross_correlations

        n = self.y.size
        ut, nu = self.utau(), self.nu
        pos = {j: i for i, j in enumerate(self.cs_refs)}
        refs = sorted({min(j, n - 1 - j) for j in self.cs_refs})
        srow = {name: q for q, name in enumerate(SPECTRA_ROWS)}
        out = {"ref_planes": np.array(refs), "ref_y_plus": (1.0 + self.y[refs]) * ut / nu, "y_plus": (1.0 + self.y) * ut / nu,
               "R_x": {}, "R_z": {}, "R_y": {}, "coherence_kx": {}, "coherence_kz": {}}

        def ratio(a, d):
            ok = d > 0
            return np.where(ok, a / np.where(ok, d, 1.0), 0.0)

        for d, k, c, e, nn in (("x", self.cs_k[0], self.cs_kx / self.ncs, self.cs_ekx / self.ncs, self.cs_nxz[0]),
                               ("z", self.cs_k[1], self.cs_kz / self.ncs, self.cs_ekz / self.ncs, self.cs_nxz[1])):
            out[f"r_{d}_plus"] = (np.arange(nn) - nn // 2) * (2.0 * np.pi / k[1] / nn if k.size > 1 else 0.0) * ut / nu
            for q, row in enumerate(self.cs_rows):
                ea, eb = e[srow[ROW_FACTORS[row][0]]], e[srow[ROW_FACTORS[row][1]]]
                C = np.zeros((len(refs),) + c.shape[2:], complex)
                Ea = np.zeros((len(refs),) + ea.shape)
                Eb = np.zeros((len(refs), eb.shape[1]))
                for r, j in enumerate(refs):
                    parts = 0
                    if j in pos:
                        C[r] += c[q, pos[j]]
                        Ea[r] += ea
                        Eb[r] += eb[j]
                        parts += 1
                    if n - 1 - j != j and n - 1 - j in pos:
                        C[r] += (-1.0 if row in ODD_ROWS else 1.0) * c[q, pos[n - 1 - j]][::-1]
                        Ea[r] += ea[::-1]
                        Eb[r] += eb[n - 1 - j]
                        parts += 1
                    C[r] /= parts
                    Ea[r] /= parts
                    Eb[r] /= parts
                norm = np.sqrt(Ea.sum(-1) * Eb.sum(-1)[:, None])              # [nref', NY]
                out[f"R_{d}"][row] = ratio(cross_correlations(C, nn), norm[:, :, None])
                out[f"coherence_k{d}"][row] = ratio(np.abs(C) ** 2, Ea * Eb[:, None, :])
                if d == "x":
                    out["R_y"][row] = ratio(C.real.sum(-1), norm)
        return out

    def add_pressure_strain(self, ps):
        """One sample of the pressure-strain sums [7, NY] (``PSTRAIN_ROWS``)."""
        self.pstr += np.asarray(ps, float).reshape(len(PSTRAIN_ROWS), self.y.size)
        self.nps += 1

    def pressure_strain_terms(self) -> dict:
        """Unfolded pressure-strain terms over all NY points in solver units (``PSTRAIN_TERMS``):
        pstrain_uu = 2 <p' du'/dx>, pstrain_vv = 2 <p' dv/dy>, pstrain_ww = 2 <p' dw/dz> (their sum is
        zero: continuity) and pstrain_uv = <p' (du'/dy + dv/dx)>."""
        if self.nps == 0:
            raise ValueError("no pressure-strain samples")
        ps = self.pstr / self.nps
        return {name: ps[q] for q, name in enumerate(PSTRAIN_TERMS)}

    def add_pressure(self, pm):
        """One sample of the pressure moments [4, NY] (``PRESSURE_ROWS``: plane means of p'p', p'u',
        p'v, p'w of the fluctuating static pressure)."""
        self.pres += np.asarray(pm, float).reshape(len(PRESSURE_ROWS), self.y.size)
        self.npr += 1

    def _ops(self):
        from ..reference.oracle import build_ops

        ops = build_ops(self.y.size, self.stretch)
        if not np.allclose(ops.y, self.y, rtol=0, atol=1e-12):
            raise ValueError("the grid is not the tanh grid of this stretch: pass stretch= to TurbulenceStatistics")
        return ops

    def pressure_terms(self) -> dict:
        """Unfolded pressure-diffusion terms over all NY points in solver units (``PRESSURE_TERMS``):
        pdiff_k = -D1 <p'v>, pdiff_vv = 2 pdiff_k, pdiff_uv = -D1 <p'u'> (the uu and ww budgets have
        none).  The pressure-strain terms are those of ``pressure_strain_terms``; their trace is zero,
        so ``closure_k = resid_k - pdiff_k`` is what is left of the k budget, and per component
        ``closure_s = resid_s - pdiff_s - pstrain_s``: the unsteadiness of the finite average."""
        if self.npr == 0:
            raise ValueError("no pressure samples")
        ops = self._ops()
        pm = self.pres / self.npr
        pk = -(ops.D1 @ pm[2])
        return {"pdiff_k": pk, "pdiff_vv": 2.0 * pk, "pdiff_uv": -(ops.D1 @ pm[1])}

    def add_budgets(self, grad, triple, vvv):
        """One sample of the velocity-gradient sums [7, NY] (``GRADIENT_ROWS``), the triple products
        [3, NY] (``TRANSPORT_ROWS``) and <v^3> [NY] (row 6 of the plane moments).  The budgets are
        formed from the averages, together with U and the second moments of ``add``."""
        n = self.y.size
        self.grad += np.asarray(grad, float).reshape(len(GRADIENT_ROWS), n)
        self.triple += np.asarray(triple, float).reshape(len(TRANSPORT_ROWS), n)
        self.vvv += np.asarray(vvv, float).reshape(n)
        self.nb += 1

    def budgets(self) -> dict:
        """Unfolded budget terms over all NY points in solver units: ``{term_stress: ndarray (NY,)}``
        for the terms prod, eps, visc, turb, resid of k = (uu + vv + ww) / 2, uu, vv, ww, uv:

          prod   P_k = -<u'v> U', P_uu = -2 <u'v> U', P_uv = -<vv> U', P_vv = P_ww = 0
          eps    nu (g_uu + g_vv + g_ww) for k; 2 nu g for uu, vv, ww, uv
          visc   nu D2 <.>
          turb   -D1 of (uuv + vvv + wwv) / 2, uuv, vvv, wwv, uvv
          resid  -(prod - eps + visc + turb)

        ``resid`` is what closes the balance: the pressure terms (pressure diffusion, see
        ``pressure_terms``, and pressure strain) plus the unsteadiness of the finite average.
        D1 and D2 are the dense compact operators of ``reference.oracle.build_ops``."""
        if self.n == 0 or self.nb == 0:
            raise ValueError("no budget samples")
        ops = self._ops()
        nu = self.nu
        U = self.U / self.n
        uu, vv, ww, uv = self.ms / self.n
        g = self.grad / self.nb
        uuv, wwv, uvv = self.triple / self.nb
        vvv = self.vvv / self.nb
        dU = ops.D1 @ U
        zero = np.zeros_like(U)
        stress = {"k": 0.5 * (uu + vv + ww), "uu": uu, "vv": vv, "ww": ww, "uv": uv}
        prod = {"k": -uv * dU, "uu": -2.0 * uv * dU, "vv": zero, "ww": zero, "uv": -vv * dU}
        eps = {"k": nu * (g[3] + g[4] + g[5]), "uu": 2 * nu * g[3], "vv": 2 * nu * g[4], "ww": 2 * nu * g[5],
               "uv": 2 * nu * g[6]}
        flux = {"k": 0.5 * (uuv + vvv + wwv), "uu": uuv, "vv": vvv, "ww": wwv, "uv": uvv}
        out = {}
        for s in BUDGET_STRESSES:
            out["prod_" + s] = prod[s]
            out["eps_" + s] = eps[s]
            out["visc_" + s] = nu * (ops.D2 @ stress[s])
            out["turb_" + s] = -(ops.D1 @ flux[s])
            out["resid_" + s] = -(prod[s] - eps[s] + out["visc_" + s] + out["turb_" + s])
        return out

    def add_moments(self, m):
        """One sample of the raw central moments [11, NY] (``MOMENT_ROWS``); the moments are
        averaged, the skewness and flatness ratios formed from the averages."""
        self.mom += np.asarray(m, float).reshape(len(MOMENT_ROWS), self.y.size)
        self.nm += 1

    def add(self, U, stats, utau_lo: float, utau_hi: float, t: float | None = None):
        """One sample: U(y) [NY], stats [4*NY] (uu, vv, ww, uv plane means), u_tau at both walls."""
        n = self.y.size
        st = np.asarray(stats, float).reshape(4, n)
        self.U += np.asarray(U, float)
        self.ms += st
        self.tau += 0.5 * (utau_lo ** 2 + utau_hi ** 2)
        self.n += 1
        if t is not None:
            self.t0 = t if self.t0 is None else self.t0
            self.t1 = t

    # ---- averaged results ------------------------------------------------------------------------
    def utau(self) -> float:
        return float(np.sqrt(self.tau / max(self.n, 1)))

    def profiles(self) -> dict:
        """Averaged profiles folded onto the lower half (y+ from the nearest wall)."""
        if self.n == 0:
            raise ValueError("no samples")
        n = self.y.size
        ut = self.utau()
        U = self.U / self.n
        ms = self.ms / self.n
        h = (n + 1) // 2  # lower half incl. the centre point for odd NY
        lo = np.arange(h)
        hi = n - 1 - lo  # mirror points
        fold = lambda a, s=1.0: 0.5 * (a[lo] + s * a[hi])  # noqa: E731
        yplus = (1.0 + self.y[lo]) * ut / self.nu
        out = {
            "y": self.y[lo],
            "yplus": yplus,
            "Uplus": fold(U) / ut,
            "urms": np.sqrt(np.maximum(fold(ms[0]), 0.0)) / ut,
            "vrms": np.sqrt(np.maximum(fold(ms[1]), 0.0)) / ut,
            "wrms": np.sqrt(np.maximum(fold(ms[2]), 0.0)) / ut,
            # <u'v'> is antisymmetric about the centreline
            "uvplus": -fold(ms[3], -1.0) / ut ** 2,
        }
        if self.nm:
            mom = self.mom / self.nm
            for q, (r2, r3, r4) in zip("uvw", ((1, 5, 8), (2, 6, 9), (3, 7, 10))):
                m2 = mom[r2]
                ok = m2 > 0  # (the walls: 0)
                d = np.where(ok, m2, 1.0)
                # v-skewness is antisymmetric about the centreline (v -> -v under the reflection)
                out["skew_" + q] = fold(np.where(ok, mom[r3] / d ** 1.5, 0.0), -1.0 if q == "v" else 1.0)
                out["flat_" + q] = fold(np.where(ok, mom[r4] / d ** 2, 0.0))
        if self.nb:
            g = self.grad / self.nb
            # vorticity r.m.s. in units of u_tau^2 / nu
            for q, name in enumerate(("wx_rms", "wy_rms", "wz_rms")):
                out[name] = np.sqrt(np.maximum(fold(g[q]), 0.0)) * self.nu / ut ** 2
            # budgets in units of u_tau^4 / nu; under the reflection y -> -y (v -> -v, d/dy -> -d/dy)
            # every term of the k, uu, vv, ww budgets is symmetric and every term of the uv budget
            # antisymmetric (folded like -<u'v'>: the lower half's orientation)
            sc = self.nu / ut ** 4
            for k, a in self.budgets().items():
                out[k] = sc * fold(a, -1.0 if k.endswith("_uv") else 1.0)
        if self.npr:
            pm = self.pres / self.npr
            # p' in units of u_tau^2, <p'u'> and <p'v> in u_tau^3; <p'v> is antisymmetric about the
            # centreline (v -> -v), and so is -D1 <p'u'> like every term of the uv budget
            out["p_rms"] = np.sqrt(np.maximum(fold(pm[0]), 0.0)) / ut ** 2
            out["pu"] = fold(pm[1]) / ut ** 3
            out["pv"] = fold(pm[2], -1.0) / ut ** 3
            sc = self.nu / ut ** 4
            for k, a in self.pressure_terms().items():
                out[k] = sc * fold(a, -1.0 if k.endswith("_uv") else 1.0)
            if self.nb:
                out["closure_k"] = out["resid_k"] - out["pdiff_k"]
        if self.nps:
            # pressure strain in units of u_tau^4 / nu, folded like the other terms of its budget
            sc = self.nu / ut ** 4
            for k, a in self.pressure_strain_terms().items():
                out[k] = sc * fold(a, -1.0 if k.endswith("_uv") else 1.0)
            if self.nb and self.npr:
                out["closure_uu"] = out["resid_uu"] - out["pstrain_uu"]
                out["closure_ww"] = out["resid_ww"] - out["pstrain_ww"]
                out["closure_vv"] = out["resid_vv"] - out["pdiff_vv"] - out["pstrain_vv"]
                out["closure_uv"] = out["resid_uv"] - out["pdiff_uv"] - out["pstrain_uv"]
        return out

    def summary(self) -> dict:
        p = self.profiles()
        ut = self.utau()
        U = self.U / self.n
        yb = self.y
        Ub = float(np.trapz(U, yb) / (yb[-1] - yb[0]))
        i = int(np.argmax(p["urms"]))
        return {
            "samples": self.n,
            "t_start": self.t0,
            "t_end": self.t1,
            "utau": ut,
            "Re_tau": ut / self.nu,
            "Uc_plus": float(p["Uplus"][-1]),
            "Ub_plus": Ub / ut,
            "Cf": 2.0 * ut ** 2 / Ub ** 2,
            "urms_peak": float(p["urms"][i]),
            "urms_peak_yplus": float(p["yplus"][i]),
            "vrms_max": float(p["vrms"].max()),
            "wrms_max": float(p["wrms"].max()),
            "uv_max": float(p["uvplus"].max()),
        }

    def write(self, path: str):
        """Profiles as whitespace columns (y, y+, U+, u'+, v'+, w'+, -u'v'+) with a JSON summary header."""
        p = self.profiles()
        cols = [p["y"], p["yplus"], p["Uplus"], p["urms"], p["vrms"], p["wrms"], p["uvplus"]]
        names = "y yplus Uplus urms_plus vrms_plus wrms_plus minus_uv_plus"
        if self.nm:
            extra = ["skew_u", "skew_v", "skew_w", "flat_u", "flat_v", "flat_w"]
            cols += [p[k] for k in extra]
            names += " " + " ".join(extra)
        if self.nb:
            extra = ["wx_rms", "wy_rms", "wz_rms"] + [f"{t}_{s}" for s in BUDGET_STRESSES for t in BUDGET_TERMS]
            cols += [p[k] for k in extra]
            names += " " + " ".join(extra)
        if self.npr:
            extra = ["p_rms", "pu", "pv"] + list(PRESSURE_TERMS) + (["closure_k"] if self.nb else [])
            cols += [p[k] for k in extra]
            names += " " + " ".join(extra)
        if self.nps:
            extra = list(PSTRAIN_TERMS)
            if self.nb and self.npr:
                extra += ["closure_uu", "closure_vv", "closure_ww", "closure_uv"]
            cols += [p[k] for k in extra]
            names += " " + " ".join(extra)
        cols = np.column_stack(cols)
        with open(path, "w") as f:
            f.write("# " + json.dumps(self.summary()) + "\n")
            f.write("# " + names + "\n")
            np.savetxt(f, cols, fmt="%.6e")
