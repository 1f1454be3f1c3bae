"""High-level channel-flow DNS object (one per rank / GPU).

Wraps the C++ ``Solver`` (csrc/core/solver.cpp): state, RK3 stepping (one hipGraph per step),
reference-compatible logging/statistics files and HDF5 restarts, plus the time-averaged
turbulence statistics in wall units (``TurbulenceStatistics``).  Mirrors the reference driver
(main.c:10-150): config -> device -> setUp -> IC (random / file) -> RKstep -> writeData.

Bootstrap: inside an initialised torch.distributed job the torch control plane hands out the
RCCL id (``parallel.bootstrap``); otherwise the torch-free native TCP rendezvous does
(``parallel.native_bootstrap``), which is what the driver and bench.py use.
"""
from __future__ import annotations

import math
import sys

import numpy as np

from .._native import require_core
from ..utils.config import default_config, load_config
from .statistics import TurbulenceStatistics


def _torch_dist_initialized() -> bool:
    d = sys.modules.get("torch.distributed")
    return bool(d is not None and d.is_available() and d.is_initialized())


class ChannelFlow:
    def __init__(self, config=None, *, device: int | None = None, **overrides):
        C = require_core()
        if config is None:
            cfg = default_config(**overrides)
        elif isinstance(config, str):
            cfg = load_config(config, [f"{k}={v}" for k, v in overrides.items()])
        else:
            cfg = config
            for k, v in overrides.items():
                setattr(cfg, k, v)
            cfg.validate()
        if _torch_dist_initialized():
            import torch

            from ..parallel.bootstrap import dist_info, nccl_unique_id

            rank, world, local = dist_info()
            if device is None:
                device = local % max(1, torch.cuda.device_count())
            torch.cuda.set_device(device)
            uid = nccl_unique_id()
        else:
            from ..parallel.native_bootstrap import init_native

            ri = init_native()
            rank, world, uid = ri.rank, ri.world, ri.uid
            device = ri.device if device is None else device
        if C.device_count() < 1:
            raise RuntimeError("ChannelFlow needs an MI355X GPU; use channel_gpu_amd.reference for the CPU path")
        self.rank, self.world, self.device = rank, world, device
        self.solver = C.Solver(cfg, rank, world, device, uid)
        self.cfg = cfg
        self.statistics = TurbulenceStatistics(np.asarray(self.solver.grid.y), 1.0 / cfg.Re, cfg.stretch)

    # ---- setup -----------------------------------------------------------------------------
    @property
    def plan(self):
        return self.solver.plan

    @property
    def y(self) -> np.ndarray:
        return np.asarray(self.solver.grid.y)

    def initialize(self):
        c = self.cfg
        if c.ic == "file":
            self.solver.read_restart(c.in_G, c.in_DDV, c.in_UMEAN, c.in_T if c.scalar else "-")
        else:
            self.solver.init_ic()
        self.solver.prepare()
        return self

    def set_state(self, phi, omega, U):
        self.solver.set_state(np.asarray(phi, complex), np.asarray(omega, complex), np.asarray(U, float))
        self.solver.prepare()

    def get_state(self):
        return self.solver.get_state()

    # ---- passive scalar (``scalar = true``; one rank without a communicator) ----------------------
    def set_scalar(self, theta):
        """Set theta-hat, ``(NY, nkx, nkz)`` complex like the state; its mean line (kx, kz) = (0, 0) is the
        real mean profile Theta(y).  R_theta is cleared."""
        self.solver.set_scalar(np.asarray(theta, complex))

    def get_scalar(self) -> np.ndarray:
        return np.asarray(self.solver.get_scalar())

    def scalar_sums(self) -> np.ndarray:
        """``ndarray (5, NY)``: Theta, <theta'theta'>, <u'theta'>, <v theta'>, <w theta'> of the current
        state (Parseval plane sums over the retained modes, the weights of ``stats``)."""
        return np.asarray(self.solver.scalar_sums())

    # ---- stepping ---------------------------------------------------------------------------
    def step(self, n: int = 1):
        for _ in range(n):
            self.solver.step(False)

    def run(self, nsteps: int | None = None, verbose: bool = True):
        self.solver.run(self.cfg.nsteps if nsteps is None else nsteps, verbose)

    def synchronize(self):
        self.solver.synchronize()

    def log(self):
        return self.solver.log()

    # ---- output ------------------------------------------------------------------------------
    def save(self, g: str, ddv: str, umean: str = "-", t: str = "-"):
        """Write a restart; ``t``: also theta, in a file with the layout, units and attributes of ``g``."""
        self.solver.write_restart(g, ddv, umean, t)

    def load(self, g: str, ddv: str, umean: str = "-", regrid: bool = False, src_stretch: float | None = None,
             t: str = "-"):
        """Read a restart.  ``regrid`` (or the config key of that name): the files may be on another
        grid of the same box; modes map by index and every line is interpolated along y on the device
        (README "Restarting on another grid").  ``src_stretch``: the files' tanh stretching (default:
        the config's ``regrid_stretch``, else the files' ``stretch`` attribute, else the config's)."""
        if regrid or self.cfg.regrid:
            if t != "-":
                raise ValueError("load: regrid with t= is not supported (theta restarts on its own grid only)")
            s = self.cfg.regrid_stretch if src_stretch is None else float(src_stretch)
            self.solver.read_restart_regrid(g, ddv, umean, s)
        else:
            self.solver.read_restart(g, ddv, umean, t)
        self.solver.prepare()

    def regrid_from(self, phi, omega, U, *, NX: int, NY: int, NZ: int, stretch: float | None = None):
        """Take a global state on another grid of the same box, in the one-rank ``get_state`` layout
        ``(NY, nkx, nkz)`` of that grid: the array form of ``load(..., regrid=True)`` (every rank passes
        the whole source and picks its own lines).  ``stretch``: the source's (default: the config's)."""
        s = self.cfg.stretch if stretch is None else float(stretch)
        self.solver.regrid_state(np.asarray(phi, complex), np.asarray(omega, complex), np.asarray(U, float),
                                 int(NX), int(NY), int(NZ), s)
        self.solver.prepare()

    def mean_profile(self) -> np.ndarray:
        return np.asarray(self.solver.mean_profile())

    # ---- physical space (one rank) --------------------------------------------------------------
    def physical_fields(self, planes=None, fields=("u", "v", "w")) -> dict:
        """Physical-space planes of the current state: ``{name: ndarray (nplanes, NX, Nzp)}`` for
        ``fields`` out of u, v, w, wx, wy, wz, p at the y indices ``planes`` (default: every plane).
        The step keeps no physical field in memory; this runs the export stage on request.  ``p`` is
        the fluctuating static pressure p' (zero plane mean), which runs the pressure solve first."""
        if planes is None:
            planes = range(self.cfg.NY)
        return self.solver.physical_fields([int(j) for j in planes], [str(f) for f in fields])

    def plane_moments(self) -> np.ndarray:
        """Plane means of u', u'^2, v'^2, w'^2, u'v', u'^3, v'^3, w'^3, u'^4, v'^4, w'^4 with
        u' = u - U(y): ``ndarray (11, NY)`` (``statistics.MOMENT_ROWS``)."""
        return np.asarray(self.solver.plane_moments())

    def gradient_sums(self) -> np.ndarray:
        """Velocity-gradient plane sums of the current state, ``ndarray (7, NY)``
        (``statistics.GRADIENT_ROWS``): <|wx|^2>, <|wy|^2>, <|wz|^2> and g_uu, g_vv, g_ww, g_uv with
        g_ab = <grad a' . grad b'> -- raw sums, no nu and no factor 2.  Any number of ranks."""
        return np.asarray(self.solver.gradient_sums())

    def transport_moments(self) -> np.ndarray:
        """Plane means of u'u'v, wwv, u'vv (``statistics.TRANSPORT_ROWS``): ``ndarray (3, NY)``;
        one rank without a communicator, like ``plane_moments`` (which has <v^3> in row 6)."""
        return np.asarray(self.solver.transport_moments())

    def pressure_hat(self) -> np.ndarray:
        """Pi = p + |u|^2 / 2 of the current state per (kx, kz) line, ``ndarray (NY, nkx, nkz)`` complex:
        the y-line Poisson solve with the wall condition of the v-momentum equation; zero on the mean
        line.  One rank without a communicator; the run is not disturbed."""
        return np.asarray(self.solver.pressure_hat())

    def pressure_moments(self) -> np.ndarray:
        """Plane means of p'p', p'u', p'v, p'w of the fluctuating static pressure
        (``statistics.PRESSURE_ROWS``): ``ndarray (4, NY)``; one rank without a communicator."""
        return np.asarray(self.solver.pressure_moments())

    def static_pressure_hat(self) -> np.ndarray:
        """The fluctuating static pressure p' of the current state in spectral space, truncated to the
        retained modes: ``ndarray (NY, nkx, nkz)`` complex, zero on the mean line.  The pressure-mode
        export pass with the return trip of p' to spectral space; one rank without a communicator,
        the run is not disturbed."""
        return np.asarray(self.solver.static_pressure_hat())

    def pressure_strain(self) -> np.ndarray:
        """Parseval plane sums of p' with the strain factors (``statistics.PSTRAIN_ROWS``): the
        pressure-strain terms of the uu, vv, ww, uv budgets, <p'u'>, <p'v> and the retained-band part
        of <p'p'>: ``ndarray (7, NY)``; one rank without a communicator."""
        return np.asarray(self.solver.pressure_strain())

    def plane_spectra(self, pressure: bool = False) -> dict:
        """One-dimensional spectra and co-spectra of the current state at every plane
        (``statistics.SPECTRA_ROWS``: uu, vv, ww, uv, wxwx, wywy, wzwz, pp): ``ekx`` ``(8, NY, Kx + 1)``
        by |kx| (+kx and -kx folded, summed over kz) and ``ekz`` ``(8, NY, nkz)`` by kz (summed over
        kx), with the wavenumbers ``kx`` and ``kz``.  Summing either over its wavenumber gives the
        plane mean of the product.  Any number of ranks; ``pressure``: also row ``pp`` (one rank
        without a communicator; zero otherwise)."""
        d = dict(self.solver.plane_spectra(bool(pressure)))
        d["ekx"], d["ekz"] = np.asarray(d["ekx"]), np.asarray(d["ekz"])
        d["kx"] = 2.0 * np.pi / self.cfg.LX * np.arange(d["ekx"].shape[-1])
        d["kz"] = 2.0 * np.pi / self.cfg.LZ * np.arange(d["ekz"].shape[-1])
        return d

    def plane_cross_spectra(self, ref_planes, rows: str = "velocity") -> dict:
        """Cross-spectra of every plane of the current state against the reference planes ``ref_planes``
        (distinct y indices, at most 16) of the row set ``rows``: ``"velocity"`` (uu, vv, ww, uv) or
        ``"shear"`` (u_wz, v_wz, w_wx, wz_wz), the first factor at y and the conjugated second at the
        reference plane.  ``ckx`` ``(4, nref, NY, Kx + 1)`` by |kx| (conj(e) for kx < 0, summed over kz) and
        ``ckz`` ``(4, nref, NY, nkz)`` by kz (summed over kx), complex, with the wavenumbers ``kx`` and ``kz``
        and the grid ``y``; ``reference.cross_spectra`` has the definition and ``cross_correlations`` turns
        the bins into correlation maps.  Any number of ranks; the run is not disturbed."""
        d = dict(self.solver.plane_cross_spectra([int(j) for j in ref_planes], str(rows)))
        d["ckx"], d["ckz"] = np.asarray(d["ckx"]), np.asarray(d["ckz"])
        d["rows"], d["ref_planes"] = list(d["rows"]), list(d["ref_planes"])
        d["kx"] = 2.0 * np.pi / self.cfg.LX * np.arange(d["ckx"].shape[-1])
        d["kz"] = 2.0 * np.pi / self.cfg.LZ * np.arange(d["ckz"].shape[-1])
        d["y"] = np.asarray(self.y)
        return d

    def spectral_budgets(self) -> dict:
        """Spectral Reynolds-stress budget terms of the current state at every plane
        (``statistics.SBUDGET_ROWS``; ``reference.spectral_budgets`` has the equations): ``ekx``
        ``(20, NY, Kx + 1)`` by |kx| and ``ekz`` ``(20, NY, nkz)`` by kz with the conventions of
        ``plane_spectra``, the wavenumbers ``kx`` and ``kz``, and the mean profile ``U`` and its compact
        derivative ``dU`` as the rows used them.  One rank without a communicator; the run is not
        disturbed."""
        d = dict(self.solver.spectral_budgets())
        for k in ("ekx", "ekz", "U", "dU"):
            d[k] = np.asarray(d[k])
        d["rows"] = list(d["rows"])
        d["kx"] = 2.0 * np.pi / self.cfg.LX * np.arange(d["ekx"].shape[-1])
        d["kz"] = 2.0 * np.pi / self.cfg.LZ * np.arange(d["ekz"].shape[-1])
        return d

    def plane_histograms(self, planes=None, nbins: int = 128, njoint: int = 64, span: float = 8.0,
                         vorticity: bool = False, centre=None, halfwidth=None) -> dict:
        """Histograms of u, v, w (``vorticity``: and wx, wy, wz) of the current state at the distinct y
        indices ``planes`` (default: every plane), the joint histogram of (u, v) and the quadrant split
        of u'v, formed on the device by the export stage (``reference.pdfs`` has the binning rule):
        ``hist`` ``(nhf, np, nbins + 2)`` and ``joint`` ``(np, njoint + 2, njoint + 2)``, uint64 with
        the under- and overflow bins first and last; ``quad`` ``(8, np)``, the plane means of u'v over
        Q1 .. Q4 and the quadrants' sample fractions; ``centre`` and ``halfwidth`` ``(nhf, np)`` as used
        (given, or U(y) for u, -dU/dy for wz, 0 otherwise and ``span`` times the plane r.m.s. of the
        current state); ``names``, ``planes``, ``y`` and the bin ``edges`` in units of the half-width.
        One rank without a communicator; the run is not disturbed."""
        if planes is None:
            planes = range(self.cfg.NY)
        planes = [int(j) for j in planes]
        flat = lambda a: [] if a is None else [float(v) for v in np.asarray(a, float).reshape(-1)]  # noqa: E731
        nhf = 6 if vorticity else 3
        for a, what in ((centre, "centre"), (halfwidth, "halfwidth")):
            if a is not None and np.asarray(a).shape != (nhf, len(planes)):
                raise ValueError(f"{what} must have shape ({nhf}, {len(planes)})")
        d = dict(self.solver.plane_histograms(planes, int(nbins), int(njoint), float(span), bool(vorticity),
                                              flat(centre), flat(halfwidth)))
        for k in ("hist", "joint", "quad", "centre", "halfwidth"):
            d[k] = np.asarray(d[k])
        d["names"], d["planes"] = list(d["names"]), list(d["planes"])
        d["y"] = self.y[planes]
        d["edges"] = np.linspace(-1.0, 1.0, int(nbins) + 1)
        return d

    # ---- time-averaged statistics -------------------------------------------------------------
    def sample_statistics(self, nsteps: int, every: int = 10, moments: bool = False, budgets: bool = False,
                          pressure: bool = False, pressure_strain: bool = False, spectra: bool = False,
                          spectra_pressure: bool = False, pdfs: bool = False, pdf_planes=None, pdf_bins: int = 128,
                          pdf_span: float = 8.0, pdf_vorticity: bool = False, spectral_budgets: bool = False,
                          cross_spectra: bool = False, cross_planes=None, cross_rows: str = "velocity"):
        """Advance ``nsteps`` steps, sampling U(y), the plane r.m.s. and <u'v'> (the reference's
        calcSt cadence, statistics.cu:161-243) every ``every`` steps into ``self.statistics``;
        ``moments``: also the third and fourth central moments (skewness / flatness profiles);
        ``budgets``: also the velocity-gradient sums and the triple products (vorticity r.m.s. and
        the budgets of k and the Reynolds stresses; takes the plane moments too, for <v^3>);
        ``pressure``: also the pressure moments (p r.m.s., <p'u'>, <p'v>, pressure diffusion);
        ``pressure_strain``: also the pressure-strain terms (with ``budgets`` and ``pressure`` the
        per-component budgets then close: ``closure_uu``, ``closure_vv``, ``closure_ww``, ``closure_uv``);
        ``spectra``: also the 1-D spectra at every plane (``TurbulenceStatistics.spectra``; any number
        of ranks), with row ``pp`` when ``spectra_pressure`` (one rank);
        ``pdfs``: also the histograms at ``pdf_planes`` (default: every plane) with ``pdf_bins`` bins over
        ``pdf_span`` r.m.s. either side, with the vorticity when ``pdf_vorticity``
        (``TurbulenceStatistics.pdfs``; one rank).  The first sample's centres and half-widths bin every
        later sample.
        ``spectral_budgets``: also the spectral budget rows with the stress spectra they go with
        (``TurbulenceStatistics.spectral_budgets``; one rank).
        ``cross_spectra``: also the cross-spectra of every plane against the reference planes ``cross_planes``
        (required) of the row set ``cross_rows``, with the spectra of the same state for the normalisation
        (``TurbulenceStatistics.cross_correlations``; any number of ranks)."""
        if cross_spectra and not cross_planes:
            raise ValueError("cross_spectra needs cross_planes, the reference y indices")
        done = 0
        while done < nsteps:
            k = min(every, nsteps - done)
            for i in range(k):
                self.solver.step(i == k - 1)
            done += k
            if k == every:
                L = self.solver.log()
                self.statistics.add(np.asarray(self.solver.mean_profile()), np.asarray(self.solver.stats()), L.utau_lo,
                                    L.utau_hi, L.time)
                m = self.plane_moments() if (moments or budgets) else None
                if moments:
                    self.statistics.add_moments(m)
                if budgets:
                    self.statistics.add_budgets(self.gradient_sums(), self.transport_moments(), m[6])
                if pressure:
                    self.statistics.add_pressure(self.pressure_moments())
                if pressure_strain:
                    self.statistics.add_pressure_strain(self.pressure_strain())
                if spectra:
                    sp = self.plane_spectra(spectra_pressure)
                    self.statistics.add_spectra(sp["ekx"], sp["ekz"], sp["kx"], sp["kz"], self.cfg.NX, 2 * self.cfg.NZ - 2)
                if spectral_budgets:
                    sb, sp = self.spectral_budgets(), self.plane_spectra()
                    self.statistics.add_spectral_budgets(sb["ekx"], sb["ekz"], sp["ekx"][:4], sp["ekz"][:4], sb["kx"], sb["kz"])
                if cross_spectra:
                    cs, sp = self.plane_cross_spectra(cross_planes, cross_rows), self.plane_spectra()
                    self.statistics.add_cross_spectra(cs["ckx"], cs["ckz"], cs["ref_planes"], cs["rows"], sp["ekx"], sp["ekz"],
                                                      cs["kx"], cs["kz"], self.cfg.NX, 2 * self.cfg.NZ - 2)
                if pdfs:
                    c, hw = self.statistics.pdf_frozen() or (None, None)
                    self.statistics.add_histograms(self.plane_histograms(pdf_planes, pdf_bins, math.gcd(int(pdf_bins), 64),
                                                                         pdf_span, pdf_vorticity, c, hw))
        return self.statistics

    def grid_points(self) -> int:
        c = self.cfg
        return c.NX * c.NY * (2 * c.NZ - 2)
