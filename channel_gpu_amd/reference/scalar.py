"""NumPy fp64 reference of the passive scalar transported with the flow (one rank, P = 1).

One scalar theta(x, y, z, t) obeys d(theta)/dt = -div(u theta) + kappa lap(theta) + source with Dirichlet
walls, kappa = 1 / (Re Pr): the omega_y equation of ``OracleSolver.substep`` with nu -> kappa and its own
right-hand side.  theta-hat is stored like phi and omega_y, [y][kx][kz] true Fourier coefficients of the
retained modes; its line (kx, kz) = (0, 0) holds the real mean profile Theta(y) itself.

Per substep n (dt the step's, alpha, beta, gamma, zeta the RK3 coefficients):

    F = (u theta, v theta, w theta)^        physical-space products of the stage state, 2/3-dealiased
    N = -(i al F_x + D1 F_y + i be F_z)     mean line: Re N + source
    R_n = M N
    r = M th + dt [alpha kappa (K th - k2 M th) + gamma R_n + zeta R_{n-1}]
    wall rows of r: 0 (mean line: lower, upper)
    th_new = solve((1 + beta dt kappa k2) M - beta dt kappa K with identity wall rows, r)

The order inside a substep is: scalar flux -> transforms -> momentum substep -> scalar substep; u, v, w are
those the momentum transform stage of the same substep reads.  The scalar never acts on the flow.
"""
from __future__ import annotations

import numpy as np

from . import oracle as ora


class ScalarOracle(ora.OracleSolver):
    def __init__(self, *args, Pr: float = 0.71, wall=(0.0, 0.0), source: float = 0.0, **kw):
        super().__init__(*args, **kw)
        if self.plan.P != 1:
            raise ValueError("ScalarOracle holds for P = 1 only")
        if not Pr > 0:
            raise ValueError("Pr must be positive")
        self.Pr, self.wall, self.source = float(Pr), (float(wall[0]), float(wall[1])), float(source)
        self.kappa = 1.0 / (self.Re * self.Pr)
        self.th = np.zeros(self.phi.shape, complex)
        self.Rth = np.zeros(self.phi.shape, complex)
        self.flux_on = True  # False drops the advective term (tests: the size of its effect)

    def set_scalar(self, th):
        self.th = np.array(th, complex).reshape(self.phi.shape)
        self.th[:, 0, 0] = self.th[:, 0, 0].real
        self.Rth[:] = 0

    def set_state(self, phi, om, U=None):
        super().set_state(phi, om, U)
        if hasattr(self, "Rth"):
            self.Rth[:] = 0

    def laminar_scalar(self) -> np.ndarray:
        """The steady conduction profile with the source: every other mode zero."""
        y = self.ops.y
        lo, up = self.wall
        th = np.zeros(self.phi.shape, complex)
        th[:, 0, 0] = lo + (up - lo) * 0.5 * (y + 1.0) + self.source * (1.0 - y * y) / (2.0 * self.kappa)
        return th

    # ---- the two stages of a substep ----------------------------------------------------------------
    def scalar_flux(self) -> np.ndarray:
        """[3, NY, nkx, nkz]: (u theta)^, (v theta)^, (w theta)^ of the prepared fields."""
        if self.fields is None:
            self.prepare()
        p = self.plan
        uvw = ora.spec_to_phys_full(self.fields[:3], p)
        th = ora.spec_to_phys_full(self.th, p)
        return ora.phys_to_spec_full(uvw * th[None], p)

    def scalar_substep(self, n: int, F: np.ndarray):
        ops, k2, al, be = self.ops, self.k2, self.al, self.be
        dt, kap = self.dt, self.kappa
        Fx, Fy, Fz = (self.lines(f) for f in F)
        N = -(1j * al * Fx + ops.D1 @ Fy + 1j * be * Fz)
        if not self.flux_on:
            N = np.zeros_like(N)
        m = self.mean_line
        N[:, m] = N[:, m].real + self.source
        Rn = ops.M @ N
        th = self.lines(self.th)
        Mth = ops.M @ th
        r = Mth + dt * (ora.ALPHA[n] * kap * (ops.K @ th - k2 * Mth) + ora.GAMMA[n] * Rn + ora.ZETA[n] * self.lines(self.Rth))
        r[0] = r[-1] = 0.0
        r[0, m], r[-1, m] = self.wall
        new = ora._bsolve(ora.impl_matrix(ops, k2, ora.BETA[n] * dt * kap), r)
        new[:, m] = new[:, m].real
        self.th = new.reshape(self.th.shape)
        self.Rth = Rn.reshape(self.th.shape)

    def step(self):
        if self.fields is None:
            self.prepare()
        for n in range(3):
            F = self.scalar_flux()
            self.transforms(compute_dt=(n == 0))
            self.substep(n)
            self.scalar_substep(n, F)


def scalar_sums(o: ScalarOracle) -> np.ndarray:
    """[5, NY]: Theta, <theta'theta'>, <u'theta'>, <v theta'>, <w theta'>: Parseval plane sums over the
    retained modes with the weights and the mean-line skip of ``OracleSolver.plane_stats``."""
    if o.fields is None:
        o.prepare()
    p = o.plan
    u, v, w = (o.lines(f) for f in o.fields[:3])
    th = o.lines(o.th)
    wgt = np.where(np.tile(p.kz0 + np.arange(p.nkz_loc), p.nkx_loc) == 0, 1.0, 2.0)
    wgt[o.mean_line] = 0
    dot = lambda a, b: (a.real * b.real + a.imag * b.imag) @ wgt  # noqa: E731
    return np.stack([th[:, o.mean_line].real, dot(th, th), dot(u, th), dot(v, th), dot(w, th)])


def random_scalar(plan: ora.OraclePlan, ops: ora.YOps, seed: int = 1, amp: float = 0.1, mean=None,
                  kscale: float = 32.0) -> np.ndarray:
    """Random theta-hat with a (1 - y^2) envelope, Hermitian at kz = 0; the mean line is ``mean`` (default 0)."""
    rng = np.random.default_rng(seed)
    N, y = ops.N, ops.y
    th = np.zeros((N, plan.nkx, plan.nkz), complex)
    for i in range(plan.nkx):
        kx = int(plan.kx_of(i))
        if kx < 0:
            continue
        for kz in range(plan.nkz):
            if kx == 0 and kz == 0:
                continue
            al, be = plan.ax * kx, plan.az * kz
            env = np.exp(-(al * al + be * be) / kscale)
            q = amp * env * (1 - y ** 2) * (rng.uniform(-1, 1, N) + 1j * rng.uniform(-1, 1, N))
            th[:, i, kz] = q
            if kz == 0 and kx > 0:
                th[:, plan.nkx - kx, 0] = np.conj(q)
    if mean is not None:
        th[:, 0, 0] = np.asarray(mean, float)
    return th


def linear_rate(NY: int = 33, Re: float = 400.0, Pr: float = 0.71, LX: float = 2 * np.pi, LZ: float = np.pi,
                stretch: float = 2.0, Q: float = 1.8):
    """Least-damped eigenvalue of kappa (D2 - k2) - i al U on the interior rows for the mode (kx, kz) =
    (1, 1) on the laminar U, and its eigenvector (zero at the walls): the linear advection-diffusion of
    one scalar mode, independent of the time stepping."""
    ops = ora.build_ops(NY, stretch)
    al, be = 2 * np.pi / LX, 2 * np.pi / LZ
    k2 = al * al + be * be
    U = 0.75 * Q * (1 - ops.y ** 2)
    kap = 1.0 / (Re * Pr)
    # D2 on the interior rows of a function that is zero at the walls: M^-1 K restricted there
    Mi, Ki = ops.M[1:-1, 1:-1], ops.K[1:-1, 1:-1]
    A = kap * (np.linalg.solve(Mi, Ki) - k2 * np.eye(NY - 2)) - 1j * al * np.diag(U[1:-1])
    lam, vec = np.linalg.eig(A)
    j = int(np.argmax(lam.real))
    v = np.zeros(NY, complex)
    v[1:-1] = vec[:, j]
    return lam[j], v / np.abs(v).max()
