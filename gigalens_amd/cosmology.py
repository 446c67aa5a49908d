"""Distance ratios of a flat LambdaCDM cosmology (beyond the reference; host only, numpy float64).

A lens at ``z_lens`` bends the light of a source at ``z_source`` by the physical deflection times ``D_LS / D_S``.  A model fitted
in the reduced deflection of one reference source plane ``z_ref`` therefore serves a source at another redshift with the scale

    c = [D_LS / D_S](z_source) / [D_LS / D_S](z_ref),      beta = theta - c sum alpha,   A = I - c H,

which is what ``PhysicalModel(source_light_scales=...)``, ``ForwardProbModel(centroids_scales=...)`` and the ``deflection_scale``
keyword of ``LensSimulator`` take.  In a flat universe ``D_LS / D_S = 1 - D_C(z_lens) / D_C(z_source)`` with the comoving distance
``D_C(z) = (c / H0) int_0^z dz' / E(z')``, ``E(z) = sqrt(omega_m (1 + z)^3 + 1 - omega_m)``: the Hubble constant cancels.
"""
import numpy as np

# Gauss-Legendre nodes on [-1, 1]: E(z) is smooth, 64 nodes integrate 1 / E to float64 rounding for every z of interest
_GL_X, _GL_W = np.polynomial.legendre.leggauss(64)


def comoving_distance(z, omega_m=0.3):
    """``D_C(z) H0 / c`` of flat LambdaCDM, vectorised over ``z`` (float64)."""
    z = np.asarray(z, dtype=np.float64)
    half = 0.5 * z[..., None]
    zz = half * (_GL_X + 1.0)  # nodes on [0, z]
    inv_e = 1.0 / np.sqrt(omega_m * (1.0 + zz) ** 3 + (1.0 - omega_m))
    return (inv_e * _GL_W).sum(axis=-1) * half[..., 0]


def distance_ratio(z_lens, z_source, omega_m=0.3):
    """``D_LS / D_S`` of flat LambdaCDM, vectorised over ``z_source``."""
    return 1.0 - comoving_distance(z_lens, omega_m) / comoving_distance(z_source, omega_m)


def deflection_scale(z_lens, z_source, z_ref, omega_m=0.3):
    """``c = [D_LS / D_S](z_source) / [D_LS / D_S](z_ref)``, vectorised over ``z_source`` (float64; a scalar for a scalar).
    ``ValueError`` unless every source, and the reference plane, lies behind the lens (``z > z_lens``) and ``z_lens > 0``."""
    zs = np.asarray(z_source, dtype=np.float64)
    if not (np.isfinite(z_lens) and z_lens > 0.0):
        raise ValueError(f"z_lens must be finite and > 0, got {z_lens}")
    if not np.all(np.isfinite(zs)) or np.any(zs <= z_lens):
        raise ValueError(f"every z_source must be finite and > z_lens = {z_lens}, got {zs.tolist()}")
    if not (np.isfinite(z_ref) and z_ref > z_lens):
        raise ValueError(f"z_ref must be finite and > z_lens = {z_lens}, got {z_ref}")
    c = distance_ratio(z_lens, zs, omega_m) / distance_ratio(z_lens, z_ref, omega_m)
    return float(c) if zs.ndim == 0 else c


class MultiPlane:
    """Couplings of lens planes at several redshifts (multi-plane ray tracing; host only, numpy float64).

    Every lens keeps its parameters as the reduced deflection for the reference plane ``z_ref``.  With the planes sorted by
    redshift, ``z_1 < ... < z_K``, a ray that leaves the observer at ``theta`` meets plane j at

        theta_j = theta - sum_{i<j} C_ij a_i,   a_i = sum_{lenses l on plane i} alpha_l(theta_i),   theta_1 = theta,

    and a target t behind some of the planes at ``beta_t = theta - sum_{i: z_i < z_t} C_it a_i``, with the coupling
    ``C_ij = deflection_scale(z_i, z_j, z_ref) = [D_ij / D_j] / [D_i,ref / D_ref]``.  One plane gives ``beta = theta - c sum alpha``.

    ``z_lenses``: one redshift per lens of the model, in the model's order; lenses at equal redshift share a plane.  ``z_sources``: one
    per source light.  Attributes: ``z_planes`` ``[K]`` ascending; ``plane_of_lens`` (one int per lens); ``lens_scales`` ``[K, K]``,
    strictly upper triangular; ``source_scales`` ``[K, S]`` (0 for the planes at or behind a source); ``K``, ``S``.
    ``ValueError``: a redshift that is not finite or not > 0, ``z_ref`` not behind every lens, a source at or in front of the first
    plane, more than ``MAX_PLANES`` planes."""

    MAX_PLANES = 4

    def __init__(self, z_lenses, z_sources, z_ref, omega_m=0.3):
        zl = np.atleast_1d(np.asarray(z_lenses, dtype=np.float64))
        zs = np.atleast_1d(np.asarray(z_sources, dtype=np.float64)) if np.size(z_sources) else np.zeros(0)
        if zl.ndim != 1 or zl.size == 0:
            raise ValueError("z_lenses: one redshift per lens, at least one")
        if zs.ndim != 1:
            raise ValueError("z_sources: one redshift per source light")
        for what, z in (("z_lenses", zl), ("z_sources", zs), ("z_ref", np.atleast_1d(np.float64(z_ref)))):
            if not (np.all(np.isfinite(z)) and np.all(z > 0.0)):
                raise ValueError(f"{what}: every redshift must be finite and > 0, got {z.tolist()}")
        self.z_ref, self.omega_m = float(z_ref), float(omega_m)
        if not self.z_ref > zl.max():
            raise ValueError(f"z_ref = {self.z_ref} must lie behind every lens plane (largest z_lens = {zl.max()})")
        self.z_planes, inverse = np.unique(zl, return_inverse=True)
        self.plane_of_lens = inverse.astype(np.int32).reshape(-1)
        self.K, self.S = int(self.z_planes.size), int(zs.size)
        if self.K > self.MAX_PLANES:
            raise ValueError(f"{self.K} lens planes: at most {self.MAX_PLANES} are served")
        if np.any(zs <= self.z_planes[0]):
            raise ValueError(f"every source must lie behind the first lens plane (z = {self.z_planes[0]}), got {zs.tolist()}")
        self.z_sources = zs
        self.lens_scales = np.zeros((self.K, self.K))
        for i in range(self.K - 1):
            self.lens_scales[i, i + 1:] = deflection_scale(self.z_planes[i], self.z_planes[i + 1:], self.z_ref, omega_m)
        self.source_scales = (np.stack([self.target_scales(z) for z in zs], axis=1) if self.S else np.zeros((self.K, 0)))

    def target_scales(self, z):
        """``[K]`` couplings of a target plane at redshift ``z``: ``deflection_scale(z_i, z, z_ref)`` for the planes in front of it, 0
        for those at or behind it.  ``ValueError`` unless ``z`` is finite and behind the first plane."""
        z = float(z)
        if not (np.isfinite(z) and z > self.z_planes[0]):
            raise ValueError(f"a target must be finite and lie behind the first lens plane (z = {self.z_planes[0]}), got {z}")
        out = np.zeros(self.K)
        for i, zi in enumerate(self.z_planes):
            if zi < z:
                out[i] = deflection_scale(zi, z, self.z_ref, self.omega_m)
        return out

    def delay_weights(self, z):
        """``(geom [K], pot [K])`` (float64): the weights of the arrival time of a ray to a source at redshift ``z``,

            T = sum_{i <= K_s} [ geom_i |theta_i - theta_next(i)|^2 / 2 - pot_i psi_i(theta_i) ],

        over the planes in front of the source (``next(i)`` = plane i + 1, or the source behind the last of them), in arcsec^2 times
        ``c / H0``.  With ``chi = comoving_distance``: ``geom_i = chi_i chi_next / (chi_next - chi_i)`` and
        ``pot_i = chi_i chi_ref / (chi_ref - chi_i)`` -- the potential of a lens is that of its reduced deflection for ``z_ref``, so its
        weight is a constant of the plane, and ``geom_i C_i,next(i) = pot_i``.  Planes at or behind ``z`` get 0 in both arrays.  One
        plane: ``geom_0 = D_dt H0 / c``.  ``ValueError`` under the rules of ``target_scales``."""
        z = float(z)
        if not (np.isfinite(z) and z > self.z_planes[0]):
            raise ValueError(f"a target must be finite and lie behind the first lens plane (z = {self.z_planes[0]}), got {z}")
        front = self.z_planes < z
        chi = comoving_distance(self.z_planes, self.omega_m)
        chi_ref, chi_s = (float(comoving_distance(v, self.omega_m)) for v in (self.z_ref, z))
        ks = int(front.sum())
        nxt = np.append(chi[1:ks], chi_s)  # chi of next(i) for the ks planes in front of the source
        geom, pot = np.zeros(self.K), np.zeros(self.K)
        geom[:ks] = chi[:ks] * nxt / (nxt - chi[:ks])
        pot[:ks] = chi[:ks] * chi_ref / (chi_ref - chi[:ks])
        return geom, pot


C_KM_S = 299792.458


def hubble_distance_mpc(h0):
    """``c / H0`` in Mpc for ``h0`` in km/s/Mpc (a scalar or an array).  ``ValueError`` unless every ``h0`` is finite and > 0."""
    h = np.asarray(h0, dtype=np.float64)
    if not (np.all(np.isfinite(h)) and np.all(h > 0.0)):
        raise ValueError(f"h0 must be finite and > 0 (km/s/Mpc), got {h0}")
    d = C_KM_S / h
    return float(d) if h.ndim == 0 else d
