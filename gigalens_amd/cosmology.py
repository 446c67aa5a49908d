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
