"""Shared cases of the lensing-potential tests (test_potential_host.py, test_gpu_time_delays.py): the float64 host build of
the *_pot templates (tests/hostmath/potential_host.cpp) and, for every built-in mass kind, its gl_kind, the oracle's float64
deflection and a parameter sampler that reaches well beyond the priors."""
import ctypes
import os
import subprocess
from ctypes import POINTER, c_double, c_float, c_int

import numpy as np
import torch

from oracle import ref_torch as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = None


def potential_host():
    """ctypes handle of tests/hostmath/potential_host.cpp compiled with g++ (rebuilt when it or a csrc header is newer)."""
    global _SO
    if _SO is None:
        src = os.path.join(ROOT, "tests", "hostmath", "potential_host.cpp")
        so = os.path.join(ROOT, "tests", "hostmath", "libpotential_host.so")
        csrc = os.path.join(ROOT, "gigalens_amd", "csrc")
        deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h") and not f.endswith(".hip.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
        _SO = ctypes.CDLL(so)
        _SO.pot_mass_d.argtypes = [c_int, c_int, POINTER(c_double), c_int, POINTER(c_double), POINTER(c_double), POINTER(c_double)]
        _SO.pot_mass_f.argtypes = [c_int, c_int, POINTER(c_float), c_int, POINTER(c_float), POINTER(c_float), POINTER(c_float)]
        _SO.pot_scaled_d.argtypes = [c_int, c_int, POINTER(c_float), POINTER(c_int), POINTER(c_double), c_int, POINTER(c_double),
                                     POINTER(c_double), POINTER(c_double)]
    return _SO


def _dp(a):
    return a.ctypes.data_as(POINTER(c_double))


def host_psi(kind, p, x, y, iparam=50):
    """float64 psi of one built-in lens with parameter row ``p`` at the points (x, y)."""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    pp = np.ascontiguousarray(p, dtype=np.float64)
    out = np.empty_like(x)
    potential_host().pot_mass_d(kind, iparam, _dp(pp), x.size, _dp(x), _dp(y), _dp(out))
    return out


def host_psi_scaled(base_kind, cols, table, scales, x, y):
    """float64 psi of a dPIE-family catalogue (the member sum with scaled_dyn's parameters)."""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    t = np.ascontiguousarray(table, dtype=np.float32)
    c = np.ascontiguousarray(cols, dtype=np.int32)
    s = np.zeros(3, dtype=np.float64)
    s[:len(scales)] = scales
    out = np.empty_like(x)
    potential_host().pot_scaled_d(int(base_kind), t.shape[0], t.ctypes.data_as(POINTER(c_float)), c.ctypes.data_as(POINTER(c_int)),
                                  _dp(s), x.size, _dp(x), _dp(y), _dp(out))
    return out


def _u(r, lo, hi):
    return float(r.uniform(lo, hi))


def _ell(r, lo=0.05, hi=0.6):
    """(e1, e2) with lo <= |e| <= hi (|e| = 0 is the reference's NaN deflection for SIE and dPIE)."""
    m, a = _u(r, lo, hi), _u(r, -np.pi, np.pi)
    return m * np.cos(a), m * np.sin(a)


def _c(r):
    return _u(r, -0.6, 0.6), _u(r, -0.6, 0.6)


# name -> (gl_kind, oracle deflection, sampler of one parameter row in the reference's order == the native row)
KINDS = {
    "EPL": (1, ref.epl_deriv, lambda r: [_u(r, 0.3, 4.0), _u(r, 1.15, 2.85), *_ell(r, 0.0, 0.6), *_c(r)]),
    "SIE": (2, ref.sie_deriv, lambda r: [_u(r, 0.3, 4.0), *_ell(r), *_c(r)]),
    "NFW": (3, ref.nfw_deriv, lambda r: [_u(r, 0.3, 25.0), _u(r, 0.05, 6.0), *_c(r)]),
    "SHEAR": (4, ref.shear_deriv, lambda r: [_u(r, -0.4, 0.4), _u(r, -0.4, 0.4)]),
    "SIS": (5, ref.sis_deriv, lambda r: [_u(r, 0.3, 4.0), *_c(r)]),
    "dPIS": (6, ref.dpis_deriv, lambda r: [_u(r, 0.3, 4.0), _u(r, 0.005, 1.5), _u(r, 1.6, 40.0), *_c(r)]),
    "dPIE": (7, ref.dpie_deriv, lambda r: [_u(r, 0.3, 4.0), _u(r, 0.005, 1.5), _u(r, 1.6, 40.0), *_c(r), *_ell(r)]),
    "dPIEP": (8, ref.dpiep_deriv, lambda r: [_u(r, 0.3, 4.0), _u(r, 0.005, 1.5), _u(r, 1.6, 40.0), *_c(r), *_ell(r, 0.0, 0.6)]),
    "NFW_ELLIPSE": (11, ref.nfw_ellipse_deriv, lambda r: [_u(r, 0.3, 25.0), _u(r, 0.05, 6.0), *_ell(r, 0.0, 0.6), *_c(r)]),
    "TNFW": (12, ref.tnfw_deriv, lambda r: [_u(r, 0.3, 25.0), _u(r, 0.05, 6.0), _u(r, 0.5, 80.0), *_c(r)]),
}


def row_to_kwargs(name, p):
    """The parameter row of a kind as the oracle's keyword arguments."""
    names = {"EPL": ["theta_E", "gamma", "e1", "e2", "center_x", "center_y"],
             "SIE": ["theta_E", "e1", "e2", "center_x", "center_y"],
             "NFW": ["Rs", "alpha_Rs", "center_x", "center_y"],
             "SHEAR": ["gamma1", "gamma2"],
             "SIS": ["theta_E", "center_x", "center_y"],
             "dPIS": ["theta_E", "r_core", "r_cut", "center_x", "center_y"],
             "dPIE": ["theta_E", "r_core", "r_cut", "center_x", "center_y", "e1", "e2"],
             "dPIEP": ["theta_E", "Ra", "Rs", "center_x", "center_y", "e1", "e2"],
             "NFW_ELLIPSE": ["Rs", "alpha_Rs", "e1", "e2", "center_x", "center_y"],
             "TNFW": ["Rs", "alpha_Rs", "r_trunc", "center_x", "center_y"]}[name]
    return dict(zip(names, [float(v) for v in p]))


def oracle_alpha(name, p, x, y):
    fn = KINDS[name][1]
    ax, ay = fn(torch.as_tensor(np.asarray(x, dtype=np.float64)), torch.as_tensor(np.asarray(y, dtype=np.float64)),
                **row_to_kwargs(name, p))
    return ax.numpy(), ay.numpy()


def points_away(r, n, centre, r_min=0.2, box=6.0):
    """n points in [-box, box]^2 at least r_min from ``centre``."""
    pts = []
    while len(pts) < n:
        x, y = r.uniform(-box, box, 2)
        if np.hypot(x - centre[0], y - centre[1]) >= r_min:
            pts.append((x, y))
    a = np.asarray(pts)
    return a[:, 0], a[:, 1]


def gauss_legendre_delta(alpha_fn, xa, ya, xb, yb, n_nodes=64, n_panels=16):
    """psi(B) - psi(A) as the float64 line integral of the deflection ``alpha_fn(x, y) -> (ax, ay)`` along the segment A -> B
    (composite Gauss-Legendre: n_panels panels of n_nodes nodes)."""
    t, w = np.polynomial.legendre.leggauss(n_nodes)
    xa, ya, xb, yb = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (xa, ya, xb, yb))
    edges = np.linspace(0.0, 1.0, n_panels + 1)
    s = ((edges[:-1, None] + edges[1:, None]) / 2 + (edges[1:, None] - edges[:-1, None]) / 2 * t[None, :]).reshape(-1)
    ws = (np.repeat((edges[1:] - edges[:-1]) / 2, n_nodes) * np.tile(w, n_panels))
    px = xa[:, None] + (xb - xa)[:, None] * s[None, :]
    py = ya[:, None] + (yb - ya)[:, None] * s[None, :]
    ax, ay = alpha_fn(px, py)
    return ((np.asarray(ax) * (xb - xa)[:, None] + np.asarray(ay) * (yb - ya)[:, None]) * ws[None, :]).sum(axis=1)
