import numpy as np

from gigalens_amd import _native
from gigalens_amd.profile import MassProfile


class Interpolated(MassProfile):
    """A lens given as deflection maps on a grid (beyond the reference, whose lenses are all parametric; lenstronomy's
    ``INTERPOL_SCALED`` by name): a cluster halo from a Lenstool or free-form model, a released deflection map or an N-body halo,
    held fixed while ``scale_factor, center_x, center_y`` and the lenses beside it are sampled or fitted.

    ``alpha_x`` and ``alpha_y`` are 2-D float arrays ``[H, W]`` of one shape, in arcsec, constants of the model shared by the
    whole batch; ``pitch`` is arcsec per map pixel.  With ``dx = x - center_x``, ``dy = y - center_y``::

        u = dx / pitch + (W - 1) / 2      # column coordinate, +x = increasing column
        v = dy / pitch + (H - 1) / 2      # row coordinate,    +y = increasing row
        alpha_x(x, y) = scale_factor * sum_j sum_i w(v - j) w(u - i) alpha_x[j, i]      # alpha_y likewise

    the conventions of the interpolated light.  ``w`` is Keys' cubic convolution kernel with a = -1/2 and the maps are
    zero-extended, so the deflection is C1 everywhere and 0 beyond two pixels outside the maps (a coordinate that is not finite
    included).  There is no rotation and no bilinear order.  The Hessian is the derivative of this interpolant, each entry as it
    is: ``f_xy`` and ``f_yx`` are not symmetrised.  The maps should therefore be the gradient of ONE potential, and they should
    cover the simulator's grid: outside the maps, plus two pixels, the lens is absent.

    The maps carry no potential: ``potential``, the Fermat potential, time delays and the time-delay likelihood term raise
    ``_native.UnsupportedLensError``, as do lens planes, a ``ScalingRelation`` over this profile and a model that mixes it with
    user-written profiles.  Gradients flow to the three parameters, not to the map pixels."""

    _name = "INTERPOL_SCALED"
    _params = ["scale_factor", "center_x", "center_y"]
    _kind = 14
    MAX_SIDE = 2048

    def __init__(self, alpha_x, alpha_y, pitch):
        super().__init__()
        ax, ay = np.asarray(alpha_x, dtype=np.float32), np.asarray(alpha_y, dtype=np.float32)
        for name, a in (("alpha_x", ax), ("alpha_y", ay)):
            if a.ndim != 2 or a.size == 0:
                raise ValueError(f"Interpolated: {name} must be a non-empty 2-D array, got shape {a.shape}")
        if ax.shape != ay.shape:
            raise ValueError(f"Interpolated: alpha_x {ax.shape} and alpha_y {ay.shape} must have one shape")
        if max(ax.shape) > self.MAX_SIDE:
            raise ValueError(f"Interpolated: maps of {ax.shape[0]} x {ax.shape[1]} pixels exceed {self.MAX_SIDE} per side")
        if not (np.all(np.isfinite(ax)) and np.all(np.isfinite(ay))):
            raise ValueError("Interpolated: every map value must be finite")
        try:
            pitch = float(pitch)
        except (TypeError, ValueError):
            raise ValueError(f"Interpolated: pitch must be a number, got {pitch!r}") from None
        with np.errstate(over="ignore"):  # (a pitch whose reciprocal leaves the float32 range is refused below)
            inv = np.float32(1.0 / pitch) if pitch else np.float32(np.inf)
        if not (np.isfinite(pitch) and pitch > 0 and np.isfinite(inv) and inv > 0):
            raise ValueError(f"Interpolated: pitch must be finite and > 0 (arcsec per map pixel), got {pitch!r}")
        self.alpha_x = np.ascontiguousarray(ax)
        self.alpha_y = np.ascontiguousarray(ay)
        self.pitch = pitch
        self._dev_table = None  # both maps with their zero aprons on the device, for plugin-level `deriv` / `hessian`

    def deriv(self, x, y, **kwargs):
        """Deflection ``(alpha_x, alpha_y)`` at ``(x, y)``.  Forward only."""
        return _native.interpol_mass_eval(self, x, y, kwargs, hessian=False)

    def hessian(self, x, y, **kwargs):
        """``(f_xx, f_xy, f_yx, f_yy)``: the derivative of the interpolant, from forward-mode duals.  Forward only."""
        return _native.interpol_mass_eval(self, x, y, kwargs, hessian=True)

    def potential(self, x, y, **kwargs):
        raise _native.UnsupportedLensError(f"profile {self.name!r}: deflection maps carry no potential")
