import numbers

from gigalens_amd.profile import MassProfile


class Multipole(MassProfile):
    """An m-th order multipole of the lensing potential (beyond the reference; lenstronomy's ``MULTIPOLE`` by name and parameters).

    With ``dx = x - center_x``, ``dy = y - center_y``, ``r = |(dx, dy)|``, ``phi`` the polar angle, ``C = cos(m (phi - phi_m))``,
    ``S = sin(m (phi - phi_m))`` and ``k = a_m / (1 - m^2)``::

        psi     = k r C
        alpha_x = k (cos(phi) C + m sin(phi) S)
        alpha_y = k (sin(phi) C - m cos(phi) S)
        kappa   = a_m C / (2 r)

    ``m`` is an integer constant of the profile, ``2 <= m <= 8`` (``m = 1`` has another potential and is not served).  On top of an
    EPL, ``m = 4`` makes the isodensity contours boxy or discy and ``m = 3`` skews them.  At ``r = 0`` the deflection, the potential
    and every gradient are exact zeros (the convention of ``SIS``).
    """

    _name = "MULTIPOLE"
    _params = ["a_m", "phi_m", "center_x", "center_y"]
    _kind = 15
    M_MIN, M_MAX = 2, 8

    def __init__(self, m=4):
        super().__init__()
        if isinstance(m, bool) or not isinstance(m, numbers.Integral):
            raise ValueError(f"Multipole: the order m must be an integer, got {m!r}")
        if not self.M_MIN <= int(m) <= self.M_MAX:
            raise ValueError(f"Multipole: the order m must lie in {self.M_MIN}..{self.M_MAX}, got {m!r}")
        self.m = int(m)

    def _component(self):
        return (self._kind, self.m, 0)
