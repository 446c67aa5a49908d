from gigalens_amd.profiles.mass import (dpie_series, dpie_subhalo, epl, interpol, multipole, nfw, piemd, piep,  # noqa: F401
                                        scaling_relation, shear, sie, sis, tnfw)
from gigalens_amd.profiles.mass.interpol import Interpolated  # noqa: F401
from gigalens_amd.profiles.mass.multipole import Multipole  # noqa: F401
