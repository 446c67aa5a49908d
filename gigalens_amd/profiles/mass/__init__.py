from gigalens_amd.profiles.mass import (dpie_series, dpie_subhalo, epl, interpol, nfw, piemd, piep, scaling_relation,  # noqa: F401
                                        shear, sie, sis, tnfw)
from gigalens_amd.profiles.mass.interpol import Interpolated  # noqa: F401
