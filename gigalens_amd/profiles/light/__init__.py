from gigalens_amd.profiles.light import interpol, sersic, shapelets  # noqa: F401
from gigalens_amd.profiles.light.interpol import Interpolated  # noqa: F401
