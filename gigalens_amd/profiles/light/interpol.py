import numpy as np

from gigalens_amd import _native
from gigalens_amd.profile import LightProfile


class Interpolated(LightProfile):
    """A pixelated source image rendered by interpolation (beyond the reference, whose light profiles are all parametric;
    lenstronomy's ``INTERPOL`` by name): an HST cut-out, a simulation snapshot or a reconstructed source, held fixed while its
    pose ``center_x, center_y, phi, scale`` and amplitude ``amp`` are sampled or fitted.

    ``image`` is a 2-D float array ``[H, W]``, a constant of the model shared by the whole batch.  With ``dx = x - center_x``,
    ``dy = y - center_y``::

        u = ( dx cos(phi) + dy sin(phi)) / scale + (W - 1) / 2      # column coordinate, +x = increasing column
        v = (-dx sin(phi) + dy cos(phi)) / scale + (H - 1) / 2      # row coordinate,    +y = increasing row
        I = amp * sum_j sum_i w(v - j) w(u - i) image[j, i]

    ``scale`` is arcsec per image pixel (> 0); ``I`` is surface brightness, not divided by ``scale**2``.  The image is
    zero-extended, so ``I`` is continuous everywhere and 0 beyond two pixels outside the image.  ``order`` 1: ``w`` is the hat
    function (bilinear); 3 (default): Keys' cubic convolution kernel with a = -1/2.  Gradients flow to the five parameters and to
    the lens (through the evaluation point), not to the pixels.  ``use_lstsq=True`` makes ``amp`` the linear coefficient."""

    _name = "INTERPOL"
    _params = ["center_x", "center_y", "phi", "scale"]
    _amp = "amp"
    _kind = 21
    MAX_SIDE = 2048

    def __init__(self, image, order=3, use_lstsq=False):
        super().__init__(use_lstsq=use_lstsq)
        img = np.asarray(image, dtype=np.float32)
        if img.ndim != 2 or img.size == 0:
            raise ValueError(f"Interpolated: image must be a non-empty 2-D array, got shape {img.shape}")
        if max(img.shape) > self.MAX_SIDE:
            raise ValueError(f"Interpolated: image of {img.shape[0]} x {img.shape[1]} pixels exceeds {self.MAX_SIDE} per side")
        if not np.all(np.isfinite(img)):
            raise ValueError("Interpolated: every image pixel must be finite")
        if order not in (1, 3):
            raise ValueError(f"Interpolated: order must be 1 (bilinear) or 3 (cubic convolution), got {order!r}")
        self.image = np.ascontiguousarray(img)
        self.order = int(order)
        self._dev_table = None  # the image with its zero apron on the device, for plugin-level `light`

    def _component(self):
        return (self._kind, 0, _native.GL_FLAG_INTERPOL_LINEAR if self.order == 1 else 0)

    def light(self, x, y, **kwargs):
        return _native.interpol_eval(self, x, y, kwargs)
