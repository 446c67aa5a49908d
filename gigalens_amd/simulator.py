"""``SimulatorConfig`` / ``LensWCS`` / ``LensSimulator`` with the reference's surface
(src/gigalens/simulator.py:11-127, src/gigalens/tf/simulator.py:13-156), executing on HIP kernels.

Differences in HOW (not WHAT): the pixel grid is stored once as two ``(N,)`` device arrays instead of
``(N, bs)`` replicas (the reference's own ``# TODO: no need for batched grid``, tf/simulator.py:11);
ray-shooting, rendering, NaN->0 and the det(T) scale are one fused kernel; gradients come from
hand-written VJP kernels wrapped in a ``torch.autograd.Function``.
"""
import math
import warnings
from dataclasses import dataclass
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from gigalens_amd import _native


@dataclass
class SimulatorConfig:
    """src/gigalens/simulator.py:11-29 (field for field)."""

    delta_pix: float
    num_pix: int
    supersample: Optional[int] = 1
    kernel: Optional[Any] = None
    transform_pix2angle: Optional[np.array] = None
    pix_region: Optional[np.array] = None


class LensWCS:
    """Pixel <-> angle transform, src/gigalens/simulator.py:32-64, quirks included: ``pix2angle``
    applies T^T while the origin uses T (:50,53); ``transform_angle2pix`` inverts the un-supersampled
    T (:37-38); ``pixel_grid`` uses ``n_y`` for both axes (:62)."""

    def __init__(self, n, supersample=1, transform_pix2angle=None, pix_scale=1.0):
        if transform_pix2angle is None:
            transform_pix2angle = np.eye(2) * pix_scale
        transform_pix2angle = np.asarray(transform_pix2angle, dtype=np.float64)
        self.transform_pix2angle = transform_pix2angle / supersample
        self.transform_angle2pix = np.linalg.inv(transform_pix2angle)
        if isinstance(n, (int, np.integer)):
            self.n_x, self.n_y = int(n), int(n)
        else:
            self.n_x, self.n_y = n
        self.supersample = supersample
        low_x = -(self.n_x * self.supersample - 1) / 2
        low_y = -(self.n_y * self.supersample - 1) / 2
        self.radec_at_xy_0 = np.squeeze(self.transform_pix2angle @ np.array([[low_x], [low_y]]))

    def pix2angle(self, x, y):
        xy = np.stack([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)])
        radec = np.tensordot(self.transform_pix2angle.T, xy, axes=1)
        ra = radec[0] + self.radec_at_xy_0[0]
        dec = radec[1] + self.radec_at_xy_0[1]
        return ra.astype(np.float32), dec.astype(np.float32)

    def angle2pix(self, ra, dec):
        radec = np.stack([np.asarray(ra, dtype=np.float64) - self.radec_at_xy_0[0],
                          np.asarray(dec, dtype=np.float64) - self.radec_at_xy_0[1]])
        return np.tensordot(self.transform_angle2pix.T, radec, axes=1).astype(np.float32)

    def pixel_grid(self):
        x = np.arange(self.n_y * self.supersample)
        X, Y = np.meshgrid(x, x)
        return self.pix2angle(X, Y)


class LensSimulatorInterface:
    """src/gigalens/simulator.py:67-127."""

    def __init__(self, phys_model, sim_config: SimulatorConfig, bs: int):
        self.phys_model = phys_model
        self.sim_config = sim_config
        self.bs = bs
        self.wcs = LensWCS(n=sim_config.num_pix, supersample=sim_config.supersample,
                           transform_pix2angle=sim_config.transform_pix2angle, pix_scale=sim_config.delta_pix)

    @staticmethod
    def get_coords(supersample: int, num_pix: int, transform_pix2angle):
        """src/gigalens/simulator.py:129-162 (a legacy helper no simulator of the reference calls): the grid with mean
        coordinate (0, 0).  The reference builds it with lenstronomy's ``PixelGrid`` (third party); its published rule is
        ``ra = ra_at_xy_0 + T00 ix + T01 iy``, ``dec = dec_at_xy_0 + T10 ix + T11 iy`` with ``ix`` along the columns,
        restated here.  Returns ``(ra_at_xy_0, dec_at_xy_0, img_x, img_y)`` with float32 ``(n, n)`` grids."""
        n = int(supersample) * int(num_pix)
        T = np.asarray(transform_pix2angle, dtype=np.float64)
        lo = np.arange(0, n, dtype=np.float32)
        lo = np.min(lo - np.mean(lo))
        ra0, dec0 = np.squeeze(T @ np.array([[lo], [lo]], dtype=np.float64))
        ix, iy = np.meshgrid(np.arange(n), np.arange(n))
        img_x = (ra0 + T[0, 0] * ix + T[0, 1] * iy).astype(np.float32)
        img_y = (dec0 + T[1, 0] * ix + T[1, 1] * iy).astype(np.float32)
        return ra0, dec0, img_x, img_y


class _SimulateFn(torch.autograd.Function):
    """autograd glue: forward = gl_simulate_fwd, backward = gl_simulate_bwd (both HIP)."""

    @staticmethod
    def forward(ctx, params, model):
        ctx.model = model
        ctx.save_for_backward(params)
        return model.simulate_fwd(params)

    @staticmethod
    def backward(ctx, grad_img):
        (params,) = ctx.saved_tensors
        return ctx.model.simulate_bwd(params, grad_img), None


class _PointImagesFn(torch.autograd.Function):
    """autograd glue: forward = gl_ptimg_render, backward = gl_ptimg_render_bwd (both HIP)."""

    @staticmethod
    def forward(ctx, x, y, amplitude, model, transform):
        ctx.model, ctx.transform = model, transform
        ctx.save_for_backward(x, y, amplitude)
        return model.ptimg_render(x, y, amplitude, transform)

    @staticmethod
    def backward(ctx, grad_img):
        x, y, amplitude = ctx.saved_tensors
        gx, gy, ga = ctx.model.ptimg_render_bwd(x, y, amplitude, ctx.transform, grad_img.contiguous())
        return gx, gy, ga, None, None


class LensSimulator(LensSimulatorInterface):
    """Drop-in for ``gigalens.tf.simulator.LensSimulator`` (tf/simulator.py:13-156).

    Attributes kept from the reference: ``img_X``, ``img_Y`` (here ``(N,)``, not ``(N, bs)``), ``img_region``,
    ``region``, ``bs``, ``wcs``, ``supersample``, ``conversion_factor``.
    """

    def __init__(self, phys_model, sim_config: SimulatorConfig, bs: int, supersampled_kernel=None):
        """``sim_config.kernel`` with ``supersample > 1`` is brought to the supersampled grid like the reference does
        (tf/simulator.py:60-70: lenstronomy's ``subgrid_kernel(kernel, supersample, odd=True)``, restated in
        gigalens_amd/kernel_util.py -- third party, parity unpinned).  ``supersampled_kernel`` overrides it with a PSF
        already sampled on the supersampled grid."""
        super().__init__(phys_model, sim_config, bs)
        self.device = _native.device()
        self.supersample = int(sim_config.supersample)
        T = (np.eye(2) * sim_config.delta_pix if sim_config.transform_pix2angle is None
             else np.asarray(sim_config.transform_pix2angle, dtype=np.float64))
        # tf/simulator.py:27-29: det of the un-supersampled transform, in float32
        self.conversion_factor = float(np.float32(np.linalg.det(T.astype(np.float32))))
        ss = self.supersample
        Hs, Ws = self.wcs.n_x * ss, self.wcs.n_y * ss
        if sim_config.pix_region is None:  # tf/simulator.py:34-42
            region = np.ones((Hs, Ws), dtype=bool)
            img_region = np.ones((self.wcs.n_x, self.wcs.n_y))
        else:
            img_region = np.asarray(sim_config.pix_region)
            region = np.repeat(np.repeat(img_region, ss, axis=0), ss, axis=1).astype(bool)
        self._region_np = np.argwhere(region)  # == tf.where: row-major [row, col]
        img_X, img_Y = self.wcs.pix2angle(self._region_np[:, 1], self._region_np[:, 0])
        full = self._region_np.shape[0] == Hs * Ws
        pix_index = None if full else (self._region_np[:, 0] * Ws + self._region_np[:, 1]).astype(np.int32)
        self.region = torch.from_numpy(self._region_np).to(self.device)
        self.img_region = torch.from_numpy(img_region.astype(np.float32)).to(self.device)
        self.img_X = torch.from_numpy(img_X).to(self.device)
        self.img_Y = torch.from_numpy(img_Y).to(self.device)
        self.numPix = sim_config.num_pix
        self.depth = len(phys_model.lens_light) + len(phys_model.source_light)
        psf = None
        if supersampled_kernel is not None:
            psf = np.asarray(supersampled_kernel, dtype=np.float32)
        elif sim_config.kernel is not None:
            from gigalens_amd.kernel_util import subgrid_kernel
            psf = np.asarray(subgrid_kernel(np.asarray(sim_config.kernel), ss, odd=True), dtype=np.float32)
        self.kernel = psf
        # what the probabilistic models keep per simulator
        self._n_eff = None  # pixels of the region (ForwardProbModel._n_eff)
        self._linear_cols_dev = None  # the linear columns of the layout on the device (BackwardProbModel.log_prob)
        self._lp_graphs = {}  # {(id(prob_model), shape of z): model._GraphEntry} of log_prob_and_grad(graph=True)
        self._lp_captures = 0  # how many of them were captured so far
        self._point_cache = None  # (key, inputs, checked data) of the last point-image fit on device tensors (_point_data)
        self._mp =getattr(phys_model, "multiplane", None)  # lenses on planes of their own (PhysicalModel multiplane, K >= 2)
        if self._mp is not None:
            self._refuse_on_planes_profiles()
        bodies = []  # user-written profile bodies (profile.py `hip_body`): compiled into this model's kernels
        comps = ([_native.component_of(p, bodies) for p in phys_model.lenses]
                 + [_native.component_of(p, bodies) for p in phys_model.lens_light]
                 + [_native.component_of(p, bodies) for p in phys_model.source_light])
        self._model = _native.Model(comps, len(phys_model.lenses), len(phys_model.lens_light),
                                    len(phys_model.source_light), Hs, Ws, ss, img_X, img_Y, pix_index,
                                    self.conversion_factor, psf, bodies=bodies)
        for i, lens in enumerate(phys_model.lenses):
            if getattr(lens, "_kind", 0) == 10:  # series expansion: the field must live on THIS pixel list
                if lens.x is not self.img_X or lens._coefs is None:
                    lens.set_grid(self.img_X, self.img_Y)
                    lens.set_deriv()
                self._model.set_series(i, lens.series_var_0, lens._coefs)
            elif getattr(lens, "_kind", 0) == 9:  # galaxy catalogues of ScalingRelation lenses (fused dPIE-family kernels)
                self._model.set_catalogue(i, *lens._catalogue())
            elif getattr(lens, "_kind", 0) == _native.GL_INTERPOL_MASS:  # the deflection maps of an Interpolated lens
                self._model.set_lens_maps(i, lens.alpha_x, lens.alpha_y, lens.pitch)
        for i, light in enumerate(list(phys_model.lens_light) + list(phys_model.source_light)):
            if getattr(light, "_kind", 0) == _native.GL_INTERPOL:  # the image of an Interpolated light, a constant of the model
                self._model.set_light_image(len(phys_model.lenses) + i, light.image)
        if self._mp is not None:
            self._model.set_lens_planes(self._mp.plane_of_lens, self._mp.lens_scales, self._mp.source_scales)
        if getattr(phys_model, "_source_scales_given", False):  # sources on planes of their own (PhysicalModel source_light_scales)
            self._model.set_source_scales(phys_model.source_light_scales)
        self._layout = phys_model._packing()
        assert self._layout.P == self._model.P

    # -- lenses on planes of their own (PhysicalModel multiplane with K >= 2) ------------------------
    def _refuse_on_planes_profiles(self):
        pm = self.phys_model
        for i, lens in enumerate(pm.lenses):
            if getattr(lens, "_kind", 0) == 10:
                raise _native.UnsupportedLensError(f"lens {i} ({lens.name}): a series expansion stores its field on the image-plane "
                                                   "grid, not at the ray's position on the lens's own plane: not served on lens planes")
            if getattr(lens, "_kind", 0) == _native.GL_INTERPOL_MASS:
                raise _native.UnsupportedLensError(f"lens {i} ({lens.name}): an interpolated lens is not served on lens planes")
        for p in list(pm.lenses) + list(pm.lens_light) + list(pm.source_light):
            if not getattr(p, "_kind", 0):
                raise _native.UnsupportedLensError(f"profile {p.name!r}: user-written bodies (hip_body) and run-time compiled member "
                                                   "loops are not served on lens planes")

    def _single_plane(self, what):
        if self._mp is not None:
            raise _native.UnsupportedLensError(f"{what} does not serve a model with {self._mp.K} lens planes: multi-plane ray tracing "
                                               "serves beta, magnification, convergence, shear, rotation, simulate*, simulate_vjp, "
                                               "the pixel likelihood with its gradient, image_positions(source_redshifts=...), "
                                               "time_delays(source_redshifts=...), fermat_potential(source_redshift=...), "
                                               "critical_curves(source_redshifts=...) and einstein_radius(source_redshifts=...)")

    def _target_scales(self, deflection_scale):
        """The ``deflection_scale`` keyword of the lens maps on a multi-plane model: a source index, or the ``[K]`` couplings of the
        target plane (``MultiPlane.target_scales(z)``)."""
        mp = self._mp
        if isinstance(deflection_scale, (int, np.integer)) and not isinstance(deflection_scale, bool):
            if not 0 <= int(deflection_scale) < mp.S:
                raise ValueError(f"deflection_scale: source index {deflection_scale} outside [0, {mp.S})")
            return np.asarray(mp.source_scales[:, int(deflection_scale)], dtype=np.float32)
        t = np.asarray(deflection_scale, dtype=np.float64)
        if t.shape != (mp.K,):
            raise ValueError(f"deflection_scale: a model with {mp.K} lens planes takes a source index or the [{mp.K}] couplings of "
                             f"the target plane (MultiPlane.target_scales(z)), got {deflection_scale!r}")
        if not (np.all(np.isfinite(t)) and np.all(t >= 0)):
            raise ValueError(f"deflection_scale: every coupling must be finite and >= 0, got {t.tolist()}")
        return t.astype(np.float32)

    def _mp_maps(self, what, x, y, lens_params, deflection_scale):
        t = self._target_scales(deflection_scale)
        packed = self._lens_rows(lens_params)
        self._forward_only(what, packed, x, y)
        return self._model.multiplane_maps(packed, x, y, t)

    # -- packing between the reference's nested parameter dicts and the native [B, P] rows ---------
    def pack(self, params: Dict[str, List[Dict]]):
        return self._layout.pack(params, self.bs, self.device)

    @staticmethod
    def _scale(deflection_scale):
        """A scalar ``deflection_scale`` keyword as a float (``ValueError`` unless finite and > 0)."""
        return float(_native.deflection_scales(deflection_scale, 1, "deflection_scale")[0])

    def beta(self, x, y, lens_params: List[Dict], deflection_scale=1.0):
        """tf/simulator.py:72-78 on arbitrary points (plugin-level kernels, one per lens).  ``deflection_scale`` (beyond the
        reference, as on the methods below): the scale c of a source plane at another redshift than the model's reference plane
        (``gigalens_amd.cosmology.deflection_scale``): ``beta = theta - c sum alpha``, Hessian ``c H``."""
        if self._mp is not None:  # lens planes: ``deflection_scale`` a source index or MultiPlane.target_scales(z)
            maps = self._mp_maps("beta", x, y, lens_params, deflection_scale)
            return maps[0], maps[1]
        cs = self._scale(deflection_scale)
        beta_x, beta_y = x, y
        for lens, p, c in zip(self.phys_model.lenses, lens_params, self.phys_model.lenses_constants):
            f_xi, f_yi = lens.deriv(x, y, **p, **c)
            beta_x, beta_y = beta_x - f_xi, beta_y - f_yi
        if cs != 1.0:
            beta_x, beta_y = x + cs * (beta_x - x), y + cs * (beta_y - y)
        return beta_x, beta_y

    def _lens_maps(self, x, y, lens_params):
        packed = self._pack_partial({"lens_mass": lens_params}) if not torch.is_tensor(lens_params) else lens_params
        series = [(i, l) for i, l in enumerate(self.phys_model.lenses) if getattr(l, "_kind", 0) == 10]
        if not series:
            return self._model.lens_maps(packed, x, y)
        # a series lens answers on its own grid whatever (x, y) it is handed (series_profile.py:76,83 TODO); the
        # reference then silently mixes grids -- here anything but the simulator's grid is refused
        xt = torch.as_tensor(x, dtype=torch.float32, device=self.device)
        yt = torch.as_tensor(y, dtype=torch.float32, device=self.device)
        n = self.img_X.numel()
        if xt.numel() % n or yt.numel() % n or xt.shape[0] != n or yt.shape[0] != n or \
                not (torch.equal(xt.reshape(n, -1)[:, 0], self.img_X) and torch.equal(yt.reshape(n, -1)[:, 0], self.img_Y)):
            raise ValueError("a model with series-expansion lenses maps only the simulator's own grid (img_X, img_Y)")
        for i, lens in series:
            if lens._hcoefs is None:
                lens.set_hessian()
            if getattr(lens, "_hessian_bound", None) is not lens._hcoefs:
                self._model.set_series_hessian(i, lens._hcoefs)
                lens._hessian_bound = lens._hcoefs
        return self._model.lens_maps(packed, None, None)

    def beta_vjp(self, x, y, lens_params, cot_x, cot_y, deflection_scale=1.0):
        """The VJP of ``beta`` with respect to the lens parameters (beyond the reference, whose tape does this): the cotangents
        ``cot_x, cot_y`` on ``beta_x, beta_y`` at ``(x, y)`` (point layout as the lens maps: broadcastable to ``(..., B)``) -> the
        gradient ``[B, P]`` in packed order, zero outside the lens-mass columns.  ``beta = theta - c sum alpha``, so the cotangent is
        scaled by ``c = deflection_scale``.  A point whose two cotangents are both exactly 0, or not finite, is skipped (its
        deflection is never formed).  Deterministic.  ``UnsupportedLensError``: lens planes, series and user-written lenses."""
        self._single_plane("beta_vjp")
        cs = self._scale(deflection_scale)
        packed = self._pack_partial({"lens_mass": lens_params}) if not torch.is_tensor(lens_params) else lens_params
        cot_x = torch.as_tensor(cot_x, dtype=torch.float32, device=self.device)
        cot_y = torch.as_tensor(cot_y, dtype=torch.float32, device=self.device)
        if cs != 1.0:
            cot_x, cot_y = cs * cot_x, cs * cot_y
        return self._model.lens_maps_vjp(packed, x, y, cot_x, cot_y)

    def hessian_vjp(self, x, y, lens_params, cot_xx, cot_xy, cot_yx, cot_yy, deflection_scale=1.0):
        """The VJP of the summed Hessian ``f_xx, f_xy, f_yx, f_yy`` of the lens maps (what ``convergence``, ``shear`` and
        ``magnification`` are made of) with respect to the lens parameters (beyond the reference, whose tape does this): the four
        cotangents at ``(x, y)`` (point layout as the lens maps: broadcastable to ``(..., B)``) -> the gradient ``[B, P]`` in packed
        order, zero outside the lens-mass columns.  The Hessian of a plane at ``c = deflection_scale`` is ``c H``, so the
        cotangents are scaled by ``c``.  A point whose four cotangents are all exactly 0, or one of which is not finite, is
        skipped (its lens is never evaluated).  Deterministic.  ``UnsupportedLensError``: lens planes, series and user-written
        lenses."""
        self._single_plane("hessian_vjp")
        cs = self._scale(deflection_scale)
        packed = self._pack_partial({"lens_mass": lens_params}) if not torch.is_tensor(lens_params) else lens_params
        cots = [torch.as_tensor(c, dtype=torch.float32, device=self.device) for c in (cot_xx, cot_xy, cot_yx, cot_yy)]
        if cs != 1.0:
            cots = [cs * c for c in cots]
        return self._model.lens_hessian_vjp(packed, x, y, *cots)

    def reduced_shear(self, x, y, lens_params, deflection_scale=1.0):
        """Reduced shear ``(g1, g2)`` as a weak-lensing ellipticity estimates it (beyond the reference): ``g = gamma / (1 - kappa)``
        from ``shear`` and ``convergence`` where ``|g| <= 1``, and ``1 / g* = g / |g|^2`` where ``|g| > 1`` (continuous at
        ``|g| = 1``).  Forward only."""
        fxx, fxy, _, fyy = self._hessian(x, y, lens_params, deflection_scale)
        omk = 1.0 - 0.5 * (fxx + fyy)
        g1, g2 = 0.5 * (fxx - fyy) / omk, fxy / omk
        n2 = g1 * g1 + g2 * g2
        weak = n2 <= 1.0
        return torch.where(weak, g1, g1 / n2), torch.where(weak, g2, g2 / n2)

    def shear_log_like_and_grad(self, lens_params, catalogue, want_grad=True):
        """The weak-lensing likelihood of a ``model.ShearCatalogue`` (beyond the reference): with the reduced shear ``g^`` of
        ``reduced_shear`` at every galaxy, on the plane of the galaxy's own deflection scale,
        ``chi2 = sum [(e1 - g^1)^2 + (e2 - g^2)^2] / sigma^2`` and ``log_like = -1/2 (chi2 + 2 sum log(2 pi sigma^2))``.  Returns
        ``dict(log_like [B], chi2 [B], model_g [2, N, B], grad)``: ``grad`` is ``d log_like / d`` packed rows ``[B, P]`` (zero outside
        the lens-mass columns) through the kernels of ``hessian_vjp``, or None without ``want_grad``.  Deterministic; no host
        synchronisation.  ``UnsupportedLensError``: lens planes, series and user-written lenses."""
        self._single_plane("shear_log_like_and_grad")
        packed = self._lens_rows(lens_params)
        tabs = catalogue.device_tables(self.device)
        ll, chi2, model_g, grad = self._model.shear_loglike(packed.detach(), tabs["x"], tabs["y"], tabs["e1"], tabs["e2"], tabs["sigma"],
                                                            scales=tabs["scales"], want_grad=want_grad)
        return dict(log_like=ll, chi2=chi2, model_g=model_g, grad=grad)

    def image_plane_log_like_and_grad(self, lens_params, families, *, source_x=None, source_y=None, tol=None, max_iter=30,
                                      want_grad=True):
        """The image-plane position likelihood of a ``model.ImageFamilies`` (beyond the reference, whose position term is the
        source-plane linearisation; the refinement stage after a source-plane fit).  The source of family f is ``source_x/_y``
        ``[B, F]`` or, by default, the barycentre of its back-traced observed images (the source ``predicted_positions`` solves
        for; two or more images per family).  The predicted image of observed image j is the root of ``beta(theta) = beta_f`` that
        Newton reaches from ``theta_obs_j`` (the iteration of ``image_positions``; ``tol`` defaults to ``IMAGE_TOL_EPS eps32 max
        |coordinate|``), every step at most ``cap_j = families.max_shift[j]`` long.  It is LOST when Newton has not converged after
        ``max_iter`` steps, the point is not finite, it lies further than ``cap_j`` from ``theta_obs_j``, or the Jacobian of ``beta`` is singular there.
        ``chi2 = sum_j min(|theta_pred_j - theta_obs_j|^2, cap_j^2) / sigma_j^2`` (a lost image sits at the cap) and
        ``log_like = -chi2 / 2 - sum_j log(2 pi sigma_j^2)``: finite for every sample.

        Returns ``dict(log_like [B], chi2 [B], n_lost [B], predicted_x, predicted_y [B, J] (NaN where lost), lost [B, J], grad,
        grad_source_x, grad_source_y)``: ``grad`` is ``d log_like / d`` packed rows ``[B, P]`` (zero outside the lens-mass columns) by
        the implicit function theorem through the kernels of ``beta_vjp`` -- exact, a lost image contributes nothing -- and
        ``grad_source_x/_y`` ``[B, F]`` the gradient on explicit sources; None without ``want_grad`` (or without sources).
        Deterministic; no host synchronisation.  ``UnsupportedLensError``: lens planes, series and user-written lenses;
        ``NotImplementedError``: an input that requires a gradient (wrap the entry as ``model.ImagePlaneProbModel`` does)."""
        self._single_plane("image_plane_log_like_and_grad")
        packed = self._lens_rows(lens_params)
        if any(torch.is_tensor(t) and t.requires_grad for t in (packed, source_x, source_y)):
            raise NotImplementedError("image_plane_log_like_and_grad carries no autograd graph: its gradient is the returned grad")
        B = int(packed.shape[0])
        if (source_x is None) != (source_y is None):
            raise ValueError("source_x and source_y must both be given or both be None")
        source = None
        if source_x is None:
            if families.min_count < 2:
                raise ValueError("a family of one image has no barycentre source: give source_x / source_y")
        else:
            sx, sy = (torch.as_tensor(s, dtype=torch.float32, device=self.device) for s in (source_x, source_y))
            if tuple(sx.shape) != (B, families.F) or tuple(sy.shape) != (B, families.F):
                raise ValueError(f"source_x / source_y must have shape {(B, families.F)}, got {tuple(sx.shape)} and {tuple(sy.shape)}")
            source = torch.stack([sx, sy])
        if tol is None:
            tol = self.IMAGE_TOL_EPS * float(np.finfo(np.float32).eps) * families.max_coordinate
        tabs = families.device_tables(self.device)
        ll, chi2, n_lost, pred, grad, grad_src = self._model.imgplane_loglike(packed, tabs["image"], tabs["family"], families.offsets,
                                                                              source=source, tol=tol, max_iter=max_iter,
                                                                              want_grad=want_grad)
        px, py = pred[0].t(), pred[1].t()
        return dict(log_like=ll, chi2=chi2, n_lost=n_lost, predicted_x=px, predicted_y=py, lost=torch.isnan(px), grad=grad,
                    grad_source_x=None if grad_src is None else grad_src[0], grad_source_y=None if grad_src is None else grad_src[1])

    def _hessian(self, x, y, lens_params, deflection_scale):
        """``f_xx, f_xy, f_yx, f_yy`` of ``_lens_maps`` on the plane of ``deflection_scale`` (linear in it: ``c H``).  With lens
        planes: ``I - A_t`` of the target plane, which is not symmetric."""
        if self._mp is not None:
            return tuple(self._mp_maps("the lens maps", x, y, lens_params, deflection_scale)[2:])
        cs = self._scale(deflection_scale)
        h = self._lens_maps(x, y, lens_params)[2:]
        return tuple(h) if cs == 1.0 else tuple(cs * f for f in h)

    def magnification(self, x, y, lens_params: List[Dict], deflection_scale=1.0):
        """tf/simulator.py:80-91: ``1 / det(1 - Hessian)`` at ``(x, y)`` (trailing axis = batch)."""
        fxx, fxy, fyx, fyy = self._hessian(x, y, lens_params, deflection_scale)
        return 1.0 / ((1 - fxx) * (1 - fyy) - fxy * fyx)

    def convergence(self, x, y, lens_params: List[Dict], deflection_scale=1.0):
        """tf/simulator.py:93-98 (sum of the lenses' ``(f_xx + f_yy) / 2``, tf/profile.py:30-34)."""
        fxx, _, _, fyy = self._hessian(x, y, lens_params, deflection_scale)
        return 0.5 * (fxx + fyy)

    def shear(self, x, y, lens_params: List[Dict], deflection_scale=1.0):
        """tf/simulator.py:100-107: ``(gamma1, gamma2) = ((f_xx - f_yy)/2, f_xy)`` (tf/profile.py:36-42)."""
        fxx, fxy, _, fyy = self._hessian(x, y, lens_params, deflection_scale)
        return 0.5 * (fxx - fyy), fxy

    def rotation(self, x, y, lens_params: List[Dict], deflection_scale=1.0):
        """Rotation ``(A_xy - A_yx) / 2`` of the lensing Jacobian ``A = I - Hessian`` (beyond the reference): zero to rounding for one
        lens plane, where A is symmetric, and the signature of lens-lens coupling between several."""
        _, fxy, fyx, _ = self._hessian(x, y, lens_params, deflection_scale)
        return 0.5 * (fyx - fxy)

    # default Newton tolerance |beta(theta) - beta_s| of image_positions, in units of the float32 spacing at the window's largest
    # coordinate: beta = theta - alpha is a float32 difference of numbers of that size, so its rounding alone is a few ulp of it
    # (plus the rounding of alpha itself); 8 eps |theta|_max (8 to 16 ulp) is reached by every converging candidate, and is
    # still ~1e-6 arcsec on a 10-arcsec window.  A polishing step after convergence takes the point to the noise floor.
    IMAGE_TOL_EPS = 8.0

    def _source_rows(self, source_x, source_y, B):
        """Source positions as ``[B, S]`` float32 device tensors (scalars and ``[B]`` broadcast)."""
        sx = torch.as_tensor(source_x, dtype=torch.float32, device=self.device)
        sy = torch.as_tensor(source_y, dtype=torch.float32, device=self.device)
        if sx.dim() == 0:
            sx = sx.expand(B)
        if sy.dim() == 0:
            sy = sy.expand(B)
        if sx.dim() == 1:
            sx = sx.reshape(-1, 1)
        if sy.dim() == 1:
            sy = sy.reshape(-1, 1)
        sx, sy = torch.broadcast_tensors(sx, sy)
        if sx.dim() != 2 or sx.shape[0] != B:
            raise ValueError(f"source_x / source_y must have shape [B] or [B, S] with B = {B}, got {tuple(sx.shape)}")
        return sx, sy

    def _source_targets(self, source_redshifts, S, deflection_scale):
        """The ``source_redshifts`` keyword of ``image_positions``: ``(mp, [S, K] couplings)`` of the ``MultiPlane`` the model was
        built with -- row s is ``mp.target_scales(z_s)``."""
        if not (np.ndim(deflection_scale) == 0 and float(deflection_scale) == 1.0):
            raise ValueError("source_redshifts and deflection_scale are two ways to place the sources: give one")
        mp = self._mp if self._mp is not None else getattr(self.phys_model, "_multiplane_single", None)
        if mp is None:
            raise ValueError("source_redshifts needs a PhysicalModel built with a cosmology.MultiPlane (its planes turn the redshifts "
                             "into couplings); on a model without one, place the sources with deflection_scale")
        z = np.asarray(source_redshifts, dtype=np.float64)
        if z.ndim == 0:
            z = np.broadcast_to(z, (S,))
        if z.ndim != 1 or z.size != S:
            raise ValueError(f"source_redshifts: a scalar or one redshift per source ({S}), got shape {z.shape}")
        if not np.all(np.isfinite(z)) or np.any(z <= mp.z_planes[0]):
            raise ValueError(f"source_redshifts: every redshift must be finite and lie behind the first lens plane "
                             f"(z = {mp.z_planes[0]}), got {z.tolist()}")
        return mp, np.stack([mp.target_scales(zs) for zs in z], axis=0)

    def image_positions(self, lens_params, source_x, source_y, *, window=None, num_cells=None, max_images=8, tol=None,
                        max_iter=30, strict=False, deflection_scale=1.0, source_redshifts=None):
        """Solve the lens equation beta(theta) = beta_s for every sample (beyond the reference: it only maps theta -> beta).

        ``lens_params``: the ``lens_mass`` list of dicts, a nested dict with a ``lens_mass`` entry, or packed ``[B, P]`` rows.
        ``source_x`` / ``source_y``: ``[B]`` or ``[B, S]``.  ``window`` = ``(x_lo, x_hi, y_lo, y_hi)`` (default: the bounding box
        of the simulator's grid), searched on ``num_cells`` x ``num_cells`` cells (default ``2 * num_pix``).
        Returns ``x, y, mu`` ``[B, S, max_images]`` (images sorted by x then y, NaN-padded; ``mu`` is the signed
        magnification, the quantity ``magnification`` returns) and ``n`` ``[B, S]``.  Images that were found but could not be
        stored or refined (``max_images`` exceeded, Newton not converged, converged outside the window) warn, or raise
        ``RuntimeError`` with ``strict=True``.  ``deflection_scale``: a scalar, or one value per source ``[S]`` -- source s is solved
        on its own plane ``beta_s(theta) = theta - c_s sum alpha`` (``mu`` is that plane's magnification).  Forward only (no gradient).

        ``source_redshifts`` (instead of ``deflection_scale``; a model built with a ``cosmology.MultiPlane``): a scalar, or one
        redshift per source ``[S]``.  On two to four lens planes source s is traced through the planes in front of it,
        ``beta_s(theta) = theta - sum_i T_si a_i(theta)`` with ``T_s = MultiPlane.target_scales(z_s)`` (``gl_multiplane_image_positions``;
        ``mu`` is ``1 / det A`` of the full, non-symmetric Jacobian on that source's plane); such a model without
        ``source_redshifts`` raises ``UnsupportedLensError`` -- a source without a redshift names no plane.  On a one-plane
        ``MultiPlane`` the redshifts become the per-source ``deflection_scale``.  ``ValueError``: together with a
        ``deflection_scale``, a wrong count, a redshift that is not finite or not behind the first lens plane, a model without a
        ``MultiPlane``.

        The window is half-open for an image exactly ON its boundary: two of the four sides count, one of ``y_lo`` / ``y_hi`` and
        one of ``x_lo`` / ``x_hi`` -- those whose counter-clockwise direction, mapped by ``sign(det A) A`` (``A = I - H``), points
        upwards or exactly to the right; without a lens ``y = y_lo`` and ``x = x_hi``, the corner ``(x_hi, y_lo)`` included.  An
        image on the other two sides is neither returned nor counted.  Strictly inside, an image on a shared cell edge or
        vertex is found once."""
        if source_redshifts is None:
            self._single_plane("image_positions")
        if torch.is_tensor(lens_params):
            packed = lens_params
        elif isinstance(lens_params, dict):
            packed = self._pack_partial(lens_params)
        else:
            packed = self._pack_partial({"lens_mass": lens_params})
        if packed.requires_grad:
            raise NotImplementedError("image_positions is a forward-only diagnostic (no gradient)")
        B = packed.shape[0]
        sx, sy = self._source_rows(source_x, source_y, B)
        if window is None:
            window = (float(self.img_X.min()), float(self.img_X.max()), float(self.img_Y.min()), float(self.img_Y.max()))
        window = tuple(float(v) for v in window)
        if num_cells is None:
            num_cells = 2 * int(self.numPix)
        if tol is None:
            tol = self.IMAGE_TOL_EPS * float(np.finfo(np.float32).eps) * max(abs(v) for v in window)
        S = sx.shape[1]
        targets = None
        if source_redshifts is not None:
            mp, targets = self._source_targets(source_redshifts, S, deflection_scale)
            if mp.K == 1:  # one plane: the existing path on the sources' own scales
                deflection_scale, targets = targets[:, 0], None
        if targets is not None:
            out, n, dropped = self._model.multiplane_image_positions(packed, sx, sy, targets, window, int(num_cells), int(max_images),
                                                                     float(tol), int(max_iter))
        else:
            scales = np.asarray(deflection_scale, dtype=np.float32)
            scales = _native.deflection_scales(np.broadcast_to(scales, (S,)) if scales.ndim == 0 else scales, S, "deflection_scale")
            out, n, dropped = self._model.image_positions(packed, sx, sy, window, int(num_cells), int(max_images), float(tol),
                                                          int(max_iter), scales=scales if np.any(scales != 1.0) else None)
        n_drop = int(dropped.sum())
        if n_drop:
            msg = (f"image_positions: {n_drop} image(s) found but not returned over {int((dropped > 0).sum())} "
                   f"(sample, source) pair(s) (max_images={max_images} exceeded, Newton not converged, or converged outside "
                   f"the window)")
            if strict:
                raise RuntimeError(msg)
            warnings.warn(msg, RuntimeWarning, stacklevel=2)
        return out[..., 0], out[..., 1], out[..., 2], n

    def critical_curves(self, lens_params, *, window=None, num_cells=None, max_segments=None, strict=False, deflection_scale=1.0,
                        source_redshifts=None):
        """Critical curves (``det(I - H) = 0``) and caustics of every sample (beyond the reference), as line segments.

        ``lens_params`` as ``image_positions`` takes them.  ``window`` = ``(x_lo, x_hi, y_lo, y_hi)`` (default: the bounding box of
        the simulator's grid) is contoured on ``num_cells`` x ``num_cells`` cells (default ``2 * num_pix``) by marching squares;
        every endpoint is refined on its grid edge to float32 accuracy, the curve between two endpoints is a chord of a cell.
        Returns a dict: ``critical``, ``caustic`` ``[B, M, 2, 2]`` (segment, endpoint, x / y; the caustic holds ``beta`` at the same
        endpoints; NaN-padded; ``M = max_segments``, default ``8 * num_cells``), ``kind`` ``[B, M]`` (0 tangential, 1 radial,
        -1 padding), ``n`` ``[B]``, ``closed`` ``[B]`` (no curve reaches the window boundary, nothing dropped or flagged), and the
        enclosed areas ``area_tangential``, ``area_radial``, ``caustic_area_tangential``, ``caustic_area_radial`` ``[B]`` (NaN
        where not ``closed``; each the absolute value of the signed sum over all loops of its kind, i.e. the enclosed area when there
        is one loop of that kind; per-loop areas: ``chain_curves``).  Segments are oriented with ``det < 0`` on their left; ``chain_curves`` joins them into polylines.
        Segments beyond ``max_segments`` and cells skipped because a vertex is singular while its neighbours differ in sign warn,
        or raise ``RuntimeError`` with ``strict=True``.  Built-in kinds and dPIE-family catalogues; series expansions, user-written
        bodies and run-time compiled ScalingRelation member loops raise ``_native.UnsupportedLensError``.  ``deflection_scale``: the
        curves of the source plane with that scale, ``det(I - c H) = 0`` and ``beta = theta - c sum alpha``.  Forward only.

        ``source_redshifts`` (instead of ``deflection_scale``; a model built with a ``cosmology.MultiPlane``): a scalar returns the
        dict above for the source plane at that redshift; a sequence of S redshifts returns a list of S such dicts, views of one
        ``[B, S, ...]`` result of one native call.  On two to four lens planes the curves are ``det A_t = 0`` of the full,
        non-symmetric Jacobian ``A_t = d beta_t / d theta`` with ``beta_t = theta - sum_i T_si a_i(theta)``,
        ``T_s = MultiPlane.target_scales(z_s)`` (``gl_multiplane_critical_curves``): the caustic is ``beta_t``, a segment is
        tangential when ``tr A_t > 0``; ``closed``, the NaN areas, the warning and ``strict`` hold per (sample, source).  Such a model
        without ``source_redshifts`` raises ``UnsupportedLensError``.  On a one-plane ``MultiPlane`` every redshift becomes a
        ``deflection_scale`` (one single-plane call each).  ``ValueError``: as ``image_positions``."""
        if source_redshifts is None:
            self._single_plane("critical_curves")
        packed = self._lens_rows(lens_params)
        self._forward_only("critical_curves", packed)
        if source_redshifts is not None:
            return self._critical_curves_at(packed, source_redshifts, deflection_scale, window, num_cells, max_segments, strict)
        cs = self._scale(deflection_scale)
        if window is None:
            window = (float(self.img_X.min()), float(self.img_X.max()), float(self.img_Y.min()), float(self.img_Y.max()))
        window = tuple(float(v) for v in window)
        if num_cells is None:
            num_cells = 2 * int(self.numPix)
        if max_segments is None:
            max_segments = 8 * int(num_cells)
        seg, cau, kind, n, dropped, flagged, opened, area = self._model.critical_curves(packed, window, int(num_cells),
                                                                                         int(max_segments),
                                                                                         scale=None if cs == 1.0 else cs)
        return self._curves_result(seg, cau, kind, n, dropped, flagged, opened, area, max_segments, strict, "sample(s)", 3)

    @staticmethod
    def _curves_result(seg, cau, kind, n, dropped, flagged, opened, area, max_segments, strict, rows, stacklevel):
        """The dict of ``critical_curves`` from the native outputs, whose leading axes are ``[B]`` or ``[B, S]`` (``rows``: what one
        entry of them is called in the warning)."""
        n_drop, n_flag = int(dropped.sum()), int(flagged.sum())
        if n_drop or n_flag:
            msg = (f"critical_curves: {n_drop} segment(s) not returned over {int((dropped > 0).sum())} {rows} "
                   f"(max_segments={max_segments} exceeded), {n_flag} cell(s) skipped over {int((flagged > 0).sum())} {rows} "
                   f"(a singular vertex between vertices of different sign)")
            if strict:
                raise RuntimeError(msg)
            warnings.warn(msg, RuntimeWarning, stacklevel=stacklevel)
        closed = (opened == 0) & (dropped == 0) & (flagged == 0)
        area = torch.where(closed[..., None], area.abs(), torch.full_like(area, float("nan")))
        return {"critical": seg, "caustic": cau, "kind": kind, "n": n, "closed": closed,
                "area_tangential": area[..., 0], "area_radial": area[..., 1],
                "caustic_area_tangential": area[..., 2], "caustic_area_radial": area[..., 3]}

    def _critical_curves_at(self, packed, source_redshifts, deflection_scale, window, num_cells, max_segments, strict):
        """``critical_curves(source_redshifts=...)``: one dict for a scalar redshift, a list of dicts for a sequence."""
        scalar = np.ndim(source_redshifts) == 0
        S = 1 if scalar else int(np.size(source_redshifts))
        if S < 1:
            raise ValueError("source_redshifts: a scalar or a non-empty sequence of redshifts")
        mp, targets = self._source_targets(source_redshifts, S, deflection_scale)
        if mp.K == 1:  # one plane: the existing path on every source's own scale
            out = [self.critical_curves(packed, window=window, num_cells=num_cells, max_segments=max_segments, strict=strict,
                                        deflection_scale=float(c)) for c in targets[:, 0]]
            return out[0] if scalar else out
        if window is None:
            window = (float(self.img_X.min()), float(self.img_X.max()), float(self.img_Y.min()), float(self.img_Y.max()))
        window = tuple(float(v) for v in window)
        if num_cells is None:
            num_cells = 2 * int(self.numPix)
        if max_segments is None:
            max_segments = 8 * int(num_cells)
        native = self._model.multiplane_critical_curves(packed, targets, window, int(num_cells), int(max_segments))
        res = self._curves_result(*native, max_segments, strict, "(sample, source) pair(s)", 4)
        views = [{k: v[:, s] for k, v in res.items()} for s in range(S)]
        return views[0] if scalar else views

    def einstein_radius(self, lens_params, **kwargs):
        """Effective Einstein radius ``sqrt(A / pi)`` ``[B]`` of every sample (beyond the reference), ``A`` the area the tangential
        critical curve encloses (``critical_curves``, which takes ``kwargs``, ``deflection_scale`` among them).  NaN where the tangential curve is not closed inside
        the window or absent; such samples are counted in a ``RuntimeWarning``.  ``source_redshifts``: ``[B]`` for a scalar
        redshift, ``[B, S]`` for a sequence of S (one ``critical_curves`` call)."""
        res = self.critical_curves(lens_params, **kwargs)

        def radius(r):
            has_tangential = (r["kind"] == 0).any(dim=1)
            theta = torch.sqrt(r["area_tangential"] / math.pi)
            return torch.where(has_tangential, theta, torch.full_like(theta, float("nan")))
        theta = torch.stack([radius(r) for r in res], dim=1) if isinstance(res, list) else radius(res)
        n_bad = int(torch.isnan(theta).sum())
        if n_bad:
            rows = "(sample, source) pair(s)" if isinstance(res, list) else "sample(s)"
            warnings.warn(f"einstein_radius: the tangential critical curve is open or absent in {n_bad} of {theta.numel()} {rows}",
                          RuntimeWarning, stacklevel=2)
        return theta

    @staticmethod
    def chain_curves(result, b):
        """Join the segments of sample ``b`` of a ``critical_curves`` result into ordered polylines (host side, numpy).  Returns a list
        of ``(kind, closed, xy[K, 2], beta[K, 2])`` in the order of each chain's first segment: ``xy`` the image-plane points along
        the curve (the first point is not repeated at the end of a closed one), ``beta`` the caustic at the same points, ``kind``
        that of the chain's first segment.  Endpoints shared by two segments are bitwise equal, so they are matched exactly."""
        n = int(result["n"][b])
        seg = np.asarray(result["critical"][b, :n].cpu() if torch.is_tensor(result["critical"]) else result["critical"][b, :n])
        cau = np.asarray(result["caustic"][b, :n].cpu() if torch.is_tensor(result["caustic"]) else result["caustic"][b, :n])
        kind = np.asarray(result["kind"][b, :n].cpu() if torch.is_tensor(result["kind"]) else result["kind"][b, :n])
        live = [i for i in range(n) if kind[i] >= 0]
        key = lambda p: (float(p[0]), float(p[1]))
        at = {}  # point -> [(segment, which end)]
        for i in live:
            for e in (0, 1):
                at.setdefault(key(seg[i, e]), []).append((i, e))
        used = set()

        def walk(i, e):
            """Follow the chain out of end ``e`` of segment ``i``; returns the (segment, entered-at end) pairs visited."""
            out = []
            while True:
                nxt = [(j, f) for j, f in at[key(seg[i, e])] if j != i and j not in used]
                if not nxt:
                    return out
                j, f = nxt[0]
                used.add(j)
                out.append((j, f))
                i, e = j, 1 - f
        chains = []
        for i in live:
            if i in used:
                continue
            used.add(i)
            fwd = walk(i, 1)
            closed = bool(fwd) and key(seg[fwd[-1][0], 1 - fwd[-1][1]]) == key(seg[i, 0])
            back = [] if closed else walk(i, 0)
            # points: backwards chain reversed (far ends first), the seed segment, the forward chain's far ends
            pts = [(j, 1 - f) for j, f in reversed(back)] + [(i, 0), (i, 1)] + [(j, 1 - f) for j, f in fwd]
            if closed:
                pts = pts[:-1]
            xy = np.array([seg[j, e] for j, e in pts], dtype=seg.dtype).reshape(-1, 2)
            beta = np.array([cau[j, e] for j, e in pts], dtype=cau.dtype).reshape(-1, 2)
            chains.append((int(kind[i]), closed, xy, beta))
        return chains

    def _potential_lenses(self):
        """The lensing-potential calls serve built-in kinds and fused catalogues; refuse the rest with a typed error up front."""
        for i, lens in enumerate(self.phys_model.lenses):
            kind = getattr(lens, "_kind", 0)
            if kind == 10:
                raise _native.UnsupportedLensError(f"lens {i} ({lens.name}): a series expansion stores its deflection on the pixel "
                                                   "grid only, no potential")
            if kind == _native.GL_INTERPOL_MASS:
                raise _native.UnsupportedLensError(f"lens {i} ({lens.name}): deflection maps carry no potential")
            if not kind and getattr(lens, "profile", None) is not None and getattr(lens, "scaling_params", None) is not None:
                raise _native.UnsupportedLensError(f"lens {i} ({lens.name}): a ScalingRelation compiled at run time as a member loop "
                                                   "(base profile outside the dPIE family) defines a deflection only, no potential")
            if not kind:
                raise _native.UnsupportedLensError(f"lens {i} ({lens.name}): a user-written body defines a deflection only, "
                                                   "no potential")

    def _forward_only(self, what, *tensors):
        if any(torch.is_tensor(t) and t.requires_grad for t in tensors):
            raise NotImplementedError(f"{what} is a forward-only diagnostic (no gradient)")

    def _lens_rows(self, lens_params):
        if torch.is_tensor(lens_params):
            return lens_params
        if isinstance(lens_params, dict):
            return self._pack_partial(lens_params)
        return self._pack_partial({"lens_mass": lens_params})

    def potential(self, x, y, lens_params):
        """Lensing potential ``psi`` summed over the lenses at ``(x, y)`` (beyond the reference; trailing axis = batch, as
        ``convergence``): the potential whose gradient is the deflection ``beta`` subtracts.  Each kind's additive constant is
        fixed (zero at its centre), so only differences are physical.  Built-in kinds and dPIE-family catalogues; series
        expansions, user-written bodies and run-time compiled ScalingRelation member loops raise
        ``_native.UnsupportedLensError``.  Forward only."""
        self._single_plane("potential")
        packed = self._lens_rows(lens_params)
        self._forward_only("potential", packed, x, y)
        self._potential_lenses()
        return self._model.lens_potential(packed, x, y)

    def _delay_weights(self, source_redshifts, S):
        """``(mp, targets [S, K], geom [S, K], pot [K])`` of sources at ``source_redshifts`` (a scalar or ``[S]``): the couplings of
        ``_source_targets`` and the arrival-time weights ``MultiPlane.delay_weights`` (float64).  ``pot`` is a constant of the plane:
        every source's row holds it for the planes in front of that source, so the largest over the rows is the plane's."""
        mp, targets = self._source_targets(source_redshifts, S, 1.0)
        z = np.broadcast_to(np.asarray(source_redshifts, dtype=np.float64), (S,))
        weights = [mp.delay_weights(zs) for zs in z]
        return mp, targets, np.stack([w[0] for w in weights], axis=0), np.max(np.stack([w[1] for w in weights], axis=0), axis=0)

    def fermat_potential(self, x, y, source_x, source_y, lens_params, *, source_redshift=None):
        """Fermat potential ``phi = |theta - beta_s|^2 / 2 - psi(theta)`` at ``theta = (x, y)`` for the source ``beta_s`` (beyond the
        reference; arcsec^2).  ``source_x`` / ``source_y`` broadcast against ``x``, ``y`` (trailing axis = batch).  Forward only.

        ``source_redshift`` (a model built with a ``cosmology.MultiPlane``): the arrival time ``T`` of the ray from ``theta`` to a source
        at that redshift, through the lens planes in front of it (``gl_multiplane_fermat``, the formula of
        ``MultiPlane.delay_weights``), in arcsec^2 times ``c / H0`` and in float64.  On one plane ``T = geom_0 (|theta - beta_s|^2 / 2 -
        c psi)`` with the source's ``deflection_scale`` c.  A model with lens planes serves this form alone: without a redshift
        it raises ``UnsupportedLensError``."""
        self._forward_only("fermat_potential", source_x, source_y)
        if source_redshift is None:
            psi = self.potential(x, y, lens_params)
            x = torch.as_tensor(x, dtype=torch.float32, device=self.device)
            y = torch.as_tensor(y, dtype=torch.float32, device=self.device)
            sx = torch.as_tensor(source_x, dtype=torch.float32, device=self.device)
            sy = torch.as_tensor(source_y, dtype=torch.float32, device=self.device)
            return 0.5 * ((x - sx) ** 2 + (y - sy) ** 2) - psi
        if np.ndim(source_redshift) != 0:
            raise ValueError(f"source_redshift: one redshift, got shape {np.shape(source_redshift)}")
        packed = self._lens_rows(lens_params)
        self._forward_only("fermat_potential", packed, x, y)
        self._potential_lenses()
        mp, targets, geom, pot = self._delay_weights(source_redshift, 1)
        B = packed.shape[0]
        x, y, sx, sy = torch.broadcast_tensors(*(torch.as_tensor(v, dtype=torch.float32, device=self.device)
                                                 for v in (x, y, source_x, source_y)))
        if x.dim() == 0 or x.shape[-1] not in (1, B):
            raise ValueError(f"x, y and the source must broadcast to (..., B = {B}), got {tuple(x.shape)}")
        shape = tuple(x.shape[:-1]) + (B,)
        x, y, sx, sy = (v.expand(shape).reshape(-1, B).t().contiguous() for v in (x, y, sx, sy))  # [B, N]
        if mp.K == 1:  # one plane: the source's own scale on the single-plane potential
            psi = self._model.lens_potential(packed, x.t(), y.t()).t()
            phi = 0.5 * ((x.double() - sx.double()) ** 2 + (y.double() - sy.double()) ** 2) - float(targets[0, 0]) * psi.double()
            T = phi * float(geom[0, 0])
        else:  # every point is the one image of a source of its own
            N = x.shape[1]
            T = self._model.multiplane_fermat(packed, x[..., None], y[..., None], sx, sy, np.repeat(geom, N, axis=0), pot)[..., 0]
        return T.t().reshape(shape)

    # D_dt / c * (1 arcsec)^2 in days per Mpc: the time-delay distance turns a Fermat-potential difference in arcsec^2 into a delay
    # (IAU 2012 astronomical unit -> parsec -> Mpc, c exact, 1 day = 86400 s)
    MPC_M = 648000.0 / np.pi * 149597870700.0 * 1e6
    DAYS_PER_MPC_ARCSEC2 = MPC_M / 299792458.0 * (np.pi / 648000.0) ** 2 / 86400.0

    def time_delays(self, lens_params, source_x, source_y, *, source_redshifts=None, h0=None, time_delay_distance=None,
                    **solver_kwargs):
        """Images of the sources and their arrival times for every sample (beyond the reference).

        Calls ``image_positions`` (``solver_kwargs`` go there) and returns its ``x, y, mu, n`` plus ``dt`` ``[B, S, max_images]``:
        the arrival time of every image relative to the first-arriving image of its (sample, source), i.e. its Fermat-potential
        excess ``phi - min phi`` (``dt >= 0``; NaN where ``x`` is NaN).  Units: arcsec^2, or days when ``time_delay_distance``
        (D_dt in Mpc, a scalar or ``[B]``) is given: ``dt * D_dt * DAYS_PER_MPC_ARCSEC2``.  Forward only.

        ``source_redshifts`` (a model built with a ``cosmology.MultiPlane``; a scalar or one redshift per source): the images come
        from ``image_positions(source_redshifts=...)`` and ``dt = T - min T`` with the arrival time ``T`` of the ray through the lens
        planes in front of each source (``gl_multiplane_fermat``; float64 on the device, cast to float32 last).  Units: arcsec^2
        times ``c / H0`` -- the weights are comoving distances in that unit --, or days with ``h0`` (km/s/Mpc, a scalar or ``[B]``):
        ``dt * cosmology.hubble_distance_mpc(h0) * DAYS_PER_MPC_ARCSEC2``.  On a one-plane ``MultiPlane`` source s is solved with its
        ``deflection_scale`` c_s and ``T = geom_s0 (|theta - beta_s|^2 / 2 - c_s psi)``.  A model with lens planes needs the
        redshifts (``UnsupportedLensError`` without).  ``ValueError``: ``time_delay_distance`` together with ``source_redshifts`` (on
        planes there is no single distance), ``h0`` without ``source_redshifts``."""
        if source_redshifts is not None and time_delay_distance is not None:
            raise ValueError("time_delay_distance and source_redshifts: with redshifts every plane brings a distance of its own; give "
                             "h0 for days")
        if source_redshifts is None and h0 is not None:
            raise ValueError("h0 turns the arrival times of sources with redshifts into days: give source_redshifts (or, without "
                             "redshifts, time_delay_distance)")
        if source_redshifts is None:
            self._single_plane("time_delays")
        packed = self._lens_rows(lens_params)
        self._forward_only("time_delays", packed, source_x, source_y)
        self._potential_lenses()
        B = packed.shape[0]
        sx, sy = self._source_rows(source_x, source_y, B)                   # [B, S]
        if source_redshifts is not None:
            if h0 is not None:
                from gigalens_amd.cosmology import hubble_distance_mpc
                time_delay_distance = hubble_distance_mpc(h0.detach().cpu().numpy() if torch.is_tensor(h0) else h0)
            mp, targets, geom, pot = self._delay_weights(source_redshifts, sx.shape[1])
            solver_kwargs = dict(solver_kwargs, source_redshifts=source_redshifts)
        x, y, mu, n = self.image_positions(packed, source_x, source_y, **solver_kwargs)
        ok = ~torch.isnan(x)
        if source_redshifts is not None and mp.K >= 2:
            phi = self._model.multiplane_fermat(packed, x, y, sx, sy, geom, pot)  # [B, S, M] float64; NaN where x is
        else:
            xs, ys = torch.where(ok, x, torch.zeros_like(x)), torch.where(ok, y, torch.zeros_like(y))
            psi = self._model.lens_potential(packed, xs.permute(1, 2, 0), ys.permute(1, 2, 0)).permute(2, 0, 1).double()  # [B, S, M]
            if source_redshifts is not None:  # one plane: the sources' own scales, and the weight in place of D_dt
                psi = psi * torch.as_tensor(targets[:, 0], dtype=torch.float64, device=self.device)[None, :, None]
            phi = 0.5 * ((xs.double() - sx[..., None].double()) ** 2 + (ys.double() - sy[..., None].double()) ** 2) - psi
            if source_redshifts is not None:
                phi = phi * torch.as_tensor(geom[:, 0], dtype=torch.float64, device=self.device)[None, :, None]
        phi = torch.where(ok, phi, torch.full_like(phi, float("inf")))
        dt = phi - phi.amin(dim=2, keepdim=True)
        if time_delay_distance is not None:
            dd = torch.as_tensor(time_delay_distance, dtype=torch.float64, device=self.device).reshape(-1, 1, 1)
            dt = dt * dd * self.DAYS_PER_MPC_ARCSEC2
        dt = torch.where(ok, dt, torch.full_like(dt, float("nan"))).to(torch.float32)
        return x, y, mu, n, dt

    REGULARIZATIONS = {"identity": 0, "gradient": 1, "curvature": 2}
    MAX_SOURCE_NODES = 1024

    @staticmethod
    def log_det_regularization(regularization, n_src):
        """``log det R`` of the regularisation of ``reconstruct_source`` on a ``(ny, nx)`` grid, in float64 from the closed-form
        eigenvalues ``2 - 2 cos(k pi / (n + 1))`` of ``T_n = tridiag(-1, 2, -1)``: ``identity`` 0, ``gradient`` the sum of
        ``log(e_x + e_y)``, ``curvature`` of ``log(e_x^2 + e_y^2)``."""
        if regularization not in LensSimulator.REGULARIZATIONS:
            raise ValueError(f"regularization must be one of {sorted(LensSimulator.REGULARIZATIONS)}, got {regularization!r}")
        ny, nx = (int(v) for v in n_src)
        if regularization == "identity":
            return 0.0
        ex = 2.0 - 2.0 * np.cos(np.arange(1, nx + 1, dtype=np.float64) * np.pi / (nx + 1))
        ey = 2.0 - 2.0 * np.cos(np.arange(1, ny + 1, dtype=np.float64) * np.pi / (ny + 1))
        if regularization == "curvature":
            ex, ey = ex * ex, ey * ey
        return float(np.sum(np.log(ey[:, None] + ex[None, :])))

    def _per_sample(self, value, B, what, positive):
        """A scalar or ``[B]`` keyword as a float32 ``[B]`` host array (``ValueError`` unless finite, and > 0 when ``positive``)."""
        self._forward_only("reconstruct_source", value)
        arr = np.asarray(value.detach().cpu() if torch.is_tensor(value) else value, dtype=np.float64)
        if arr.size == 1:
            arr = arr.reshape(())
        if arr.ndim > 1 or (arr.ndim == 1 and arr.size != B):
            raise ValueError(f"{what}: expected a scalar or [B={B}], got shape {tuple(arr.shape)}")
        arr = np.broadcast_to(arr, (B,))
        if not np.all(np.isfinite(arr)) or (positive and not np.all(arr > 0)):
            raise ValueError(f"{what}: every value must be finite{' and > 0' if positive else ''}, got {arr.tolist()}")
        return arr.astype(np.float32)

    def reconstruct_source(self, params, observed_image, err_map, *, n_src, pitch, center=(0.0, 0.0), regularization="gradient",
                           strength=1.0, mask=None, deflection_scale=1.0):
        """Pixelated source reconstruction with the Bayesian evidence of every sample (beyond the reference): the most probable
        source on a regular grid given the lens model (semi-linear inversion, Warren & Dye 2003) and the evidence that ranks lens
        models and regularisation strengths (Suyu et al. 2006, eq. 19).

        ``params``: the nested dict or packed ``[B, P]`` rows; lenses and lens light are used, the model's ``source_light`` is ignored
        (the grid replaces it).  ``observed_image`` and ``err_map``: ``[H, W]`` (or ``[B, H, W]``, one per sample).  ``n_src = (ny, nx)``,
        ``pitch`` and ``center = (cx, cy)`` (scalars or ``[B]``) define the source grid: node ``(j, i)`` lies at ``(cx + (i - (nx-1)/2)
        pitch, cy + (j - (ny-1)/2) pitch)``, the pose of ``Interpolated(order=1)`` with ``phi = 0``, ``scale = pitch``; the source is zero
        outside the grid.  ``regularization``: ``"identity"``, ``"gradient"`` or ``"curvature"``; ``strength`` (lambda): a scalar, ``[B]``
        or ``[B, L]`` -- a scan over ``L`` strengths reuses the normal matrix of a sample.  ``mask``: ``[H, W]`` bool, combined with the
        simulator's ``pix_region``; the fit uses the pixels that remain.  ``deflection_scale``: the source plane, as on ``beta``.

        Returns a dict (an ``L`` axis follows ``B`` where ``strength`` is 2-D): ``source`` ``[B, ny, nx]``; ``model_image`` ``[B, H, W]``
        (lens light + ``F s`` on the used pixels, the lens light alone elsewhere); ``chi2``, ``reg`` (``s^T R s``), ``log_det``
        (``log det(A0 + lambda R)``) and ``log_evidence`` ``[B]`` (float64); ``ok`` ``[B]`` bool -- false where a Cholesky pivot is not
        finite or not positive, and the sample's other outputs are then NaN.  ``ValueError`` for ``ny nx > 1024``, a ``strength`` or
        ``pitch`` that is not finite or not > 0, an ``err_map`` that is not finite or not > 0 on a used pixel, an unknown
        ``regularization`` and shapes that do not match; lens kinds ``lens_maps`` refuses stay refused with its error.  Forward only."""
        p = self._pixsrc_prepare("reconstruct_source", params, observed_image, err_map, n_src, pitch, center, regularization, strength,
                                 mask, deflection_scale)
        source, image, scal, ok = self._model.pixsrc_reconstruct(p["bx"], p["by"], p["obs_u"], p["sig_u"], p["lens_light"], p["pix"],
                                                                 p["n_src"], p["pose"], self.REGULARIZATIONS[regularization], p["lam_t"])
        out = self._pixsrc_outputs(p, regularization, source, image, scal, ok)
        return out if p["scan"] else {k: v[:, 0] for k, v in out.items()}

    def _pixsrc_outputs(self, p, regularization, source, image, scal, ok):
        """The result dict of the pixelated-source calls from the native outputs (an ``L`` axis after ``B`` on every entry)."""
        ny, nx = p["n_src"]
        S = ny * nx
        chi2, reg, log_det = scal[..., 0], scal[..., 1], scal[..., 2]
        lam64 = p["lam_t"].double()
        noise = torch.log(2.0 * math.pi * p["sig_u"].double() ** 2).sum(dim=1, keepdim=True)
        log_ev = (-0.5 * chi2 - 0.5 * lam64 * reg - 0.5 * log_det + 0.5 * S * torch.log(lam64)
                  + 0.5 * self.log_det_regularization(regularization, (ny, nx)) - 0.5 * noise)
        return {"source": source, "model_image": image, "chi2": chi2, "reg": reg, "log_det": log_det, "log_evidence": log_ev,
                "ok": ok != 0}

    def _pixsrc_prepare(self, what, params, observed_image, err_map, n_src, pitch, center, regularization, strength, mask,
                        deflection_scale):
        """Validation and input preparation the pixelated-source calls share: the used pixels, data and rms on them, the rays of
        the whole supersampled frame, the lens-light image, pose and strengths, all on the device."""
        self._single_plane(what)
        if regularization not in self.REGULARIZATIONS:
            raise ValueError(f"regularization must be one of {sorted(self.REGULARIZATIONS)}, got {regularization!r}")
        ny, nx = (int(v) for v in n_src)
        if ny < 1 or nx < 1 or ny * nx > self.MAX_SOURCE_NODES:
            raise ValueError(f"n_src = ({ny}, {nx}): the source grid must have 1 .. {self.MAX_SOURCE_NODES} nodes")
        packed = self._pack_partial(params)
        self._forward_only(what, packed, observed_image, err_map, strength)
        B = packed.shape[0]
        H, W = self._model.out_h, self._model.out_w
        ss, dev = self.supersample, self.device
        cs = self._scale(deflection_scale)
        pitch_h = self._per_sample(pitch, B, "pitch", True)
        if len(center) != 2:
            raise ValueError("center must be (cx, cy)")
        cx_h, cy_h = self._per_sample(center[0], B, "center[0]", False), self._per_sample(center[1], B, "center[1]", False)
        lam = np.asarray(strength.detach().cpu() if torch.is_tensor(strength) else strength, dtype=np.float64)
        scan = lam.ndim == 2
        if lam.ndim > 2 or (lam.ndim >= 1 and lam.shape[0] != B) or lam.size == 0:
            raise ValueError(f"strength: expected a scalar, [B={B}] or [B, L], got shape {tuple(lam.shape)}")
        lam = np.broadcast_to(lam.reshape(-1, 1) if lam.ndim == 1 else lam, (B, lam.shape[1] if scan else 1)).astype(np.float32)
        if not (np.all(np.isfinite(lam)) and np.all(lam > 0)):
            raise ValueError("strength: every value must be finite and > 0 (as float32)")
        used = np.asarray(self.img_region.cpu()) != 0
        if mask is not None:
            mk = np.asarray(mask.cpu() if torch.is_tensor(mask) else mask)
            if mk.shape != (H, W):
                raise ValueError(f"mask must be [{H}, {W}], got {tuple(mk.shape)}")
            used = used & mk.astype(bool)
        pix = np.flatnonzero(used.reshape(-1)).astype(np.int32)
        if pix.size == 0:
            raise ValueError("no pixel is left to fit (mask and pix_region)")

        def per_pixel(a, what):
            t = torch.as_tensor(a, dtype=torch.float32, device=dev)
            if tuple(t.shape) not in ((H, W), (B, H, W)):
                raise ValueError(f"{what} must be [{H}, {W}] or [{B}, {H}, {W}], got {tuple(t.shape)}")
            return t.reshape(-1, H * W)[:, torch.from_numpy(pix.astype(np.int64)).to(dev)].expand(B, pix.size).contiguous()
        obs_u, sig_u = per_pixel(observed_image, "observed_image"), per_pixel(err_map, "err_map")
        if not bool((torch.isfinite(sig_u) & (sig_u > 0)).all()):
            raise ValueError("err_map must be finite and > 0 on every used pixel")
        # ray shooting on the whole supersampled frame (gl_lens_maps); pixels outside pix_region are not rendered by the simulator:
        # a NaN there gives them a row of zeros
        Hs, Ws = H * ss, W * ss
        cc, rr = np.meshgrid(np.arange(Ws), np.arange(Hs))
        gx, gy = self.wcs.pix2angle(cc.reshape(-1), rr.reshape(-1))
        gx_t, gy_t = torch.from_numpy(gx).to(dev), torch.from_numpy(gy).to(dev)
        maps = self._lens_maps(gx_t.reshape(-1, 1), gy_t.reshape(-1, 1), packed)
        bx, by = maps[0].reshape(Hs * Ws, B), maps[1].reshape(Hs * Ws, B)
        if cs != 1.0:
            bx, by = gx_t[:, None] + cs * (bx - gx_t[:, None]), gy_t[:, None] + cs * (by - gy_t[:, None])
        bx, by = bx.t().contiguous(), by.t().contiguous()
        if self._region_np.shape[0] != Hs * Ws:
            outside = torch.ones(Hs * Ws, dtype=torch.bool, device=dev)
            outside[self.region[:, 0] * Ws + self.region[:, 1]] = False
            bx[:, outside] = float("nan")
            by[:, outside] = float("nan")
        lens_light = self._model.simulate_parts(packed, 2) if len(self.phys_model.lens_light) else None
        pose = torch.from_numpy(np.stack([pitch_h, cx_h, cy_h], axis=1)).to(dev)
        lam_t = torch.from_numpy(np.ascontiguousarray(lam)).to(dev)
        return {"packed": packed, "B": B, "n_src": (ny, nx), "scan": scan, "cs": cs, "pix": torch.from_numpy(pix).to(dev), "obs_u": obs_u,
                "sig_u": sig_u, "gx": gx_t, "gy": gy_t, "bx": bx, "by": by, "lens_light": lens_light, "pose": pose, "lam_t": lam_t}

    def source_evidence_and_grad(self, params, observed_image, err_map, *, n_src, pitch, center=(0.0, 0.0), regularization="gradient",
                                 strength=1.0, mask=None, deflection_scale=1.0):
        """``reconstruct_source`` for one strength per sample (``strength``: a scalar or ``[B]``; 2-D raises ``ValueError``) with the
        gradient of the evidence.  Returns the dict of ``reconstruct_source`` plus ``grad`` ``[B, P]`` (float32, packed order:
        d log_evidence / d lens-mass parameters through the rays, d / d lens-light parameters through the lens-light image, 0 in
        the source-light columns), ``grad_pose`` ``[B, 3]`` = d / d(pitch, cx, cy) and ``grad_beta`` ``[2, B, Hs Ws]`` (d / d beta_x,
        beta_y of every supersampled pixel).  The gradient is that of the evidence with the set of finite rays held fixed; the
        evidence is continuous but only piecewise smooth in the lens: it has a kink wherever a ray crosses a source-grid line.
        Rows with ``ok == False`` are NaN.  Deterministic.  Inputs must not require a gradient (``model.SourceEvidenceProbModel``
        is the autograd entry); lens planes, series and user-written lenses raise ``UnsupportedLensError``."""
        if np.ndim(strength.detach().cpu() if torch.is_tensor(strength) else strength) > 1:
            raise ValueError("source_evidence_and_grad: strength must be a scalar or [B] (one strength per sample, no scan)")
        p = self._pixsrc_prepare("source_evidence_and_grad", params, observed_image, err_map, n_src, pitch, center, regularization,
                                 strength, mask, deflection_scale)
        packed, B = p["packed"], p["B"]
        source, image, scal, ok, gb, gimg = self._model.pixsrc_evidence_grad(
            p["bx"], p["by"], p["obs_u"], p["sig_u"], p["lens_light"], p["pix"], p["n_src"], p["pose"],
            self.REGULARIZATIONS[regularization], p["lam_t"][:, 0].contiguous())
        out = self._pixsrc_outputs(p, regularization, source[:, None], image[:, None], scal[:, None], ok[:, None])
        out = {k: v[:, 0] for k, v in out.items()}
        good = out["ok"]
        # lens mass: the VJP of the ray-shoot with the ray cotangents (rays with a row of zeros carry an exact 0 and are skipped)
        grad = self.beta_vjp(p["gx"].reshape(-1, 1), p["gy"].reshape(-1, 1), packed, gb[0].t(), gb[1].t(), deflection_scale=p["cs"])
        if p["lens_light"] is not None:  # lens light: the VJP of the render, its lens-light columns alone
            g_img = self._model.simulate_bwd(packed, torch.where(good[:, None, None], gimg, torch.zeros_like(gimg)))
            cols = torch.tensor([k for k, slot in enumerate(self._layout.slots) if slot[0] == "lens_light"], dtype=torch.long,
                                device=self.device)
            grad[:, cols] = g_img[:, cols]
        # pose: u = (beta_x - cx) / pitch + const, so d/dcx = -sum g_x, d/dpitch = -sum (g_x (beta_x - cx) + g_y (beta_y - cy)) / pitch
        gx64, gy64 = gb[0].double(), gb[1].double()
        pitch64, cx64, cy64 = (p["pose"][:, k:k + 1].double() for k in range(3))
        zero = torch.zeros((), dtype=torch.float64, device=self.device)
        tx = torch.where(gx64 != 0, gx64 * (p["bx"].double() - cx64), zero)
        ty = torch.where(gy64 != 0, gy64 * (p["by"].double() - cy64), zero)
        grad_pose = torch.stack([-(tx + ty).sum(dim=1) / pitch64[:, 0], -gx64.sum(dim=1), -gy64.sum(dim=1)], dim=1)
        nan = float("nan")
        out["grad"] = torch.where(good[:, None], grad, torch.full_like(grad, nan))
        out["grad_pose"] = torch.where(good[:, None], grad_pose, torch.full_like(grad_pose, nan))
        out["grad_beta"] = gb
        return out

    # -- point images in the pixel likelihood (gl_ptimg_*; beyond the reference) ---------------------------------------
    MAX_POINT_IMAGES = 8

    def _point_transform(self):
        """``(x0, y0, m00, m01, m10, m11)``: a position in arcsec -> supersampled pixel coordinates, ``(u, v) = M (x - x0, y - y0)``
        with ``u`` along the columns: ``supersample * wcs.angle2pix``, the inverse of ``wcs.pix2angle`` on the supersampled grid
        (``M = supersample inv(T^T)``, the ``T`` / ``T^T`` quirk of ``LensWCS`` kept)."""
        m = self.supersample * self.wcs.transform_angle2pix.T
        x0, y0 = self.wcs.radec_at_xy_0
        return (float(x0), float(y0), float(m[0, 0]), float(m[0, 1]), float(m[1, 0]), float(m[1, 1]))

    def _point_rows(self, what, *rows):
        """``[B, J]`` float32 device tensors of one shape (``ValueError`` otherwise, or for ``J`` outside ``1..MAX_POINT_IMAGES``)."""
        out = [torch.as_tensor(r, dtype=torch.float32, device=self.device) for r in rows]
        shape = tuple(out[0].shape)
        if len(shape) != 2 or any(tuple(t.shape) != shape for t in out):
            raise ValueError(f"{what}: x, y (and amplitude) must be [B, J] of one shape, got {[tuple(t.shape) for t in out]}")
        if not 1 <= shape[1] <= self.MAX_POINT_IMAGES:
            raise ValueError(f"{what}: {shape[1]} images per sample (1..{self.MAX_POINT_IMAGES})")
        if shape[0] < 1:
            raise ValueError(f"{what}: an empty batch")
        return out

    def point_images(self, x, y, amplitude):
        """The image of ``J`` point sources per sample seen through the PSF (beyond the reference): ``x, y`` in arcsec and
        ``amplitude`` (flux in image counts), ``[B, J]`` each -> ``[B, H, W]`` = ``sum_j amplitude_j D(x_j, y_j)``.

        The unit point image ``D(x, y)``: with ``(u, v) = supersample * wcs.angle2pix(x, y)`` the position on the supersampled grid,
        Keys' cubic weights (``a = -1/2``) of the 4 x 4 nodes around it on a zero supersampled frame (nodes outside the frame are
        dropped), the PSF applied as ``simulate`` applies it (``[[1]]`` without one), then the **sum** over ``supersample`` x
        ``supersample`` sub-pixels, without the ``det T`` factor.  ``sum(D) = sum(psf)`` while the footprint lies inside the frame;
        ``D`` is C1 in ``(x, y)`` and, the cubic weights being negative between one and two nodes from the position, has negative
        lobes: 5e-3 of its peak behind a PSF with sigma = 1.6 nodes, more behind a narrower one, up to 1/9 with none.  A position that is not finite, or whose footprint misses the frame, gives ``D = 0`` and a
        zero gradient.  ``pix_region`` does not apply (the fit uses it).  Differentiable in all three arguments (HIP kernels both
        ways); lens planes raise ``UnsupportedLensError``."""
        self._single_plane("point_images")
        x, y, amplitude = self._point_rows("point_images", x, y, amplitude)
        return _PointImagesFn.apply(x, y, amplitude, self._model, self._point_transform())

    def _point_prepare(self, what, params, x, y, observed_image, err_map, mask):
        """Validation and inputs the point-image fits share: positions, the extended image, data and weights on the device."""
        self._single_plane(what)
        packed = params if torch.is_tensor(params) else self.pack(params)
        x, y = self._point_rows(what, x, y)
        self._forward_only(what, packed, x, y, observed_image, err_map)
        B = packed.shape[0]
        if x.shape[0] != B:
            raise ValueError(f"{what}: x, y must be [B={B}, J], got {tuple(x.shape)}")
        data = self._point_data(B, observed_image, err_map, mask)
        return {"packed": packed, "x": x, "y": y, "extended": self._model.simulate_fwd(packed), **data}

    def _point_data(self, B, observed_image, err_map, mask):
        """The data side of a point-image fit, checked: ``obs``, ``weight`` (``1 / err_map^2`` on the used pixels, 0 elsewhere) and
        ``noise`` (``sum_U log(2 pi err^2)``, float64).  The checks read the device; for device tensors that were not written to since
        the last call (a probabilistic model's data, step after step) the result of that call is handed back."""
        given = (observed_image, err_map, mask)
        key = None
        if all(t is None or (torch.is_tensor(t) and t.device == self.device) for t in given):
            key = (B,) + tuple(None if t is None else (id(t), t._version) for t in given)
            if self._point_cache is not None and self._point_cache[0] == key:
                return self._point_cache[2]
        H, W = self._model.out_h, self._model.out_w
        dev = self.device
        used = self.img_region != 0
        if mask is not None:
            mk = torch.as_tensor(mask, device=dev)
            if tuple(mk.shape) != (H, W):
                raise ValueError(f"mask must be [{H}, {W}], got {tuple(mk.shape)}")
            used = used & mk.bool()
        if not bool(used.any()):
            raise ValueError("no pixel is left to fit (mask and pix_region)")

        def per_pixel(a, name):
            t = torch.as_tensor(a, dtype=torch.float32, device=dev)
            if tuple(t.shape) not in ((H, W), (B, H, W)):
                raise ValueError(f"{name} must be [{H}, {W}] or [{B}, {H}, {W}], got {tuple(t.shape)}")
            return t.contiguous()
        obs, err = per_pixel(observed_image, "observed_image"), per_pixel(err_map, "err_map")
        good = torch.isfinite(err) & (err > 0)
        if not bool((good | ~used).all()):
            raise ValueError("err_map must be finite and > 0 on every used pixel")
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        weight = torch.where(used & good, 1.0 / (err * err), zero).contiguous()
        noise = torch.where(used & good, torch.log(2.0 * math.pi * err.double() ** 2), zero.double()).reshape(-1, H * W).sum(dim=1)
        data = {"obs": obs, "weight": weight, "noise": noise}
        if key is not None:  # (the tensors are kept alongside: their ids stay theirs)
            self._point_cache = (key, given, data)
        return data

    def _point_outputs(self, p, amp, model, chi2, ok):
        good = ok != 0
        return {"amplitudes": amp, "model_image": model, "extended_image": p["extended"], "chi2": chi2,
                "log_like": -0.5 * chi2 - 0.5 * p["noise"], "ok": good}

    def fit_point_images(self, params, x, y, observed_image, err_map, *, mask=None):
        """The extended model plus ``J`` point images at ``(x, y)`` ``[B, J]`` whose amplitudes are solved per sample (beyond the
        reference; the linear amplitudes of lenstronomy's point sources): ``m = E + sum_j a_j D_j`` with ``E = simulate(params)`` and
        ``D_j`` the unit point images of ``point_images``.  On the used pixels ``U`` (``pix_region`` and ``mask`` ``[H, W]`` bool), with
        ``w = 1 / err_map^2``: ``N_jk = sum_U w D_j D_k``, ``r_j = sum_U w D_j (obs - E)``, ``a = N^-1 r`` by Cholesky (sums and solve
        in float64), ``chi2 = sum_U w (obs - m)^2``, ``log_like = -chi2 / 2 - sum_U log(2 pi err^2) / 2``.  The amplitudes are not
        constrained in sign.

        ``observed_image``, ``err_map``: ``[H, W]`` or ``[B, H, W]``.  Returns a dict: ``amplitudes`` ``[B, J]``, ``model_image`` and
        ``extended_image`` ``[B, H, W]``, ``chi2`` and ``log_like`` ``[B]`` (float64), ``ok`` ``[B]`` bool -- false where a Cholesky
        pivot is not finite or not above 1e-6 of its diagonal entry (coincident images, an image on unused pixels alone, an image
        outside the frame); that sample's other outputs (``extended_image`` aside) are then NaN.  ``ValueError``: shapes, more than
        ``MAX_POINT_IMAGES`` images, an ``err_map`` that is not finite or not > 0 on a used pixel, no used pixel.  Forward only."""
        p = self._point_prepare("fit_point_images", params, x, y, observed_image, err_map, mask)
        amp, model, _, chi2, ok, _, _ = self._model.ptimg_fit(p["x"], p["y"], self._point_transform(), p["extended"], p["obs"],
                                                              p["weight"], False)
        return self._point_outputs(p, amp, model, chi2, ok)

    def point_image_log_like_and_grad(self, params, x, y, observed_image, err_map, *, mask=None):
        """``fit_point_images`` with the gradient of ``log_like``: the dict gains ``grad`` ``[B, P]`` (packed order) and ``grad_x``,
        ``grad_y`` ``[B, J]``.  The amplitudes maximise ``log_like``, so no term goes through them (envelope theorem):
        ``d log_like / dE = w (obs - m)`` on the used pixels -- handed to the render's VJP for ``grad`` -- and
        ``d log_like / d(x_j, y_j) = a_j sum_U w (obs - m) dD_j / d(x_j, y_j)``.  Rows with ``ok == False`` are NaN.  Deterministic."""
        p = self._point_prepare("point_image_log_like_and_grad", params, x, y, observed_image, err_map, mask)
        amp, model, cot, chi2, ok, gx, gy = self._model.ptimg_fit(p["x"], p["y"], self._point_transform(), p["extended"], p["obs"],
                                                                  p["weight"], True)
        out = self._point_outputs(p, amp, model, chi2, ok)
        good = out["ok"]
        grad = self._model.simulate_bwd(p["packed"], torch.where(good[:, None, None], cot, torch.zeros_like(cot)))
        out["grad"] = torch.where(good[:, None], grad, torch.full_like(grad, float("nan")))
        out["grad_x"], out["grad_y"] = gx, gy
        return out

    def simulate(self, params, no_deflection=False):
        """tf/simulator.py:109-156.  Returns ``(bs, H, W)`` squeezed like ``tf.squeeze``."""
        packed = params if torch.is_tensor(params) else self.pack(params)
        if no_deflection:  # tf/simulator.py:125-126: sources are rendered on the un-deflected grid
            return self._parts(packed, 2 | 4)
        if self._mp is not None:  # lens planes: no autograd node (the gradient entry is simulate_vjp)
            return self._parts(packed, 1 | 2 | 4)
        img = _SimulateFn.apply(packed, self._model)
        return torch.squeeze(img)

    def simulate_vjp(self, params, cotangent):
        """The vector-Jacobian product of ``simulate``: ``cotangent`` ``[B, H, W]`` (or broadcastable to it) -> ``[B, P]`` in packed
        order.  On a model with several lens planes this is the gradient entry of ``simulate`` (``torch.autograd`` through
        ``simulate`` is served on one plane only)."""
        packed = params if torch.is_tensor(params) else self.pack(params)
        packed, cotangent = packed.detach(), torch.as_tensor(cotangent, device=packed.device)
        return self._model.multiplane_simulate_bwd(packed, cotangent) if self._mp is not None else self._model.simulate_bwd(packed, cotangent)

    def _parts(self, packed, parts):
        if self._mp is not None:
            if packed.requires_grad:
                raise NotImplementedError("renders of a model with several lens planes carry no autograd graph: simulate_vjp is their gradient")
            return torch.squeeze(self._model.multiplane_simulate(packed, parts))
        if packed.requires_grad:
            raise NotImplementedError("partial renders are forward-only helpers (no gradient)")
        return torch.squeeze(self._model.simulate_parts(packed, parts))

    def _pack_partial(self, params):
        """Partial renders only receive the groups they use; the unused columns are filled with a valid dummy (1)."""
        if torch.is_tensor(params):
            return params
        cols = []
        for g, i, name, const in self._layout.slots:
            grp = params.get(g)
            v = grp[i].get(name) if grp is not None and i < len(grp) else None
            v = const if v is None else v
            v = torch.as_tensor(1.0 if v is None else v, dtype=torch.float32, device=self.device)
            cols.append(v.reshape(-1).expand(self.bs) if v.numel() != self.bs else v.reshape(self.bs))
        return torch.stack(cols, dim=1)

    def simulate_source(self, params):
        """tf/simulator.py:242-269: the sources on the image grid, without lensing."""
        return self._parts(self._pack_partial(params), 4)

    def simulate_lens_light(self, params):
        """tf/simulator.py:271-297."""
        return self._parts(self._pack_partial(params), 2)

    def simulate_images(self, params):
        """tf/simulator.py:299-328: the lensed sources only."""
        return self._parts(self._pack_partial(params), 1 | 4)

    def lstsq_simulate(self, params, observed_image, err_map, return_stacked=False, return_coeffs=False,
                       no_deflection=False):
        """tf/simulator.py:158-240: render every ``use_lstsq`` light component as unit-amplitude basis images, solve
        ``coeffs = pinv(X^T X, rcond=1e-6) X^T Y`` per sample and return the best-fit image (default), the stack
        ``(bs, H, W, depth)`` or the coefficients ``(bs, depth)``.  All light profiles of the model must have been
        built with ``use_lstsq=True`` (the reference stacks every component, :183-201)."""
        self._single_plane("lstsq_simulate")
        if len(self._layout.linear) != self._model.num_linear():
            raise ValueError("lstsq_simulate needs every light profile built with use_lstsq=True")
        packed = params if torch.is_tensor(params) else self.pack(params)
        parts = (0 if no_deflection else 1) | 2 | 4
        if return_stacked:
            (stack,) = self._model.lstsq(packed, None, None, parts, want="stacked")
            return stack.permute(0, 2, 3, 1)
        obs = torch.as_tensor(observed_image, dtype=torch.float32, device=self.device).contiguous()
        err = torch.as_tensor(err_map, dtype=torch.float32, device=self.device).contiguous()
        if return_coeffs:
            return self._model.lstsq(packed, obs, err, parts, want="coeffs")[0]
        return torch.squeeze(self._model.lstsq(packed, obs, err, parts, want="image")[0])
