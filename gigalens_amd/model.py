"""``PhysicalModel`` and ``ForwardProbModel`` with the reference's surface
(src/gigalens/model.py:7-73, src/gigalens/tf/model.py:12-194,276-306).

``ForwardProbModel.log_prob(simulator, z)`` returns ``(log_prob, red_chi2)`` exactly like the reference;
the pixel log-likelihood and its gradient w.r.t. every profile parameter come from ONE fused HIP launch
sequence (prep -> main -> finalize, see csrc/gl_kernels.hip.h); prior densities and bijectors are a few
elementwise torch ops on ``(B, d)``.
"""
import math
import weakref
from typing import Dict, List

import numpy as np
import torch

from gigalens_amd import _native
from gigalens_amd import prior as _prior

_GROUPS = ("lens_mass", "lens_light", "source_light")


class _Packing:
    """Map between the reference's nested parameter structure and the native ``[B, P]`` rows
    (component-major: lenses, lens light, source light; inside a component the reference's
    ``params`` order).  Fixed parameters come from the ``*_constants`` dicts (model.py:29-44)."""

    def __init__(self, phys_model):
        self.slots = []  # (group, index, name, const_value_or_None)
        groups = ((phys_model.lenses, phys_model.lenses_constants),
                  (phys_model.lens_light, phys_model.lens_light_constants),
                  (phys_model.source_light, phys_model.source_light_constants))
        self.linear = []  # packed columns of amplitudes solved by least squares (use_lstsq profiles)
        for gname, (profiles, consts) in zip(_GROUPS, groups):
            for i, (prof, c) in enumerate(zip(profiles, consts)):
                for name in prof._native_params():
                    if name not in prof.params:  # linear amplitude: unit placeholder until lstsq fills it
                        self.linear.append(len(self.slots))
                        self.slots.append((gname, i, name, np.float32(1.0)))
                    else:
                        self.slots.append((gname, i, name, c.get(name)))
        self.P = len(self.slots)

    def pack(self, params: Dict[str, List[Dict]], bs: int, device):
        cols = []
        for gname, i, name, const in self.slots:
            grp = params.get(gname)
            v = grp[i].get(name) if grp is not None and i < len(grp) else None
            if v is None:
                v = const
            if v is None:
                raise KeyError(f"parameter {gname}[{i}]['{name}'] is neither given nor a model constant")
            v = torch.as_tensor(v, dtype=torch.float32, device=device)
            cols.append(v.reshape(-1).expand(bs) if v.numel() != bs else v.reshape(bs))
        if not cols:
            return torch.zeros((bs, 0), dtype=torch.float32, device=device)
        return torch.stack(cols, dim=1)


class PhysicalModelBase:
    """src/gigalens/model.py:7-44."""

    def __init__(self, lenses, lens_light, source_light, lenses_constants: List[Dict] = None,
                 lens_light_constants: List[Dict] = None, source_light_constants: List[Dict] = None):
        self.lenses = lenses
        self.lens_light = lens_light
        self.source_light = source_light
        if lenses_constants is None:
            lenses_constants = [dict() for _ in range(len(lenses))]
        if lens_light_constants is None:
            lens_light_constants = [dict() for _ in range(len(lens_light))]
        if source_light_constants is None:
            source_light_constants = [dict() for _ in range(len(source_light))]
        self.lenses_constants = lenses_constants
        self.lens_light_constants = lens_light_constants
        self.source_light_constants = source_light_constants


class PhysicalModel(PhysicalModelBase):
    """src/gigalens/tf/model.py:276-306: constants are cast to float32."""

    def __init__(self, lenses, lens_light, source_light, lenses_constants: List[Dict] = None,
                 lens_light_constants: List[Dict] = None, source_light_constants: List[Dict] = None,
                 source_light_scales=None, multiplane=None):
        """``source_light_scales`` (beyond the reference): one deflection scale per ``source_light`` entry, for sources at different
        redshifts behind the one lens plane -- source s is rendered at ``beta_s = theta - c_s sum alpha``
        (``gigalens_amd.cosmology.deflection_scale`` gives c from the redshifts).  Default: all 1, the reference's single plane.

        ``multiplane`` (beyond the reference): a ``gigalens_amd.cosmology.MultiPlane`` -- the lenses sit at redshifts of their own.
        With one plane it is rewritten here into ``source_light_scales`` (the existing kernels, the existing bits).  With two to four
        planes ``LensSimulator`` traces every ray through them in redshift order (``self.multiplane``): lens maps, renders with
        ``LensSimulator.simulate_vjp``, ``ForwardProbModel.stats_pixels`` and, on a ``ForwardProbModel`` without image positions, the
        fused ``log_prob`` / ``log_prob_and_grad`` / ``term_log_prob_and_grad`` that MAP, SVI, HMC and SMC run on -- with the
        image-position likelihood when the ``ForwardProbModel`` places its families by ``centroids_redshifts``.
        ``LensSimulator.image_positions(source_redshifts=...)`` solves the lens equation for sources at redshifts of their own.
        ``BackwardProbModel`` / ``lstsq_simulate``, the solver without ``source_redshifts``, curves, potentials and
        ``reconstruct_source`` raise ``_native.UnsupportedLensError``."""
        super().__init__(lenses, lens_light, source_light, lenses_constants, lens_light_constants,
                         source_light_constants)
        self.multiplane = None
        self._multiplane_single = None  # a one-plane MultiPlane, kept for ForwardProbModel(centroids_redshifts=...)
        if multiplane is not None:
            if source_light_scales is not None:
                raise ValueError("multiplane and source_light_scales are two ways to place the sources: give one")
            if len(multiplane.plane_of_lens) != len(lenses) or multiplane.S != len(source_light):
                raise ValueError(f"multiplane describes {len(multiplane.plane_of_lens)} lens(es) and {multiplane.S} source(s), the model "
                                 f"has {len(lenses)} and {len(source_light)}")
            if multiplane.K == 1:
                source_light_scales = multiplane.source_scales[0]
                self._multiplane_single = multiplane
            else:
                self.multiplane = multiplane
        self.source_light_scales = _native.deflection_scales(source_light_scales, len(source_light), "source_light_scales")
        self._source_scales_given = source_light_scales is not None
        cast = lambda ds: [{k: np.asarray(v, dtype=np.float32) for k, v in d.items()} for d in ds]
        self.lenses_constants = cast(self.lenses_constants)
        self.lens_light_constants = cast(self.lens_light_constants)
        self.source_light_constants = cast(self.source_light_constants)

    def _packing(self):
        return _Packing(self)


class ProbabilisticModel:
    """src/gigalens/model.py:47-73."""

    def __init__(self, prior, bij=None, *args):
        self.prior = prior
        self.bij = bij

    def log_prob(self, simulator, z):
        raise NotImplementedError


class _GradFn(torch.autograd.Function):
    """The autograd glue of every native likelihood whose gradient comes out of the same launches as its value:
    ``fn(*detached inputs, want_grad)`` returns ``(outputs, grads)`` -- one gradient ``[B, ...]`` of the first output per input, kept
    for ``backward`` -- and every output but the first is a statistic that carries no gradient.  ``want_grad`` tells ``fn`` whether
    any input requires one; without, nothing is kept."""

    @staticmethod
    def forward(ctx, fn, *inputs):
        want = any(t.requires_grad for t in inputs)
        outputs, grads = fn(*(t.detach() for t in inputs), want)
        if want:
            ctx.save_for_backward(*grads)
        ctx.mark_non_differentiable(*outputs[1:])
        return tuple(outputs)

    @staticmethod
    def backward(ctx, g, *_):
        return (None,) + tuple(g[:, None] * grad for grad in ctx.saved_tensors)


def _split(result):
    """``(outputs..., grad)`` of a native entry as the ``(outputs, grads)`` of ``_GradFn``."""
    return result[:-1], result[-1:]


def _from_dict(res, outputs, grads=("grad",)):
    """The dict of a ``LensSimulator.*_and_grad`` method (float64 statistics as float32) as the ``(outputs, grads)`` of ``_GradFn``."""
    return tuple(res[k].float() for k in outputs), tuple(res[k] for k in grads)


def _log_like(packed, model, *image):
    """``(log_like, chi2)`` of gl_loglike_fwd_bwd, differentiable in the packed rows; forward only when they need no gradient."""
    return _GradFn.apply(lambda p, want: _split(model.loglike(p, *image, want)), packed)


def _point_term(packed, entry):
    """``(log_like, chi2)`` of a point-image term of the native model, differentiable in the packed rows: ``entry`` is its bound
    ``positions`` (gl_positions_fwd_bwd), ``multiplane_positions`` (gl_multiplane_positions_fwd_bwd), ``position_fluxes``
    (gl_position_fluxes_fwd_bwd) or ``position_delays`` (gl_position_delays_fwd_bwd); forward only when they need no gradient."""
    return _GradFn.apply(lambda p, want: _split(entry(p, want)), packed)


class _GraphEntry:
    """One captured ``log_prob_and_grad`` launch sequence with what its device pointers refer to: the static input and outputs, the
    workspace (held here, so the caching allocator cannot hand it out while the graph lives) and, to tell whether the rest still
    stands, the native model's generation at capture and the image tensors of the owning ``ForwardProbModel``."""
    __slots__ = ("graph", "z_static", "outs", "owner", "terms", "workspace", "generation", "inputs")

    def __init__(self, graph, z_static, outs, owner, simulator, terms):
        model = simulator._model
        self.graph, self.z_static, self.outs, self.owner, self.terms = graph, z_static, outs, owner, terms
        self.workspace = model._workspace(z_static.shape[0])
        self.generation = model.generation
        self.inputs = (owner.observed_image, owner.error_map, owner._mask(simulator))

    def valid(self, simulator):
        """False once anything was handed to the native model after the capture (every ``set_*`` frees or re-sizes device buffers the
        graph points into), another model was bound, or the owner's image tensors were replaced."""
        model, owner = simulator._model, self.owner
        obs, err, mask = self.inputs
        return (model.generation == self.generation and model.prior_owner is owner
                and (model.positions_owner is owner or not self.terms & 2)
                and owner.observed_image is obs and owner.error_map is err and owner._mask(simulator) is mask)


def _family_fluxes(fluxes, errors, centroids_x):
    """``(fluxes, errors, n_flux)`` of ``ForwardProbModel(centroids_fluxes=..., centroids_fluxes_errors=...)``: one float32 array per
    family shaped like its ``centroids_x``, NaN where an image has no measurement (its error is not looked at), errors broadcast as
    the position errors are.  ``ValueError`` as the constructor documents."""
    if (fluxes is None) != (errors is None):
        raise ValueError("centroids_fluxes and centroids_fluxes_errors come together: give both or neither")
    if fluxes is None:
        return None, None, 0.0
    if centroids_x is None:
        raise ValueError("centroids_fluxes needs centroids_x/centroids_y (include_positions=True)")
    if len(fluxes) != len(centroids_x) or len(errors) != len(centroids_x):
        raise ValueError(f"centroids_fluxes / centroids_fluxes_errors: one entry per image family ({len(centroids_x)}), got "
                         f"{len(fluxes)} / {len(errors)}")
    out_f, out_s, n_flux = [], [], 0
    for f, (F, s, x) in enumerate(zip(fluxes, errors, centroids_x)):
        if F is None:  # a family without fluxes
            out_f.append(np.full(x.shape, np.nan, dtype=np.float32))
            out_s.append(np.full(x.shape, np.nan, dtype=np.float32))
            continue
        F = np.atleast_1d(np.asarray(F, dtype=np.float32))
        if F.shape != x.shape:
            raise ValueError(f"centroids_fluxes[{f}] has shape {F.shape}, the family's centroids_x {x.shape}")
        if s is None:
            raise ValueError(f"centroids_fluxes[{f}] without centroids_fluxes_errors[{f}]")
        try:
            s = np.broadcast_to(np.atleast_1d(np.asarray(s, dtype=np.float32)), x.shape).copy()
        except ValueError:
            raise ValueError(f"centroids_fluxes_errors[{f}] does not broadcast to the family's shape {x.shape}") from None
        measured = ~np.isnan(F)
        if not np.all(np.isfinite(F[measured])):
            raise ValueError(f"centroids_fluxes[{f}]: a measured flux must be finite (NaN marks an image without one), got {F.tolist()}")
        if not np.all(np.isfinite(s[measured])):
            raise ValueError(f"centroids_fluxes_errors[{f}]: the error of a measured flux must be finite, got {s.tolist()}")
        if np.any(s[measured] <= 0):
            raise ValueError(f"centroids_fluxes_errors[{f}]: the error of a measured flux must be > 0, got {s.tolist()}")
        if int(measured.sum()) == 1:
            raise ValueError(f"centroids_fluxes[{f}]: one measured flux -- the term constrains flux ratios, a family takes two or more "
                             "measured fluxes, or none")
        n_flux += int(measured.sum())
        out_f.append(F)
        out_s.append(s)
    return out_f, out_s, float(n_flux)


def _family_h0(h0, n_fam):
    """``[F]`` float64 of ``ForwardProbModel(time_delay_h0=...)`` in km/s/Mpc, NaN where the family's H0 is profiled out:
    ``"profile"``, one float for every family, or a sequence of ``n_fam`` entries, each a float or ``None`` (profiled).  ``ValueError``
    for a wrong count and a value that is not finite and > 0."""
    if isinstance(h0, str):
        if h0 != "profile":
            raise ValueError(f"time_delay_h0: 'profile', a float in km/s/Mpc or one float / None per image family, got {h0!r}")
        return np.full(n_fam, np.nan)
    entries = [h0] * n_fam if np.ndim(h0) == 0 else list(h0)
    if len(entries) != n_fam:
        raise ValueError(f"time_delay_h0: one entry per image family ({n_fam}), got {len(entries)}")
    out = np.asarray([np.nan if v is None else float(v) for v in entries], dtype=np.float64)
    given = np.asarray([v is not None for v in entries], dtype=bool)
    if np.any(given & ~(np.isfinite(out) & (out > 0.0))):
        raise ValueError(f"time_delay_h0: every H0 must be finite and > 0 (km/s/Mpc; None: profiled out), got {entries!r}")
    return out


def _family_delays(delays, errors, distances, centroids_x, scale_name="time_delay_distances"):
    """``(delays, errors, distances [F] float64 with NaN = profiled, n_delay)`` of ``ForwardProbModel(centroids_time_delays=...,
    centroids_time_delays_errors=..., time_delay_distances=...)``: one float32 array per family shaped like its ``centroids_x``, NaN
    where an image has no measured arrival time (its error is not looked at), errors broadcast as the flux errors are.
    ``ValueError`` as the constructor documents.  ``scale_name``: the keyword the scales came from (``time_delay_h0`` hands its
    entries in here, so that the family-size rules read them)."""
    if (delays is None) != (errors is None):
        raise ValueError("centroids_time_delays and centroids_time_delays_errors come together: give both or neither")
    if delays is None:
        if distances is not None:
            raise ValueError("time_delay_distances needs centroids_time_delays / centroids_time_delays_errors")
        return None, None, None, 0.0
    if centroids_x is None:
        raise ValueError("centroids_time_delays needs centroids_x/centroids_y (include_positions=True)")
    n_fam = len(centroids_x)
    if len(delays) != n_fam or len(errors) != n_fam:
        raise ValueError(f"centroids_time_delays / centroids_time_delays_errors: one entry per image family ({n_fam}), got "
                         f"{len(delays)} / {len(errors)}")
    if distances is None:
        distances = [None] * n_fam
    elif np.ndim(distances) == 0:
        raise ValueError(f"time_delay_distances: one float (Mpc) or None per image family ({n_fam}), or a single None; got {distances!r}")
    if len(distances) != n_fam:
        raise ValueError(f"time_delay_distances: one entry per image family ({n_fam}), got {len(distances)}")
    dist = np.asarray([np.nan if d is None else float(d) for d in distances], dtype=np.float64)
    out_t, out_s, n_delay = [], [], 0
    for f, (t, s, x) in enumerate(zip(delays, errors, centroids_x)):
        if t is None:  # a family without delays
            out_t.append(np.full(x.shape, np.nan, dtype=np.float32))
            out_s.append(np.full(x.shape, np.nan, dtype=np.float32))
            continue
        t = np.atleast_1d(np.asarray(t, dtype=np.float32))
        if t.shape != x.shape:
            raise ValueError(f"centroids_time_delays[{f}] has shape {t.shape}, the family's centroids_x {x.shape}")
        if s is None:
            raise ValueError(f"centroids_time_delays[{f}] without centroids_time_delays_errors[{f}]")
        try:
            s = np.broadcast_to(np.atleast_1d(np.asarray(s, dtype=np.float32)), x.shape).copy()
        except ValueError:
            raise ValueError(f"centroids_time_delays_errors[{f}] does not broadcast to the family's shape {x.shape}") from None
        measured = ~np.isnan(t)
        if not np.all(np.isfinite(t[measured])):
            raise ValueError(f"centroids_time_delays[{f}]: a measured arrival time must be finite (NaN marks an image without one), got "
                             f"{t.tolist()}")
        if not np.all(np.isfinite(s[measured])):
            raise ValueError(f"centroids_time_delays_errors[{f}]: the error of a measured arrival time must be finite, got {s.tolist()}")
        if np.any(s[measured] <= 0):
            raise ValueError(f"centroids_time_delays_errors[{f}]: the error of a measured arrival time must be > 0, got {s.tolist()}")
        n = int(measured.sum())
        if n == 1:
            raise ValueError(f"centroids_time_delays[{f}]: one measured arrival time -- the term constrains delay differences, a family "
                             "takes two or more measured times, or none")
        if n and np.isinf(dist[f]):
            raise ValueError(f"{scale_name}[{f}] must be finite (None: profiled out), got {dist[f]}")
        if n == 2 and np.isnan(dist[f]):
            raise ValueError(f"centroids_time_delays[{f}]: two measured arrival times with a profiled time-delay distance -- the fit is "
                             f"exact and constrains nothing; give {scale_name} or three or more measured times")
        n_delay += n
        out_t.append(t)
        out_s.append(s)
    return out_t, out_s, dist, float(n_delay)


class _PackBijector:
    """``pack_bij`` (tf/model.py:78-85): ``(B, d)`` <-> nested structure, column k = k-th nest leaf."""

    def __init__(self, template):
        self.template = template
        self.d = len(_prior.nest_flatten(template))

    def forward(self, z):
        return _prior.nest_pack(self.template, [z[..., k] for k in range(self.d)])

    def inverse(self, struct):
        leaves = [torch.as_tensor(v, dtype=torch.float32) for v in _prior.nest_flatten(struct)]
        dev = next((v.device for v in leaves if v.is_cuda), leaves[0].device)
        return torch.stack(torch.broadcast_tensors(*[v.to(dev) for v in leaves]), dim=-1)


class _ChainBijector:
    """``bij = Chain([unconstraining_bij, pack_bij])`` (tf/model.py:87)."""

    def __init__(self, unconstraining, pack):
        self.unconstraining, self.pack = unconstraining, pack

    def forward(self, z):
        return self.unconstraining.forward(self.pack.forward(z))

    def inverse(self, x_struct):
        return self.pack.inverse(self.unconstraining.inverse(x_struct))


class _StreamProbModel(ProbabilisticModel):
    """What every probabilistic model here shares: the device, the prior's flat form with its bijectors, ``log_prior``, and what
    ``ModellingSequence.MAP / SVI / HMC`` ask of a model on the stream path -- ``log_prob_and_grad`` by autograd through the
    subclass's ``log_prob``, ``init_centroids``, and the counts its loss is sized with (``ForwardProbModel`` has a fused
    ``log_prob_and_grad`` of its own)."""

    include_pixels, include_positions, n_position, n_flux, n_delay = True, False, 0.0, 0.0, 0.0

    def __init__(self, prior):
        super().__init__(prior)
        # host logic (prior, bijectors) also runs without a GPU; the likelihood itself never does
        self.device = _native.device() if torch.cuda.is_available() else torch.device("cpu")

    def _bind_prior_structure(self, prior):
        """``_flat``, ``pack_bij``, ``unconstraining_bij`` and ``bij`` (tf/model.py:78-87) of ``prior``; returns the example sample
        the structure is read from.  Called by a constructor after its own argument checks."""
        self._flat = prior.flat(self.device)
        example = prior.sample(seed=0)
        self.pack_bij = _PackBijector(example)
        self.unconstraining_bij = _prior.JointBijector(self._flat)
        self.bij = _ChainBijector(self.unconstraining_bij, self.pack_bij)
        return example

    def _log_prior_at(self, z, x):
        return self._flat.log_prob(x) + self._flat.fldj_columns(z).sum(-1)

    def _x_and_log_prior(self, z):
        """``z`` as a float32 tensor on the model's device, the constrained ``x`` and ``log_prior(z)``."""
        z = torch.as_tensor(z, dtype=torch.float32, device=self.device)
        x = self._flat.forward(z)
        return z, x, self._log_prior_at(z, x)

    def log_prior(self, z):
        """tf/model.py:182-185."""
        return self._x_and_log_prior(z)[2]

    def log_prob_and_grad(self, simulator, z, graph=False):
        """``(log_prob, red_chi2, d log_prob / d z)``, detached, by autograd through ``log_prob``; ``graph`` is accepted and ignored."""
        zz = torch.as_tensor(z, dtype=torch.float32, device=self.device).detach().requires_grad_(True)
        lp, red = self.log_prob(simulator, zz)
        (g,) = torch.autograd.grad(lp.sum(), zz)
        return lp.detach(), red.detach(), g

    def init_centroids(self, bs):
        """tf/model.py:187-194 (no-op without the position branch)."""
        return None


class _JoinsStrong(_StreamProbModel):
    """A point-like term of its own (``n_own`` data) that a ``ForwardProbModel`` over the same prior may join (``strong=``): the prior
    is counted once, inside ``strong``'s term, and the reduced chi^2 weighs the two by their data counts."""

    def _bind_strong(self, strong, n_own):
        """The check of ``strong`` and what ``ModellingSequence`` sizes its loss with: the ``n_own`` data count with the point terms."""
        if strong is not None and not isinstance(strong, ForwardProbModel):
            raise TypeError("strong must be a ForwardProbModel over the same prior")
        self.strong = strong
        self.include_pixels = bool(strong is not None and strong.include_pixels)
        self.include_positions = True
        self.n_position = n_own
        if strong is not None and strong.include_positions:
            self.n_position += strong.n_position + strong.n_flux + strong.n_delay

    def _join(self, simulator, z, x, ll, chi2, n_own):
        """``(log_prob, reduced chi^2)`` of this model's ``(ll, chi2)`` over ``n_own`` data, with ``strong``'s when there is one."""
        if self.strong is None:
            return ll + self._log_prior_at(z, x), chi2 / n_own
        lp_strong, red_strong = self.strong.log_prob(simulator, z)  # (carries the prior)
        n_strong = float(self.strong._n_eff(simulator))
        return ll + lp_strong, (chi2 + red_strong * n_strong) / (n_own + n_strong)


class ForwardProbModel(_StreamProbModel):
    """Drop-in for ``gigalens.tf.model.ForwardProbModel`` (tf/model.py:12-194): pixel likelihood and
    image-position likelihood.  With the reference's default ``include_positions=True`` and no centroids the
    reference itself fails (it iterates ``None``, tf/model.py:69-70), so that combination raises ``TypeError``."""

    def __init__(self, prior, observed_image=None, background_rms=None, exp_time=None, error_map=None,
                 centroids_x=None, centroids_y=None, centroids_errors_x=None, centroids_errors_y=None,
                 include_pixels=True, include_positions=True, centroids_scales=None, centroids_redshifts=None,
                 centroids_fluxes=None, centroids_fluxes_errors=None, centroids_time_delays=None,
                 centroids_time_delays_errors=None, time_delay_distances=None, time_delay_h0=None):
        """``centroids_scales`` (beyond the reference): one deflection scale per image family of ``centroids_x`` -- a family at its
        own redshift is traced with ``beta = theta - c_f alpha`` and ``A = I - c_f H`` in the position likelihood, the predicted
        positions and the image-plane rms.  Default: all 1.

        ``centroids_redshifts`` (beyond the reference; instead of ``centroids_scales``): one redshift per image family, for a
        ``PhysicalModel`` built with a ``cosmology.MultiPlane``.  When the model is bound to a simulator the family's couplings are
        ``MultiPlane.target_scales(z_f)``: on two to four lens planes every observed image is traced back through the planes in
        front of its family (``beta = theta - sum_i T_f,i a_i``, ``A = d beta / d theta``) in ``stats_positions`` and the fused
        ``log_prob`` / ``log_prob_and_grad`` / ``term_log_prob_and_grad``; on one plane they are the ``centroids_scales``.
        ``ValueError``: a redshift that is not finite, given together with ``centroids_scales`` or without centroids; at bind time, a
        family at or in front of the first plane, or a model without a ``MultiPlane`` (use ``centroids_scales``).

        ``centroids_fluxes`` / ``centroids_fluxes_errors`` (beyond the reference): one array per image family, shaped like
        ``centroids_x[f]`` -- the measured fluxes ``F_j`` of the images and their errors ``s_j`` (broadcast as the position errors are);
        NaN marks an image without a measurement, ``None`` or an all-NaN array a family without fluxes.  With ``m_j = 1 / |det A_j|`` at
        the observed positions the family's unlensed flux is profiled out, ``S_f = sum w F m / sum w m^2`` (``w = 1 / s^2``), and
        ``log_like_f = -1/2 (sum w (F - S_f m)^2 + sum log(2 pi s^2))`` joins the image-position term of ``log_prob``,
        ``log_prob_unfused``, ``log_like``, ``log_prob_and_grad`` and ``term_log_prob_and_grad(..., "positions")``, whose reduced chi^2
        becomes ``(chi2_pos + chi2_flux) / (n_position + n_flux)``; ``stats_fluxes`` and ``predicted_fluxes`` give the term alone.  Only
        flux ratios are constrained.  ``ValueError``: fluxes without centroids, fluxes without errors or the reverse, a shape mismatch,
        exactly one measured flux in a family, a measured flux that is not finite or whose error is not finite and > 0.

        ``centroids_time_delays`` / ``centroids_time_delays_errors`` (beyond the reference): one array per image family, shaped like
        ``centroids_x[f]`` -- the measured arrival times ``t_j`` of the images in days, relative to any zero, and their errors ``s_j``
        (broadcast as the flux errors are); NaN marks an image without a measurement, ``None`` or an all-NaN array a family without
        delays.  ``time_delay_distances``: ``D_dt`` of every family in Mpc, or ``None`` to profile it out (a single ``None``: all).
        With the Fermat potential ``phi_j = |theta_j - mean beta|^2 / 2 - psi(theta_j)`` of the family's barycentre source,
        ``lambda_f = D_dt DAYS_PER_MPC_ARCSEC2`` (or ``sum w t~ phi~ / sum w phi~^2``, ``~``: minus the ``w = 1 / s^2`` weighted mean)
        and ``log_like_f = -1/2 (sum w (t~ - lambda_f phi~)^2 + sum log(2 pi s^2))`` joins the image-position term of ``log_prob``,
        ``log_prob_unfused``, ``log_like``, ``log_prob_and_grad`` and ``term_log_prob_and_grad(..., "positions")``, whose reduced chi^2
        becomes ``(chi2_pos + chi2_flux + chi2_delay) / (n_position + n_flux + n_delay)``; ``stats_time_delays`` and
        ``fitted_time_delays`` give the term alone.  The zero of every family's clock is profiled out: only delay differences are
        constrained.  ``ValueError``: delays without centroids, delays without errors or the reverse, a shape mismatch, exactly one
        measured time in a family, two with a profiled distance (the fit is exact), a measured time that is not finite or whose error
        is not finite and > 0, a distance that is not finite.  At bind time: ``UnsupportedLensError`` on lens planes and for lenses
        without a potential (series expansions, user-written bodies), ``NotImplementedError`` for a family with delays whose
        ``centroids_scales`` differs from 1.

        ``time_delay_h0`` (with ``centroids_redshifts`` and the delays; instead of ``time_delay_distances``): the opt-in to the
        time-delay term on two to four lens planes.  ``"profile"``, one H0 in km/s/Mpc for every family, or one entry per family,
        each a float or ``None`` (profiled).  Family f is traced through the planes in front of it, its source is ``mean beta``, and
        ``phi_j = T(theta_j; mean beta)`` is the arrival time of the ray through the planes in arcsec^2 ``c / H0``
        (``MultiPlane.delay_weights(z_f)``; ``LensSimulator.time_delays(source_redshifts=...)`` evaluates the same sum); the rest
        of the term is as above with ``lambda_f = cosmology.hubble_distance_mpc(h0_f) DAYS_PER_MPC_ARCSEC2``, so a profiled scale
        is ``c / H0`` itself: ``fitted_time_delays`` returns it in Mpc and ``fitted_h0`` as H0.  ``ValueError``: together with
        ``time_delay_distances``, without delays or without ``centroids_redshifts``, a wrong count, a value that is not finite and
        > 0; two measured times need a given H0.  At bind time: ``ValueError`` for a simulator without several lens planes (give
        ``time_delay_distances`` there).  A model built without ``time_delay_h0`` is refused on lens planes as before."""
        super().__init__(prior)
        self.include_pixels = include_pixels
        self.include_positions = include_positions
        self.observed_image = None
        self.error_map = None
        self.background_rms = None
        self.exp_time = None
        if self.include_pixels:
            self.observed_image = torch.as_tensor(np.asarray(observed_image, dtype=np.float32), device=self.device).contiguous()
            if error_map is not None:
                self.error_map = torch.as_tensor(np.asarray(error_map, dtype=np.float32), device=self.device).contiguous()
            else:
                self.background_rms = float(np.float32(background_rms))
                self.exp_time = float(np.float32(exp_time))
        self.centroids_x = self.centroids_y = self.centroids_errors_x = self.centroids_errors_y = None
        self.n_position = 0.0
        if self.include_positions:
            if centroids_x is None:
                raise TypeError("include_positions=True needs centroids_x/centroids_y (the reference iterates them, "
                                "tf/model.py:69-70); pass include_positions=False for a pixel-only model")
            f32 = lambda L: [np.atleast_1d(np.asarray(v, dtype=np.float32)) for v in L]
            self.centroids_x, self.centroids_y = f32(centroids_x), f32(centroids_y)
            self.centroids_errors_x = [np.broadcast_to(e, x.shape).copy() for e, x in zip(f32(centroids_errors_x), self.centroids_x)]
            self.centroids_errors_y = [np.broadcast_to(e, x.shape).copy() for e, x in zip(f32(centroids_errors_y), self.centroids_y)]
            self.n_position = 2.0 * float(sum(x.size for x in self.centroids_x))  # tf/model.py:74
        if centroids_scales is not None and self.centroids_x is None:
            raise ValueError("centroids_scales needs centroids_x/centroids_y (include_positions=True)")
        n_fam = len(self.centroids_x) if self.centroids_x is not None else 0
        self.centroids_scales = _native.deflection_scales(centroids_scales, n_fam, "centroids_scales")
        self._centroids_scales_given = centroids_scales is not None
        self.centroids_redshifts = None
        if centroids_redshifts is not None:
            if centroids_scales is not None:
                raise ValueError("centroids_redshifts and centroids_scales are two ways to place the image families: give one")
            if self.centroids_x is None:
                raise ValueError("centroids_redshifts needs centroids_x/centroids_y (include_positions=True)")
            zf = np.atleast_1d(np.asarray(centroids_redshifts, dtype=np.float64))
            if zf.shape != (n_fam,):
                raise ValueError(f"centroids_redshifts: one redshift per image family ({n_fam}), got shape {zf.shape}")
            if not np.all(np.isfinite(zf)):
                raise ValueError(f"centroids_redshifts: every redshift must be finite, got {zf.tolist()}")
            self.centroids_redshifts = zf
        self.centroids_fluxes, self.centroids_fluxes_errors, self.n_flux = _family_fluxes(centroids_fluxes, centroids_fluxes_errors,
                                                                                          self.centroids_x)
        self.time_delay_h0 = None
        if time_delay_h0 is None:
            (self.centroids_time_delays, self.centroids_time_delays_errors, self.time_delay_distances,
             self.n_delay) = _family_delays(centroids_time_delays, centroids_time_delays_errors, time_delay_distances, self.centroids_x)
        else:  # the time-delay term on lens planes: H0 in the place of the distances
            if time_delay_distances is not None:
                raise ValueError("time_delay_h0 and time_delay_distances are two ways to scale the delays: give one (lens planes have "
                                 "no single time-delay distance, one plane takes no h0)")
            if centroids_time_delays is None or centroids_time_delays_errors is None:
                raise ValueError("time_delay_h0 needs centroids_time_delays / centroids_time_delays_errors")
            if self.centroids_redshifts is None:
                raise ValueError("time_delay_h0 needs centroids_redshifts: the arrival time through the lens planes depends on the "
                                 "redshift of every family (one plane: time_delay_distances)")
            h0 = _family_h0(time_delay_h0, n_fam)
            (self.centroids_time_delays, self.centroids_time_delays_errors, h0,
             self.n_delay) = _family_delays(centroids_time_delays, centroids_time_delays_errors,
                                            [None if np.isnan(v) else v for v in h0], self.centroids_x, "time_delay_h0")
            self.time_delay_h0, self.time_delay_distances = h0, np.full(n_fam, np.nan)
        self._paths = _prior.nest_paths(self._bind_prior_structure(prior))
        self._perm_cache = {}

    # ---- z columns -> native packed rows, without materialising the nested structure ----------------
    def _perm(self, simulator):
        key = id(simulator._layout)
        hit = self._perm_cache.get(key)
        if hit is None:
            index = {}
            for k, path in enumerate(self._paths):
                if len(path) != 3 or path[0] not in _GROUPS:
                    raise ValueError(f"prior leaf {path} does not follow {{group: [ {{name: dist}} ]}}")
                index[path] = k
            d = len(self._paths)
            cols, consts = [], []
            for gname, i, name, const in simulator._layout.slots:
                k = index.get((gname, i, name))
                if k is not None:
                    cols.append(k)
                elif const is not None:
                    cols.append(d + len(consts))
                    consts.append(float(np.asarray(const, dtype=np.float32).reshape(-1)[0]))
                else:
                    raise KeyError(f"{gname}[{i}]['{name}'] has neither a prior nor a constant")
            hit = (torch.tensor(cols, dtype=torch.int64, device=self.device),
                   torch.tensor(consts, dtype=torch.float32, device=self.device))
            self._perm_cache = {key: hit}
        return hit

    def _bind_prior(self, simulator):
        """Hand the prior / bijector column table to the simulator's native model (once per pairing)."""
        model = simulator._model
        if model.prior_owner is not self:
            slot_of = {(g, i, n): p for p, (g, i, n, _) in enumerate(simulator._layout.slots)}
            columns = []
            for k, (path, leaf) in enumerate(zip(self._paths, self._flat.leaves)):
                if tuple(path) not in slot_of:
                    raise KeyError(f"prior leaf {path} is not a parameter of the physical model")
                a, b, lo, hi = leaf._p()
                columns.append((slot_of[tuple(path)], leaf.bij, leaf.kind, a, b, lo, hi, float(self._flat.logz[k])))
            const_row = np.zeros(simulator._layout.P, dtype=np.float32)
            driven = {c[0] for c in columns}
            for p, (g, i, n, const) in enumerate(simulator._layout.slots):
                if p not in driven:
                    if const is None:
                        raise KeyError(f"{g}[{i}]['{n}'] has neither a prior nor a constant")
                    const_row[p] = float(np.asarray(const, dtype=np.float32).reshape(-1)[0])
            model.set_prior(columns, const_row)
            model.prior_owner = self
        return model

    def position_targets(self, multiplane):
        """``[F, K]`` couplings of the image families on the planes of ``multiplane``: row f = ``multiplane.target_scales(z_f)``, 0 for
        the planes at or behind family f.  ``ValueError`` for a family at or in front of the first plane."""
        if self.centroids_redshifts is None:
            raise ValueError("position_targets needs a model built with centroids_redshifts")
        return np.stack([multiplane.target_scales(z) for z in self.centroids_redshifts], axis=0)

    def _family_scales(self, simulator):
        """``(scales [F], given)``: the deflection scale of every image family on a single-plane simulator -- ``centroids_scales``, or
        ``centroids_redshifts`` through the one-plane ``MultiPlane`` the physical model was built with."""
        if self.centroids_redshifts is None:
            return self.centroids_scales, self._centroids_scales_given
        if simulator._mp is not None:
            raise _native.UnsupportedLensError(f"a model with {simulator._mp.K} lens planes: one deflection scale per family exists on a "
                                               "single plane alone (the solver, the predicted positions and their users)")
        mp = getattr(simulator.phys_model, "_multiplane_single", None)
        if mp is None:
            raise ValueError("centroids_redshifts needs a PhysicalModel built with a cosmology.MultiPlane (its planes turn the "
                             "redshifts into couplings); on a model without one give centroids_scales")
        return _native.deflection_scales(self.position_targets(mp)[:, 0], len(self.centroids_x), "centroids_redshifts"), True

    def _bind_positions(self, simulator):
        model = simulator._model
        if model.positions_owner is not self:
            mp = simulator._mp
            # (validated before anything is handed over: a refusal leaves the native model as it was)
            targets = self.position_targets(mp) if mp is not None and self.centroids_redshifts is not None else None
            if self.n_delay and self.time_delay_h0 is not None and mp is None:
                self._plane_delay_tables(simulator, None)  # (its ValueError: time_delay_h0 serves lens planes)
            scales, given = self._family_scales(simulator) if mp is None else (None, False)
            delay_scales = plane_delays = None
            if self.n_delay and self.time_delay_h0 is not None:
                plane_delays = self._plane_delay_tables(simulator, targets)
            elif self.n_delay:
                delay_scales = self._delay_scales(simulator, scales)
            model.set_positions(self.centroids_x, self.centroids_y, self.centroids_errors_x, self.centroids_errors_y)
            if targets is not None:
                model.set_position_targets(targets)
            elif given:
                model.set_position_scales(scales)
            if self.n_flux:  # (set_positions has cleared the fluxes of an earlier owner)
                model.set_position_fluxes(np.concatenate(self.centroids_fluxes), np.concatenate(self.centroids_fluxes_errors))
            if plane_delays is not None:  # (... and the arrival times: on lens planes, after the targets)
                model.set_position_plane_delays(np.concatenate(self.centroids_time_delays),
                                                np.concatenate(self.centroids_time_delays_errors), *plane_delays)
            elif self.n_delay:
                model.set_position_delays(np.concatenate(self.centroids_time_delays), np.concatenate(self.centroids_time_delays_errors),
                                          delay_scales)
            model.positions_owner = self
        return model

    def _delay_scales(self, simulator, scales):
        """``lambda_f [F]`` in days / arcsec^2 (NaN: profiled out) for a simulator the time-delay term is served on; its refusals, as
        ``predicted_time_delays`` words them, before anything is handed to the native model."""
        if simulator._mp is not None:
            raise _native.UnsupportedLensError(f"a model with {simulator._mp.K} lens planes: the time-delay term (centroids_time_delays) "
                                               "with time_delay_distances stays single-plane; on lens planes build the model with "
                                               "time_delay_h0")
        from gigalens_amd.simulator import LensSimulator
        LensSimulator._potential_lenses(simulator)
        has = np.asarray([bool(np.any(~np.isnan(t))) for t in self.centroids_time_delays])
        if np.any(has & (np.asarray(scales) != 1.0)):
            raise NotImplementedError("centroids_time_delays: the Fermat potential of a scaled source plane (centroids_scales != 1) "
                                      "is not served; time delays stay single-plane")
        return (self.time_delay_distances * LensSimulator.DAYS_PER_MPC_ARCSEC2).astype(np.float32)

    def _plane_delay_tables(self, simulator, targets):
        """``(geom [F, K] float64, pot [K] float64, lambda_f [F] float32)`` of a model built with ``time_delay_h0`` on a simulator
        with several lens planes: ``MultiPlane.delay_weights`` of every family, the potential weights of the farthest family with
        delays, and ``c / H0`` in days per arcsec^2 (NaN: profiled out).  Its refusals come before anything is handed to the native
        model."""
        mp = simulator._mp
        if mp is None or targets is None:
            raise ValueError("time_delay_h0 serves a model with several lens planes (a PhysicalModel built with a cosmology.MultiPlane "
                             "of two to four planes); on one plane give time_delay_distances")
        from gigalens_amd.cosmology import hubble_distance_mpc
        from gigalens_amd.simulator import LensSimulator
        LensSimulator._potential_lenses(simulator)
        weights = [mp.delay_weights(z) for z in self.centroids_redshifts]
        has = np.asarray([bool(np.any(~np.isnan(t))) for t in self.centroids_time_delays])
        far = int(np.argmax(np.where(has, self.centroids_redshifts, -np.inf)))
        given = ~np.isnan(self.time_delay_h0)
        lam = np.full(len(weights), np.nan)
        lam[given] = hubble_distance_mpc(self.time_delay_h0[given]) * LensSimulator.DAYS_PER_MPC_ARCSEC2
        return np.stack([g for g, _ in weights], axis=0), np.asarray(weights[far][1], dtype=np.float64), lam.astype(np.float32)

    def _delay_entry(self, simulator):
        """The native entry of the time-delay term alone, bound: gl_multiplane_position_delays_fwd_bwd for a model built with
        ``time_delay_h0`` (lens planes), gl_position_delays_fwd_bwd otherwise."""
        if self.time_delay_h0 is not None:
            self._on_planes(simulator)  # (its refusals)
            return self._bind_positions(simulator).multiplane_position_delays
        return self._bind_positions(simulator).position_delays

    def _on_planes(self, simulator):
        """True for a simulator with several lens planes, whose fused log-probability comes from the multi-plane entries.  A model
        that carries image positions is served there when its families have redshifts (``centroids_redshifts``); without them it is
        refused -- a family names no plane."""
        mp = simulator._mp
        if mp is None:
            return False
        if not (self.include_pixels or self.include_positions):
            raise _native.UnsupportedLensError(f"a model with {mp.K} lens planes and no likelihood term")
        if self.include_positions and self.centroids_redshifts is None:
            raise _native.UnsupportedLensError(f"a model with {mp.K} lens planes traces an image family through the planes in front of "
                                               "it: its image positions need centroids_redshifts (or include_positions=False); a "
                                               "family without a redshift names no plane")
        return True

    def _fused(self, simulator, z, want_grad, terms):
        """``(log_prob, log_like, red_chi2, d log_prob / d z or None)`` of ``terms`` (1 pixels, 2 image positions, 3 both): bijector ->
        prep -> fused render/chi2/VJP -> finalize + prior, all inside the native library.  The one place that binds this model to
        the simulator's native model and calls its fused entry; the reduced chi^2 of the pixels divides by the region's pixel count
        (the library does not look at the divisor without the pixel term)."""
        on_planes = self._on_planes(simulator)
        model = self._bind_prior(simulator)
        if terms & 2:
            self._bind_positions(simulator)
        entry = model.multiplane_logprob if on_planes else model.logprob
        return entry(z.detach(), self.observed_image, self.error_map, self._mask(simulator), self.background_rms or 0.0,
                     self.exp_time or 1.0, want_grad, self._n_eff(simulator) if terms & 1 else 1.0, terms)

    def _terms(self):
        return (1 if self.include_pixels else 0) | (2 if self.include_positions else 0)

    def _mask(self, simulator):
        return simulator.img_region if simulator.sim_config.pix_region is not None else None

    def stats_positions(self, simulator, params):
        """tf/model.py:103-124: ``(log_like, red_chi2)`` of the image-position term."""
        packed = params if torch.is_tensor(params) else simulator.pack(params)
        on_planes = self.centroids_x is not None and self._on_planes(simulator)
        model = self._bind_positions(simulator)
        ll, chi2 = _point_term(packed, model.multiplane_positions if on_planes else model.positions)
        return ll, chi2 / self.n_position

    def _need_fluxes(self, what):
        if not self.n_flux:
            raise ValueError(f"{what} needs a model built with centroids_fluxes / centroids_fluxes_errors")

    def stats_fluxes(self, simulator, params):
        """``(log_like, chi2 / n_flux)`` of the flux-ratio term alone (beyond the reference; see ``centroids_fluxes``), differentiable
        in packed ``params``.  On lens planes the families need ``centroids_redshifts``, as in ``stats_positions``."""
        self._need_fluxes("stats_fluxes")
        packed = params if torch.is_tensor(params) else simulator.pack(params)
        self._on_planes(simulator)  # (its refusals; one native entry serves one plane and lens planes)
        ll, chi2 = _point_term(packed, self._bind_positions(simulator).position_fluxes)
        return ll, chi2 / self.n_flux

    def predicted_fluxes(self, simulator, params):
        """``(amplitude [B, F], model_flux [B, J])``: the profiled unlensed flux ``S_f`` of every family and the fluxes ``S_f |mu_j|`` the
        model gives its images, in the concatenated image order; NaN for a family without fluxes.  Forward only."""
        self._need_fluxes("predicted_fluxes")
        packed = params if torch.is_tensor(params) else simulator.pack(params)
        if packed.requires_grad:
            raise NotImplementedError("predicted_fluxes is a forward-only diagnostic (no gradient)")
        self._on_planes(simulator)
        return self._bind_positions(simulator).position_fluxes(packed, False, want_model=True)[3:]

    def _need_delays(self, what):
        if not self.n_delay:
            raise ValueError(f"{what} needs a model built with centroids_time_delays / centroids_time_delays_errors")

    def stats_time_delays(self, simulator, params):
        """``(log_like, chi2 / n_delay)`` of the time-delay term alone (beyond the reference; see ``centroids_time_delays``),
        differentiable in packed ``params``.  One lens plane, lenses with a potential, families with delays on the reference plane;
        or, for a model built with ``time_delay_h0``, two to four lens planes."""
        self._need_delays("stats_time_delays")
        packed = params if torch.is_tensor(params) else simulator.pack(params)
        ll, chi2 = _point_term(packed, self._delay_entry(simulator))
        return ll, chi2 / self.n_delay

    def fitted_time_delays(self, simulator, params):
        """``(D_dt [B, F], offset [B, F], model_delay [B, J])``: the time-delay distance of every family in Mpc -- the one given, or
        the profiled ``lambda_f / DAYS_PER_MPC_ARCSEC2`` --, the fitted zero ``T_f`` of its clock in days and the arrival times
        ``lambda_f phi_j + T_f`` the model gives its images, in the concatenated image order; NaN for a family without delays.
        Forward only.  A model built with ``time_delay_h0`` (lens planes): the first entry is ``c / H0`` of every family in Mpc, given
        or fitted -- ``fitted_h0`` turns it into H0."""
        self._need_delays("fitted_time_delays")
        packed = params if torch.is_tensor(params) else simulator.pack(params)
        if packed.requires_grad:
            raise NotImplementedError("fitted_time_delays is a forward-only diagnostic (no gradient)")
        lam, off, md = self._delay_entry(simulator)(packed, False, want_model=True)[3:]
        from gigalens_amd.simulator import LensSimulator
        return lam / LensSimulator.DAYS_PER_MPC_ARCSEC2, off, md

    def fitted_h0(self, simulator, params):
        """``H0 [B, F]`` in km/s/Mpc of a model built with ``time_delay_h0``: the one given, or ``c`` over the profiled ``c / H0`` of
        ``fitted_time_delays``; NaN for a family without delays.  A negative or huge value is data, not an error.  Forward only."""
        if self.time_delay_h0 is None:
            raise ValueError("fitted_h0 needs a model built with time_delay_h0 (one plane: fitted_time_delays gives D_dt)")
        from gigalens_amd.cosmology import C_KM_S
        return C_KM_S / self.fitted_time_delays(simulator, params)[0]

    def _point_stats(self, simulator, packed):
        """``(log_like, red_chi2)`` of the point-image term: the image positions and, when the model has them, the flux ratios and
        the time delays -- ``red_chi2 = (chi2_pos + chi2_flux + chi2_delay) / (n_position + n_flux + n_delay)``."""
        ll, red = self.stats_positions(simulator, packed)
        if not (self.n_flux or self.n_delay):  # the positions alone: the reference's expression, bit for bit
            return ll, red
        # (with fluxes alone this is (red n_position + red_flux n_flux) / (n_position + n_flux), operation for operation)
        chi2, n = red * self.n_position, self.n_position
        if self.n_flux:
            ll_f, red_f = self.stats_fluxes(simulator, packed)
            ll, chi2, n = ll + ll_f, chi2 + red_f * self.n_flux, n + self.n_flux
        if self.n_delay:
            ll_d, red_d = self.stats_time_delays(simulator, packed)
            ll, chi2, n = ll + ll_d, chi2 + red_d * self.n_delay, n + self.n_delay
        return ll, chi2 / n

    def predicted_positions(self, simulator, params, **solver_kwargs):
        """Images the model predicts for every family of ``centroids_x/y`` (beyond the reference).  The source of a family is
        the barycentre of its back-traced observed images, the same mean beta ``stats_positions`` compares against.  Returns
        one ``(x, y, mu, n)`` tuple per family with ``[B, max_images]`` / ``[B]`` tensors (``LensSimulator.image_positions``,
        which ``solver_kwargs`` go to)."""
        if self.centroids_x is None:
            raise ValueError("predicted_positions needs a model built with centroids_x/centroids_y")
        packed = params if torch.is_tensor(params) else simulator.pack(params)
        sx, sy = self._family_sources(simulator, packed)
        scales, given = self._family_scales(simulator)
        if given:  # every family on its own plane
            solver_kwargs = dict(solver_kwargs, deflection_scale=scales)
        x, y, mu, n = simulator.image_positions(packed, sx, sy, **solver_kwargs)
        return [(x[:, f], y[:, f], mu[:, f], n[:, f]) for f in range(len(self.centroids_x))]

    def _family_sources(self, simulator, packed):
        """Source of every family: the barycentre of its back-traced observed images (on the family's own plane), ``[B, F]`` x and y."""
        sx, sy = [], []
        for cx, cy, c in zip(self.centroids_x, self.centroids_y, self._family_scales(simulator)[0]):
            maps = simulator._model.lens_maps(packed, cx.reshape(-1, 1), cy.reshape(-1, 1))  # (6, J_f, B)
            bx, by = maps[0], maps[1]
            if c != 1.0:  # beta = theta + c (beta_1 - theta)
                tx = torch.as_tensor(cx.reshape(-1, 1), device=bx.device)
                ty = torch.as_tensor(cy.reshape(-1, 1), device=bx.device)
                bx, by = tx + float(c) * (bx - tx), ty + float(c) * (by - ty)
            sx.append(bx.mean(dim=0))
            sy.append(by.mean(dim=0))
        return torch.stack(sx, dim=1), torch.stack(sy, dim=1)

    def predicted_time_delays(self, simulator, params, time_delay_distance=None, h0=None, **solver_kwargs):
        """Images and arrival-time delays the model predicts for every family (beyond the reference), for the same barycentre
        source as ``predicted_positions``.  Returns one ``(x, y, mu, n, dt)`` tuple per family, ``dt`` ``[B, max_images]`` relative
        to the family's first-arriving image, in arcsec^2 of Fermat potential or, with ``time_delay_distance`` (D_dt in Mpc, a
        scalar or ``[B]``), in days (``LensSimulator.time_delays``, which ``solver_kwargs`` go to).  Forward only.

        A model built with ``centroids_redshifts`` on a one-plane ``MultiPlane`` goes through ``time_delays(source_redshifts=...)``,
        every family on its own scaled plane: ``dt`` in arcsec^2 times ``c / H0``, or in days with ``h0`` (km/s/Mpc); it takes no
        ``time_delay_distance``.  On several lens planes the call stays refused, as ``predicted_positions``."""
        if self.centroids_x is None:
            raise ValueError("predicted_time_delays needs a model built with centroids_x/centroids_y")
        scales = self._family_scales(simulator)[0]  # (lens planes: its UnsupportedLensError)
        by_redshift = self.centroids_redshifts is not None
        if not by_redshift:
            if h0 is not None:
                raise ValueError("predicted_time_delays: h0 serves families placed by centroids_redshifts; give time_delay_distance")
            if np.any(scales != 1.0):
                raise NotImplementedError("predicted_time_delays: the Fermat potential of a scaled source plane (centroids_scales != 1) "
                                          "is not served without redshifts (centroids_redshifts)")
        packed = params if torch.is_tensor(params) else simulator.pack(params)
        if packed.requires_grad:
            raise NotImplementedError("predicted_time_delays is a forward-only diagnostic (no gradient)")
        sx, sy = self._family_sources(simulator, packed)
        if by_redshift:
            x, y, mu, n, dt = simulator.time_delays(packed, sx, sy, source_redshifts=self.centroids_redshifts, h0=h0,
                                                    time_delay_distance=time_delay_distance, **solver_kwargs)
        else:
            x, y, mu, n, dt = simulator.time_delays(packed, sx, sy, time_delay_distance=time_delay_distance, **solver_kwargs)
        return [(x[:, f], y[:, f], mu[:, f], n[:, f], dt[:, f]) for f in range(len(self.centroids_x))]

    def image_plane_rms(self, simulator, params, **solver_kwargs):
        """Image-plane rms of every family (beyond the reference; the Delta theta cluster papers report): each observed image,
        in the order given, is paired with the nearest predicted image not yet paired.  Returns a dict of ``[B, F]`` tensors:
        ``rms`` (inf where fewer images are predicted than observed), ``n_predicted``, ``n_observed`` and ``counts_match``;
        samples whose counts differ are reported there, not left out."""
        fams = self.predicted_positions(simulator, params, **solver_kwargs)
        rms, n_pred, n_obs = [], [], []
        for (px, py, _, n), cx, cy in zip(fams, self.centroids_x, self.centroids_y):
            ox = torch.as_tensor(cx, device=px.device)
            oy = torch.as_tensor(cy, device=px.device)
            d = torch.hypot(px[:, None, :] - ox[None, :, None], py[:, None, :] - oy[None, :, None])  # [B, J, M]
            d = torch.nan_to_num(d, nan=float("inf"))
            used = torch.zeros_like(d[:, 0, :], dtype=torch.bool)
            ss = torch.zeros_like(d[:, 0, 0])
            for j in range(d.shape[1]):
                dj = d[:, j, :].masked_fill(used, float("inf"))
                k = dj.argmin(dim=1, keepdim=True)
                ss = ss + dj.gather(1, k)[:, 0] ** 2
                used = used.scatter(1, k, True)
            rms.append(torch.sqrt(ss / d.shape[1]))
            n_pred.append(n)
            n_obs.append(torch.full_like(n, int(cx.size)))
        n_pred, n_obs = torch.stack(n_pred, dim=1), torch.stack(n_obs, dim=1)
        return {"rms": torch.stack(rms, dim=1), "n_predicted": n_pred, "n_observed": n_obs, "counts_match": n_pred == n_obs}

    def _packed_from_x(self, simulator, x):
        cols, consts = self._perm(simulator)
        if consts.numel():
            x = torch.cat([x, consts.expand(x.shape[0], -1)], dim=1)
        return x.index_select(1, cols)

    def _pixel_stats_packed(self, simulator, packed):
        inputs = (self.observed_image, self.error_map, self._mask(simulator), self.background_rms or 0.0, self.exp_time or 1.0)
        if simulator._mp is not None:  # lens planes: the forward image through the image-statistics launch
            if packed.requires_grad:
                raise NotImplementedError("the pixel statistics of a model with several lens planes carry no autograd graph: the "
                                          "gradient entries are log_prob / log_prob_and_grad and _model.multiplane_loglike_grad")
            ll, chi2 = simulator._model.multiplane_loglike(packed, *inputs)
        else:
            ll, chi2 = _log_like(packed, simulator._model, *inputs)
        return ll, chi2 / self._n_eff(simulator)  # tf/model.py:100

    def stats_pixels(self, simulator, params):
        """tf/model.py:89-101: ``params`` is the nested constrained structure."""
        return self._pixel_stats_packed(simulator, simulator.pack(params))

    def _fused_ok(self, simulator):
        """False for a model with neither likelihood term: the prior alone comes from torch ops (``log_prob_unfused``)."""
        return self.include_pixels or self.include_positions

    def log_prob(self, simulator, z):
        """tf/model.py:126-167: ``z`` is ``(bs, d)`` unconstrained; returns ``(log_prob, red_chi2)``."""
        z = torch.as_tensor(z, dtype=torch.float32, device=self.device)
        terms = self._terms()
        if not terms and not self._on_planes(simulator):  # (lens planes refuse a model without a term)
            return self.log_prob_unfused(simulator, z)
        # (bijector + kernels + prior in one native launch sequence; forward only when z needs no gradient)
        lp, _, red_chi2 = _GradFn.apply(lambda zz, want: _split(self._fused(simulator, zz, want, terms)), z)
        return lp, red_chi2

    def term_log_prob_and_grad(self, simulator, z, term):
        """``(log_prior + log_like_term, log_like_term, gradient of the former w.r.t. z)`` for ONE likelihood term
        (``"pixels"`` or ``"positions"``) -- the pieces the tempered SMC target is assembled from
        (tf/inference.py:213-238,292-303)."""
        z = torch.as_tensor(z, dtype=torch.float32, device=self.device)
        if self._on_planes(simulator) and term == "positions" and not self.include_positions:
            raise _native.UnsupportedLensError("the model carries no image positions: on lens planes the position term needs "
                                               "centroids_x/centroids_y with centroids_redshifts")
        lp, ll, _, grad = self._fused(simulator, z, True, {"pixels": 1, "positions": 2}[term])
        return lp, ll, grad

    def log_prob_and_grad(self, simulator, z, graph=False):
        """``(log_prob, red_chi2, d log_prob / d z)`` from ONE native launch sequence and no autograd graph --
        what one MAP / HMC-leapfrog step of the reference computes with ``tf.GradientTape`` (tf/inference.py:33-39).

        ``graph=True`` (small problems, where the three to seven short launches of a step are host-issue bound -- BASELINE
        configs[0], one 64 x 64 sample: 7 us of kernels in a 21 us step): the launch sequence is captured once per
        (simulator, shape of ``z``) in a HIP graph and replayed.  The contract is that of torch's CUDA graphs: the three returned
        tensors are the graph's STATIC outputs, overwritten by the next call with ``graph=True`` on the same simulator; ``z`` is
        copied into the graph's static input unless it already IS that tensor (``graph_input(simulator, z)`` hands it out, for loops
        that update ``z`` in place).  Anything that re-binds the simulator's native model (another ``ForwardProbModel``, any of its
        ``set_*``) makes the next call capture again, so two models alternating on one simulator with ``graph=True`` capture on
        every call."""
        z = torch.as_tensor(z, dtype=torch.float32, device=self.device)
        terms = self._terms()
        if not terms and not self._on_planes(simulator):
            zz = z.detach().requires_grad_(True)
            lp, red = self.log_prob_unfused(simulator, zz)
            (g,) = torch.autograd.grad(lp.sum(), zz)
            return lp.detach(), red.detach(), g
        if graph and z.is_cuda:
            return self._log_prob_and_grad_graph(simulator, z).outs
        lp, _, red, grad = self._fused(simulator, z, True, terms)
        return lp, red, grad

    def _log_prob_and_grad_graph(self, simulator, z):
        """The graph of this shape of ``z``, replayed on ``z``: captured on first use, and again when its entry no longer holds."""
        key = (id(self), z.shape)  # (the entry keeps self, so its id is not reused while the entry lives)
        ent = simulator._lp_graphs.get(key)
        if ent is None or not ent.valid(simulator):
            z_static = z.detach().clone().contiguous() if ent is None else ent.z_static  # (graph_input's tensor stays the input)
            if z is not z_static and z.data_ptr() != z_static.data_ptr():
                z_static.copy_(z.detach())
            terms = self._terms()
            side = torch.cuda.Stream(device=z.device)
            side.wait_stream(torch.cuda.current_stream(z.device))
            with torch.cuda.stream(side):  # warm-up off the default stream: binds the prior, sizes the workspaces
                for _ in range(2):
                    self._fused(simulator, z_static, True, terms)
            torch.cuda.current_stream(z.device).wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                lp, _, red, grad = self._fused(simulator, z_static, True, terms)
            ent = simulator._lp_graphs[key] = _GraphEntry(g, z_static, (lp, red, grad), self, simulator, terms)
            simulator._lp_captures += 1
        elif z is not ent.z_static and z.data_ptr() != ent.z_static.data_ptr():
            ent.z_static.copy_(z.detach())
        ent.graph.replay()
        return ent

    def graph_input(self, simulator, z):
        """The static input tensor of ``log_prob_and_grad(..., graph=True)`` for this shape of ``z`` (created, and the graph
        captured, on first use), initialised with ``z``: update it in place and pass it back to skip the copy."""
        z = torch.as_tensor(z, dtype=torch.float32, device=self.device)
        return self._log_prob_and_grad_graph(simulator, z).z_static

    def _n_eff(self, simulator):
        n = simulator._n_eff
        if n is None:
            n = simulator._n_eff = float(torch.count_nonzero(simulator.img_region))
        return n

    def log_prob_unfused(self, simulator, z):
        """Same quantity with the bijector and prior evaluated by torch ops around the likelihood kernels
        (kept as the cross-check of the fused native path and for configurations it does not cover)."""
        z = torch.as_tensor(z, dtype=torch.float32, device=self.device)
        x = self._flat.forward(z)
        log_like = torch.zeros(z.shape[0], dtype=torch.float32, device=self.device)
        red_chi2 = torch.zeros_like(log_like)
        n_chi = 0
        packed = self._packed_from_x(simulator, x)
        if self.include_pixels:
            ll, rc = self._pixel_stats_packed(simulator, packed)
            log_like = log_like + ll
            red_chi2 = red_chi2 + rc
            n_chi += 1
        if self.include_positions:
            ll, rc = self._point_stats(simulator, packed)
            log_like = log_like + ll
            red_chi2 = red_chi2 + rc
            n_chi += 1
        red_chi2 = red_chi2 / max(n_chi, 1)
        log_prior = self._flat.log_prob(x) + self._flat.fldj_columns(z).sum(-1)
        return log_like + log_prior, red_chi2

    def log_like(self, simulator, z):
        """tf/model.py:169-180."""
        z = torch.as_tensor(z, dtype=torch.float32, device=self.device)
        x = self._flat.forward(z)
        ll = torch.zeros(z.shape[0], dtype=torch.float32, device=self.device)
        packed = self._packed_from_x(simulator, x)
        if self.include_pixels:
            ll = ll + self._pixel_stats_packed(simulator, packed)[0]
        if self.include_positions:
            ll = ll + self._point_stats(simulator, packed)[0]
        return ll


class BackwardProbModel(_StreamProbModel):
    """Drop-in for ``gigalens.tf.model.BackwardProbModel`` (tf/model.py:197-273): the noise map comes from the
    OBSERVED image, and the linear light amplitudes are solved by least squares inside the likelihood.

    The reference differentiates through ``tf.linalg.pinv``; here the gradient uses the envelope property of the
    solve -- the coefficients minimise exactly the chi^2 that the (fixed-noise) log-likelihood is made of, so
    ``d log_like / d theta`` equals the partial derivative at fixed coefficients, which the fused forward+gradient
    kernels evaluate with the solved amplitudes written into their columns (equal to the reference's total derivative
    wherever the normal matrix has full rank above the ``rcond`` cut)."""

    def __init__(self, prior, observed_image, background_rms, exp_time):
        super().__init__(prior)
        obs = np.asarray(observed_image, dtype=np.float32)
        err = np.sqrt(np.float32(background_rms) ** 2 + np.clip(obs, 0, np.inf) / np.float32(exp_time)).astype(np.float32)
        self.observed_image = torch.as_tensor(obs, device=self.device).contiguous()
        self.err_map = torch.as_tensor(err, device=self.device).contiguous()
        self._bind_prior_structure(prior)

    def log_prob(self, simulator, z):
        """tf/model.py:242-273: ``(log_like + log_prior, mean squared normalised residual)``."""
        z, x, log_prior = self._x_and_log_prior(z)
        packed = simulator.pack(self.pack_bij.forward(x))
        coeffs = simulator._model.lstsq(packed.detach(), self.observed_image, self.err_map, 7, want="coeffs")[0]
        lin = simulator._linear_cols_dev  # uploaded once per simulator, not per call
        if lin is None or lin.device != packed.device:
            lin = simulator._linear_cols_dev = torch.tensor(simulator._layout.linear, dtype=torch.int64, device=packed.device)
        full = packed.index_copy(1, lin, coeffs / simulator.conversion_factor)  # amplitude = coeff / det(T)
        ll, chi2 = _log_like(full, simulator._model, self.observed_image, self.err_map, None, 0.0, 1.0)
        return ll + log_prior, chi2 / float(self.observed_image.numel())


class SourceEvidenceProbModel(_StreamProbModel):
    """The Bayesian evidence of a pixelated source as the target of ``ModellingSequence.MAP / SVI / HMC`` (beyond the reference):
    ``log_prob = log_evidence + log_prior`` of ``LensSimulator.reconstruct_source`` at one regularisation strength, with the
    hand-written gradient of ``LensSimulator.source_evidence_and_grad``.  The prior is over ``lens_mass``, and over ``lens_light``
    where the model has lens light; the model's ``source_light`` is replaced by the source grid (``n_src``, ``pitch``, ``center``,
    as in ``reconstruct_source``).  The evidence is continuous but only piecewise smooth in the lens (a kink wherever a ray crosses
    a source-grid line); its gradient is taken with the set of finite rays held fixed.  Runs on the stream path."""

    def __init__(self, prior, observed_image, err_map, *, n_src, pitch, center=(0.0, 0.0), regularization="gradient", strength=1.0,
                 mask=None):
        super().__init__(prior)
        self.observed_image = torch.as_tensor(np.asarray(observed_image, dtype=np.float32), device=self.device).contiguous()
        self.err_map = torch.as_tensor(np.asarray(err_map, dtype=np.float32), device=self.device).contiguous()
        self.n_src, self.pitch, self.center = (int(n_src[0]), int(n_src[1])), pitch, tuple(center)
        self.regularization, self.strength = regularization, strength
        self.mask = None if mask is None else np.asarray(mask.cpu() if torch.is_tensor(mask) else mask).astype(bool)
        self._bind_prior_structure(prior)

    def _n_used(self, simulator):
        used = np.asarray(simulator.img_region.cpu()) != 0
        return int((used & self.mask).sum() if self.mask is not None else used.sum())

    def log_prob(self, simulator, z):
        """``(log_evidence + log_prior, chi2 / n_used)``; differentiable with respect to ``z``."""
        z, x, log_prior = self._x_and_log_prior(z)
        packed = simulator._pack_partial(self.pack_bij.forward(x))  # missing groups filled; torch.stack keeps the graph
        evidence = lambda p, _: _from_dict(simulator.source_evidence_and_grad(
            p, self.observed_image, self.err_map, n_src=self.n_src, pitch=self.pitch, center=self.center,
            regularization=self.regularization, strength=self.strength, mask=self.mask), ("log_evidence", "chi2"))
        ev, chi2 = _GradFn.apply(evidence, packed)
        return ev + log_prior, chi2 / float(self._n_used(simulator))


class _SourcePlaneTieFn(torch.autograd.Function):
    """``-1/2 sum_j |beta_j - mean beta|^2 / sigma^2`` of the images' source-plane positions ``beta_j`` (``lens_maps`` at
    ``(x_j, y_j)``).  Gradient from existing entries: the cotangent ``-(beta_j - mean beta) / sigma^2`` goes through
    ``lens_maps_vjp`` to the lens columns and through ``(I - H_j)^T`` (``H_j`` the Hessian ``lens_maps`` returns) to the positions."""

    @staticmethod
    def forward(ctx, packed, x, y, simulator, sigma):
        xp, yp = x.detach().t().contiguous(), y.detach().t().contiguous()  # [J, B]: the point layout of the lens maps
        maps = simulator._lens_maps(xp, yp, packed.detach())
        bx, by = maps[0].double(), maps[1].double()
        cx, cy = -(bx - bx.mean(dim=0, keepdim=True)) / sigma ** 2, -(by - by.mean(dim=0, keepdim=True)) / sigma ** 2
        ctx.simulator = simulator
        ctx.save_for_backward(packed.detach(), xp, yp, cx.float(), cy.float(), maps[2:])
        return (-0.5 * sigma ** 2 * (cx * cx + cy * cy).sum(dim=0)).float()

    @staticmethod
    def backward(ctx, g):
        packed, xp, yp, cx, cy, h = ctx.saved_tensors
        g_packed = ctx.simulator.beta_vjp(xp, yp, packed, cx, cy)
        gx = (1.0 - h[0]) * cx - h[2] * cy  # (I - H)^T (cx, cy), H = [[f_xx, f_xy], [f_yx, f_yy]]
        gy = -h[1] * cx + (1.0 - h[3]) * cy
        return g[:, None] * g_packed, g[:, None] * gx.t(), g[:, None] * gy.t(), None, None


class PointImageProbModel(_StreamProbModel):
    """The pixel likelihood of an extended model plus the PSF-rendered images of a lensed point source (quasar, supernova) as the
    target of ``ModellingSequence.MAP / SVI / HMC`` (beyond the reference): ``log_prob = log_like + log_prior`` of
    ``LensSimulator.fit_point_images``, where the amplitudes of the images are solved per sample, with the hand-written gradient
    of ``LensSimulator.point_image_log_like_and_grad``.

    The prior's structure carries one group beside the model's own: ``"point_images": [{"x": ..., "y": ...}] * J`` (``J <= 8``), the
    image positions in arcsec.  ``source_plane_sigma`` (arcsec, optional) ties the images to one source and so lets them constrain
    the lens: with ``beta_j`` the source-plane position of image ``j`` and ``mean beta`` their plain mean it adds
    ``-1/2 sum_j |beta_j - mean beta|^2 / sigma^2 - (J - 1) log(2 pi sigma^2)``.  Lenses ``lens_maps`` / ``lens_maps_vjp`` refuse
    stay refused with their error.  A sample whose fit is singular (``ok == False``) has a NaN ``log_prob``.  Runs on the stream
    path (``MAP(graph=True)`` falls back to it)."""

    def __init__(self, prior, observed_image, err_map, *, mask=None, source_plane_sigma=None):
        super().__init__(prior)
        self.observed_image = torch.as_tensor(np.asarray(observed_image, dtype=np.float32), device=self.device).contiguous()
        self.err_map = torch.as_tensor(np.asarray(err_map, dtype=np.float32), device=self.device).contiguous()
        self.mask = None if mask is None else torch.as_tensor(np.asarray(mask.cpu() if torch.is_tensor(mask) else mask).astype(bool),
                                                              device=self.device)
        self._n_used_of = weakref.WeakKeyDictionary()  # per simulator: the number of used pixels
        if source_plane_sigma is not None:
            source_plane_sigma = float(source_plane_sigma)
            if not (np.isfinite(source_plane_sigma) and source_plane_sigma > 0):
                raise ValueError(f"source_plane_sigma must be finite and > 0, got {source_plane_sigma}")
        self.source_plane_sigma = source_plane_sigma
        example = self._bind_prior_structure(prior)
        images = example.get("point_images") if isinstance(example, dict) else None
        if not images or any(set(d) != {"x", "y"} for d in images):
            raise ValueError('the prior needs a group "point_images": a list of {"x": ..., "y": ...}, one per image')
        if len(images) > 8:
            raise ValueError(f"{len(images)} point images: at most 8 are served")
        self.n_images = len(images)

    def _n_used(self, simulator):
        if simulator not in self._n_used_of:
            used = simulator.img_region != 0
            self._n_used_of[simulator] = int((used & self.mask.to(used.device)).sum() if self.mask is not None else used.sum())
        return self._n_used_of[simulator]

    def log_prob(self, simulator, z):
        """``(log_like + source-plane tie + log_prior, chi2 / n_used)``; differentiable with respect to ``z``."""
        z, x, log_prior = self._x_and_log_prior(z)
        struct = self.pack_bij.forward(x)
        packed = simulator._pack_partial(struct)  # groups outside the layout are ignored; torch.stack keeps the graph
        px = torch.stack([d["x"] for d in struct["point_images"]], dim=1)
        py = torch.stack([d["y"] for d in struct["point_images"]], dim=1)
        fit = lambda p, ix, iy, _: _from_dict(simulator.point_image_log_like_and_grad(
            p, ix, iy, self.observed_image, self.err_map, mask=self.mask), ("log_like", "chi2"), ("grad", "grad_x", "grad_y"))
        ll, chi2 = _GradFn.apply(fit, packed, px, py)
        lp = ll + log_prior
        if self.source_plane_sigma is not None:
            s = self.source_plane_sigma
            lp = lp + _SourcePlaneTieFn.apply(packed, px, py, simulator, s) - (self.n_images - 1) * math.log(2.0 * math.pi * s * s)
        return lp, chi2 / float(self._n_used(simulator))


class ShearCatalogue:
    """The weak-lensing catalogue of ``WeakLensingProbModel`` and ``LensSimulator.shear_log_like_and_grad``: ``N`` background
    galaxies at ``(x, y)`` (arcsec) with measured ellipticity components ``(e1, e2)``, their error ``sigma`` per component and the
    deflection scale of every galaxy's own redshift (``gigalens_amd.cosmology.deflection_scale``; default 1: the model's reference
    plane).  Everything is held as float32 ``[N]``; ``sigma`` and ``scales`` broadcast.  ``ValueError``: a shape mismatch, an
    entry that is not finite, a ``sigma`` or a scale that is not finite and > 0."""

    def __init__(self, x, y, e1, e2, sigma, scales=None):
        x = np.atleast_1d(np.asarray(x, dtype=np.float32))
        if x.ndim != 1 or x.size == 0:
            raise ValueError(f"ShearCatalogue: x must be a non-empty 1-D array, got shape {tuple(x.shape)}")
        n = x.size
        tabs = {"x": x}
        for name, v in (("y", y), ("e1", e1), ("e2", e2)):
            v = np.atleast_1d(np.asarray(v, dtype=np.float32))
            if v.shape != (n,):
                raise ValueError(f"ShearCatalogue: {name} has shape {tuple(v.shape)}, x has {(n,)}")
            tabs[name] = v
        for name, v in (("sigma", sigma), ("scales", scales)):
            if v is None and name == "scales":
                tabs[name] = None
                continue
            v = np.asarray(v, dtype=np.float32)
            if v.ndim > 1 or (v.ndim == 1 and v.size not in (1, n)):
                raise ValueError(f"ShearCatalogue: {name} has shape {tuple(v.shape)}: a scalar or {(n,)}")
            v = np.broadcast_to(v.reshape(-1) if v.ndim else v, (n,)).copy()
            if not (np.all(np.isfinite(v)) and np.all(v > 0)):
                raise ValueError(f"ShearCatalogue: every entry of {name} must be finite and > 0")
            tabs[name] = v
        for name in ("x", "y", "e1", "e2"):
            if not np.all(np.isfinite(tabs[name])):
                raise ValueError(f"ShearCatalogue: {name} holds an entry that is not finite")
        self.n = n
        self.x, self.y, self.e1, self.e2, self.sigma, self.scales = (tabs[k] for k in ("x", "y", "e1", "e2", "sigma", "scales"))
        self._dev = {}

    def __len__(self):
        return self.n

    def device_tables(self, device):
        """The arrays as device tensors (uploaded once per device); ``scales`` stays None when it was not given."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = {k: None if v is None else torch.as_tensor(v, device=device).contiguous()
                              for k, v in (("x", self.x), ("y", self.y), ("e1", self.e1), ("e2", self.e2), ("sigma", self.sigma),
                                           ("scales", self.scales))}
        return self._dev[key]


class WeakLensingProbModel(_JoinsStrong):
    """The weak-lensing shear of a ``ShearCatalogue`` as the target of ``ModellingSequence.MAP / SVI / HMC`` (beyond the reference):
    ``log_prob = log_like + log_prior`` of ``LensSimulator.shear_log_like_and_grad`` with its hand-written gradient.  The prior is
    over ``lens_mass`` (groups the physical model has beside it are packed from the prior when it carries them).

    ``strong``: a ``ForwardProbModel`` over the SAME prior -- pixels, image positions, flux ratios, time delays -- whose ``log_prob``
    is added for a joint strong + weak fit; the prior is counted once (inside ``strong``'s term).  The reduced chi^2 is then
    ``(chi2_shear + red_strong n_strong) / (2 N + n_strong)`` with ``n_strong = strong._n_eff(simulator)``; without ``strong`` it is
    ``chi2_shear / (2 N)``.  Lenses ``hessian_vjp`` refuses stay refused with their error.  Runs on the stream path
    (``MAP(graph=True)`` falls back to it)."""

    def __init__(self, prior, catalogue, strong=None):
        super().__init__(prior)
        if not isinstance(catalogue, ShearCatalogue):
            raise TypeError("catalogue must be a ShearCatalogue")
        self._bind_strong(strong, 2.0 * catalogue.n)  # the 2 N ellipticity components
        self.catalogue = catalogue
        self._bind_prior_structure(prior)

    def log_prob(self, simulator, z):
        """``(log_like + log_prior [+ strong's log_like], reduced chi^2)``; differentiable with respect to ``z``."""
        z = torch.as_tensor(z, dtype=torch.float32, device=self.device)
        x = self._flat.forward(z)
        packed = simulator._pack_partial(self.pack_bij.forward(x))  # missing groups filled; torch.stack keeps the graph
        shear = lambda p, _: _from_dict(simulator.shear_log_like_and_grad(p, self.catalogue, want_grad=True), ("log_like", "chi2"))
        ll, chi2 = _GradFn.apply(shear, packed)
        return self._join(simulator, z, x, ll, chi2, 2.0 * self.catalogue.n)


class ImageFamilies:
    """The image families of ``ImagePlaneProbModel`` and ``LensSimulator.image_plane_log_like_and_grad``: ``x, y`` are lists with one
    array of observed image positions (arcsec) per family, shaped like ``centroids_x / centroids_y`` of ``ForwardProbModel``;
    ``sigma`` the isotropic position error -- a scalar, one value per family, or one array per family; ``scales`` one deflection
    scale per family (``gigalens_amd.cosmology.deflection_scale``; default 1: the model's reference plane).

    ``max_shift``: the cap of every image -- the furthest its predicted image may lie from it, and the longest Newton step towards it.
    Default: half the distance to the nearest sibling of its family (float64 on the host, stored as float32), so the balls of two
    siblings at most touch and two observed images never claim the same predicted one.  A scalar, or one array per family (a flat
    array over all images is taken too), overrides it; a family of one image needs it.

    Everything is held concatenated family by family as float32 ``[J]``.  ``ValueError``: a shape mismatch, an entry that is not
    finite, a ``sigma``, scale or ``max_shift`` that is not finite and > 0, two coincident images in a family, a family of more than
    64 images, a family of one image without ``max_shift``."""

    MAX_FAMILY = 64

    def __init__(self, x, y, sigma, scales=None, max_shift=None):
        if isinstance(x, np.ndarray) and x.ndim == 1 or not len(x):
            raise ValueError("ImageFamilies: x and y are lists with one array per family")
        xs = [np.atleast_1d(np.asarray(v, dtype=np.float32)) for v in x]
        ys = [np.atleast_1d(np.asarray(v, dtype=np.float32)) for v in y]
        if len(ys) != len(xs):
            raise ValueError(f"ImageFamilies: {len(xs)} families in x, {len(ys)} in y")
        F = len(xs)
        for f, (a, b) in enumerate(zip(xs, ys)):
            if a.ndim != 1 or a.size == 0 or a.shape != b.shape:
                raise ValueError(f"ImageFamilies: family {f}: x has shape {tuple(a.shape)}, y has {tuple(b.shape)}")
            if a.size > self.MAX_FAMILY:
                raise ValueError(f"ImageFamilies: family {f} holds {a.size} images: at most {self.MAX_FAMILY}")
            if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
                raise ValueError(f"ImageFamilies: family {f} holds a position that is not finite")
        counts = np.array([a.size for a in xs], dtype=np.int32)
        J = int(counts.sum())

        def per_image(name, v):
            """A scalar, one value per family or one array per family (or a flat ``[J]`` array) as float32 ``[J]``, finite and > 0."""
            if isinstance(v, (list, tuple)) and len(v) == F and any(np.ndim(e) > 0 for e in v):
                parts = [np.asarray(e, dtype=np.float32) for e in v]
                for f, e in enumerate(parts):
                    if e.ndim > 1 or (e.ndim == 1 and e.size not in (1, counts[f])):
                        raise ValueError(f"ImageFamilies: {name} of family {f} has shape {tuple(e.shape)}: a scalar or {(int(counts[f]),)}")
                out = np.concatenate([np.broadcast_to(e.reshape(-1) if e.ndim else e, (counts[f],)) for f, e in enumerate(parts)])
            else:
                a = np.asarray(v, dtype=np.float32)
                if a.ndim == 0:
                    out = np.full(J, a, dtype=np.float32)
                elif a.ndim == 1 and a.size == F:
                    out = np.repeat(a, counts)
                elif a.ndim == 1 and a.size == J:
                    out = a.copy()
                else:
                    raise ValueError(f"ImageFamilies: {name} has shape {tuple(a.shape)}: a scalar, one value per family ({F}) or one "
                                     f"array per family")
            out = np.ascontiguousarray(out, dtype=np.float32)
            if not (np.all(np.isfinite(out)) and np.all(out > 0)):
                raise ValueError(f"ImageFamilies: every entry of {name} must be finite and > 0")
            return out

        self.F, self.J = F, J
        self.counts = counts
        self.offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        self.x, self.y = np.concatenate(xs), np.concatenate(ys)
        self.sigma = per_image("sigma", sigma)
        self.family_scales = _native.deflection_scales(scales, F, "ImageFamilies: scales")
        self.scales = np.repeat(self.family_scales, counts).astype(np.float32)
        half = np.full(J, np.inf)
        for f in range(F):
            a, b = xs[f].astype(np.float64), ys[f].astype(np.float64)
            if a.size < 2:
                continue
            d = np.hypot(a[:, None] - a[None, :], b[:, None] - b[None, :])
            np.fill_diagonal(d, np.inf)
            if not d.min() > 0:
                raise ValueError(f"ImageFamilies: family {f} holds two coincident images")
            half[self.offsets[f]:self.offsets[f + 1]] = 0.5 * d.min(axis=1)
        if max_shift is None:
            if counts.min() < 2:
                raise ValueError(f"ImageFamilies: family {int(np.argmin(counts))} holds one image: it has no sibling to take the "
                                 f"default max_shift from, give max_shift")
            self.max_shift = half.astype(np.float32)
        else:
            self.max_shift = per_image("max_shift", max_shift)
        self.min_count = int(counts.min())
        self.max_coordinate = float(max(np.abs(self.x).max(), np.abs(self.y).max()))
        self.norm = float(np.log(2.0 * np.pi * self.sigma.astype(np.float64) ** 2).sum())
        self._dev = {}

    def __len__(self):
        return self.J

    def device_tables(self, device):
        """The static per-image tables as device tensors (uploaded once per device): ``image`` float32 ``[5, J]`` = x, y, sigma,
        max_shift, scale; ``family`` int32 ``[3, J]`` = family, first image and count of the family of every image."""
        key = str(device)
        if key not in self._dev:
            fam = np.repeat(np.arange(self.F, dtype=np.int32), self.counts)
            image = np.stack([self.x, self.y, self.sigma, self.max_shift, self.scales]).astype(np.float32)
            family = np.stack([fam, self.offsets[:-1][fam], self.counts[fam]]).astype(np.int32)
            self._dev[key] = {"image": torch.as_tensor(image, device=device).contiguous(),
                              "family": torch.as_tensor(family, device=device).contiguous()}
        return self._dev[key]


class ImagePlaneProbModel(_JoinsStrong):
    """The image-plane position likelihood of ``ImageFamilies`` as the target of ``ModellingSequence.MAP / SVI / HMC`` (beyond the
    reference): ``log_prob = log_like + log_prior`` of ``LensSimulator.image_plane_log_like_and_grad`` with the barycentre source
    of every family and its hand-written gradient -- the stage after a source-plane fit (``ForwardProbModel``'s position term is its
    linearisation at the observed positions), started from that fit's samples.  A sample with a lost image keeps a finite
    ``log_prob``: the image sits at its cap and adds nothing to the gradient.  The prior is over ``lens_mass`` (groups the physical
    model has beside it are packed from the prior when it carries them).

    ``strong``: a ``ForwardProbModel`` over the SAME prior -- pixels, flux ratios, time delays, source-plane positions -- whose
    ``log_prob`` is added; the prior is counted once (inside ``strong``'s term).  The reduced chi^2 is then
    ``(chi2 + red_strong n_strong) / (2 J + n_strong)`` with ``n_strong = strong._n_eff(simulator)``; without ``strong`` it is
    ``chi2 / (2 J)``.  Lenses ``beta_vjp`` refuses stay refused with their error.  Runs on the stream path (``MAP(graph=True)``
    falls back to it)."""

    def __init__(self, prior, families, strong=None):
        super().__init__(prior)
        if not isinstance(families, ImageFamilies):
            raise TypeError("families must be an ImageFamilies")
        if families.min_count < 2:
            raise ValueError("ImagePlaneProbModel takes the barycentre source of every family: two or more images per family")
        self._bind_strong(strong, 2.0 * families.J)  # the 2 J image coordinates
        self.families = families
        self._bind_prior_structure(prior)

    def log_prob(self, simulator, z):
        """``(log_like + log_prior [+ strong's log_like], reduced chi^2)``; differentiable with respect to ``z``."""
        z = torch.as_tensor(z, dtype=torch.float32, device=self.device)
        x = self._flat.forward(z)
        packed = simulator._pack_partial(self.pack_bij.forward(x))  # missing groups filled; torch.stack keeps the graph
        fit = lambda p, _: _from_dict(simulator.image_plane_log_like_and_grad(p, self.families, want_grad=True), ("log_like", "chi2"))
        ll, chi2 = _GradFn.apply(fit, packed)
        return self._join(simulator, z, x, ll, chi2, 2.0 * self.families.J)
