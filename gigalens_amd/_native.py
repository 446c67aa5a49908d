"""ctypes binding of ``lib/libgigalens_hip.so`` (C ABI: ``include/gigalens_hip.h``).

PyTorch is plumbing here: it owns device memory and the stream; every number on the hot path is
produced by the HIP kernels behind this ABI.  There is deliberately no fallback -- a missing library
or a failed call raises.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p

import numpy as np
import torch

_LIB_PATH = os.environ.get("GIGALENS_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                                                           "libgigalens_hip.so")
_lib = None

GL_FLAG_SHAPELETS_INTERPOLATE = 1
GL_FLAG_INTERPOL_LINEAR = 1
GL_INTERPOL = 21
GL_INTERPOL_MASS = 14
GL_MULTIPOLE = 15


class NativeLibraryError(RuntimeError):
    pass


class UnsupportedLensError(NativeLibraryError):
    """A lens the call cannot serve (GL_EUNSUPPORTED from the lensing-potential and critical-curve calls): series expansions,
    user-written bodies and the run-time compiled ScalingRelation member loops define a deflection only, no potential, and are
    not part of the critical-curve kernels.  Also: every single-plane call on a model with several lens planes."""


class gl_component(ctypes.Structure):
    _fields_ = [("kind", c_int32), ("iparam", c_int32), ("flags", c_uint32), ("reserved", c_int32)]


class gl_zcolumn(ctypes.Structure):
    _fields_ = [("param_col", c_int32), ("bijector", c_int32), ("prior", c_int32), ("a", c_float), ("b", c_float),
                ("lo", c_float), ("hi", c_float), ("log_norm", c_float)]


class gl_workspace_layout(ctypes.Structure):
    _fields_ = [("params_offset", c_size_t), ("derived_offset", c_size_t), ("order_offset", c_size_t), ("cost_offset", c_size_t),
                ("params_count", c_size_t), ("derived_count", c_size_t), ("order_count", c_size_t), ("cost_count", c_size_t),
                ("P", c_int), ("D", c_int), ("p_off", c_int), ("d_off", c_int)]


class gl_grid(ctypes.Structure):
    _fields_ = [
        ("height", c_int32), ("width", c_int32), ("supersample", c_int32), ("n_region", c_int32),
        ("grid_x", POINTER(c_float)), ("grid_y", POINTER(c_float)), ("pix_index", POINTER(c_int32)),
        ("conversion_factor", c_float), ("psf", POINTER(c_float)), ("psf_h", c_int32), ("psf_w", c_int32),
    ]


# every symbol include/gigalens_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gl_model_create": (c_int, [POINTER(gl_component), c_int, c_int, c_int, POINTER(gl_grid), POINTER(c_void_p)]),
    "gl_model_create_user": (c_int, [POINTER(gl_component), c_int, c_int, c_int, POINTER(gl_grid), POINTER(ctypes.c_char_p), c_int,
                                     POINTER(c_void_p)]),
    "gl_model_destroy": (None, [c_void_p]),
    "gl_model_num_params": (c_int, [c_void_p]),
    "gl_model_param_offset": (c_int, [c_void_p, c_int]),
    "gl_model_num_pixels": (c_int64, [c_void_p]),
    "gl_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "gl_simulate_fwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gl_simulate_parts_fwd": (c_int, [c_void_p, c_void_p, c_int, c_uint32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gl_simulate_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gl_loglike_fwd_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gl_model_set_prior": (c_int, [c_void_p, POINTER(gl_zcolumn), c_int, POINTER(c_float)]),
    "gl_logprob_fwd_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_uint32, c_void_p, c_size_t,
                                   c_void_p]),
    "gl_model_set_positions": (c_int, [c_void_p, c_int, POINTER(c_int32), POINTER(c_float), POINTER(c_float),
                                       POINTER(c_float), POINTER(c_float)]),
    "gl_model_set_source_scales": (c_int, [c_void_p, POINTER(c_float), c_int]),
    "gl_model_set_position_scales": (c_int, [c_void_p, POINTER(c_float), c_int]),
    "gl_model_set_position_fluxes": (c_int, [c_void_p, POINTER(c_float), POINTER(c_float), c_int]),
    "gl_position_fluxes_fwd_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_size_t, c_void_p]),
    "gl_model_set_position_delays": (c_int, [c_void_p, POINTER(c_float), POINTER(c_float), c_int, POINTER(c_float), c_int]),
    "gl_position_delays_fwd_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_size_t, c_void_p]),
    "gl_model_set_position_plane_delays": (c_int, [c_void_p, POINTER(c_float), POINTER(c_float), c_int, POINTER(c_double),
                                                   POINTER(c_double), POINTER(c_float), c_int, c_int]),
    "gl_multiplane_position_delays_fwd_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                      c_void_p, c_void_p, c_size_t, c_void_p]),
    "gl_position_family_terms": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_void_p]),
    "gl_image_positions_scaled": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, POINTER(c_float), c_float, c_float,
                                          c_float, c_float, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_size_t, c_void_p]),
    "gl_critical_curves_scaled": (c_int, [c_void_p, c_void_p, c_int, c_float, c_float, c_float, c_float, c_int, c_int, c_float,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_size_t, c_void_p]),
    "gl_positions_fwd_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                     c_void_p]),
    "gl_series_precompute": (c_int, [c_int, c_int, POINTER(c_int32), c_void_p, POINTER(c_float), c_int, c_int, c_void_p,
                                     c_void_p, c_int64, c_void_p, c_void_p]),
    "gl_model_set_series": (c_int, [c_void_p, c_int, c_float, c_void_p]),
    "gl_series_eval": (c_int, [c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                               c_void_p]),
    "gl_adam_update": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float,
                               c_float, c_int64, c_void_p, c_void_p]),
    "gl_svi_sample": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_float, c_void_p, c_void_p]),
    "gl_svi_grad": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p]),
    "gl_hmc_kick_drift": (c_int, [c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_float, c_int, c_int, c_void_p, c_void_p,
                                  c_void_p]),
    "gl_hmc_accept": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                              c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gl_profile_basis": (c_int, [POINTER(gl_component), c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p,
                                 c_void_p]),
    "gl_series_precompute_hessian": (c_int, [c_int, c_int, POINTER(c_int32), c_void_p, POINTER(c_float), c_int, c_int,
                                             c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "gl_series_hessian_eval": (c_int, [c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    "gl_model_set_series_hessian": (c_int, [c_void_p, c_int, c_void_p]),
    "gl_lens_maps": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "gl_lens_maps_vjp_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int64]),
    "gl_lens_maps_vjp": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                 c_void_p]),
    "gl_lens_hessian_vjp_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int64]),
    "gl_lens_hessian_vjp": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                    c_void_p]),
    "gl_shear_loglike_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int]),
    "gl_shear_loglike": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gl_imgplane_loglike_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int]),
    "gl_imgplane_loglike": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, POINTER(c_int32), c_int, c_int, c_void_p, c_float,
                                    c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gl_model_set_lens_planes": (c_int, [c_void_p, POINTER(c_int32), c_int, c_int, POINTER(c_float), POINTER(c_float), c_int]),
    "gl_multiplane_maps": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_int, POINTER(c_float), c_int, c_void_p,
                                   c_void_p]),
    "gl_multiplane_simulate": (c_int, [c_void_p, c_void_p, c_int, c_uint32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gl_multiplane_loglike": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int, c_void_p, c_void_p,
                                      c_void_p, c_size_t, c_void_p]),
    "gl_multiplane_simulate_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gl_multiplane_loglike_fwd_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gl_multiplane_logprob_fwd_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_float, c_uint32, c_void_p, c_size_t, c_void_p]),
    "gl_model_set_position_targets": (c_int, [c_void_p, POINTER(c_float), c_int, c_int]),
    "gl_multiplane_positions_fwd_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                                c_void_p]),
    "gl_multiplane_image_positions_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int]),
    "gl_multiplane_image_positions": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, POINTER(c_float), c_int, c_float,
                                              c_float, c_float, c_float, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_size_t, c_void_p]),
    "gl_multiplane_fermat_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "gl_multiplane_fermat": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(c_double),
                                     POINTER(c_double), c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gl_lens_potential": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "gl_image_positions_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int]),
    "gl_image_positions_stage_counts": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "gl_multiplane_image_positions_stage_counts": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p,
                                                           c_void_p]),
    "gl_critical_curves_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int]),
    "gl_critical_curves": (c_int, [c_void_p, c_void_p, c_int, c_float, c_float, c_float, c_float, c_int, c_int, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gl_multiplane_critical_curves_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int]),
    "gl_multiplane_critical_curves": (c_int, [c_void_p, c_void_p, c_int, POINTER(c_float), c_int, c_int, c_float, c_float, c_float,
                                              c_float, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gl_pixsrc_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int, c_int]),
    "gl_pixsrc_layout": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, POINTER(c_int32)]),
    "gl_pixsrc_reconstruct": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                      c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                      c_void_p]),
    "gl_pixsrc_grad_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int]),
    "gl_pixsrc_grad_layout": (c_int, [c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int32)]),
    "gl_pixsrc_evidence_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                        c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_size_t, c_void_p]),
    "gl_ptimg_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "gl_ptimg_render": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(ctypes.c_double), c_void_p, c_void_p, c_size_t,
                                c_void_p]),
    "gl_ptimg_render_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(ctypes.c_double), c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gl_ptimg_fit": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(ctypes.c_double), c_void_p, c_void_p, c_int, c_void_p, c_int,
                             c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                             c_void_p]),
    "gl_image_positions": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_float, c_float, c_float, c_float,
                                   c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gl_model_num_linear": (c_int, [c_void_p]),
    "gl_model_linear_column": (c_int, [c_void_p, c_int]),
    "gl_lstsq_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "gl_lstsq_solve_flags": (c_int, [c_void_p, c_int, ctypes.POINTER(c_size_t)]),
    "gl_lstsq_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_uint32, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_size_t, c_void_p]),
    "gl_lstsq_solve_stack_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "gl_lstsq_solve_stack": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_size_t, c_void_p]),
    "gl_lstsq_last_kernels": (c_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, c_size_t]),
    "gl_model_set_catalogue": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_int32), POINTER(c_float)]),
    "gl_model_set_light_image": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_float)]),
    "gl_model_set_lens_maps": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_float), POINTER(c_float), c_double]),
    "gl_interpol_mass_eval": (c_int, [POINTER(gl_component), c_int, c_int, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_int64,
                                      c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "gl_interpol_eval": (c_int, [POINTER(gl_component), c_int, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p,
                                 c_void_p, c_int, c_void_p]),
    "gl_scaled_eval": (c_int, [c_int, c_int, POINTER(c_int32), c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int,
                               c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "gl_scaled_hessian": (c_int, [c_int, c_int, POINTER(c_int32), c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int,
                                  c_void_p, c_int, c_void_p, c_void_p]),
    "gl_profile_eval": (c_int, [POINTER(gl_component), c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p,
                                c_void_p, c_void_p, c_void_p]),
    "gl_user_model_compile_count": (ctypes.c_longlong, []),
    "gl_user_profile_check": (c_int, [ctypes.c_char_p, c_int, c_int]),
    "gl_user_points_check": (c_int, [ctypes.c_char_p, c_int]),
    "gl_user_profile_create": (c_int, [ctypes.c_char_p, c_int, c_int, POINTER(c_void_p)]),
    "gl_user_profile_eval": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
    "gl_user_profile_destroy": (None, [c_void_p]),
    "gl_profile_hessian": (c_int, [POINTER(gl_component), c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p,
                                   c_void_p, c_void_p]),
    "gl_profile_potential": (c_int, [POINTER(gl_component), c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p,
                                     c_void_p, c_void_p]),
    "gl_kind_num_params": (c_int, [POINTER(gl_component)]),
    "gl_model_set_timing": (c_int, [c_void_p, c_int]),
    "gl_model_last_main_ms": (c_int, [c_void_p, POINTER(c_float)]),
    "gl_model_set_timing_stride": (c_int, [c_void_p, c_int]),
    "gl_model_timing_drain": (c_int, [c_void_p, POINTER(c_float), c_int, POINTER(c_int)]),
    "gl_model_last_main_kernel": (c_int, [c_void_p, ctypes.c_char_p, c_size_t]),
    "gl_post_apply": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_float, c_void_p]),
    "gl_model_last_post_kernel": (c_int, [c_void_p, c_int, ctypes.c_char_p, c_size_t]),
    "gl_model_launch_shape": (c_int, [c_void_p, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_size_t)]),
    "gl_model_workspace_layout": (c_int, [c_void_p, c_int, c_int, POINTER(gl_workspace_layout)]),
    "gl_last_error": (c_char_p, []),
    "gl_version": (c_char_p, []),
}


def lib_path():
    return _LIB_PATH


def lib():
    """Load the HIP library or fail loudly (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise NativeLibraryError(
                f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). gigalens_amd has no CPU fallback.")
        try:
            h = ctypes.CDLL(_LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise NativeLibraryError(f"cannot load {_LIB_PATH}: {e}") from e
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def _check(rc):
    if rc != 0:
        raise NativeLibraryError(f"gigalens_hip error {rc}: {lib().gl_last_error().decode()}")


GL_EUNSUPPORTED = -2


def _check_potential(rc):
    """_check for the lensing-potential and critical-curve calls: GL_EUNSUPPORTED becomes UnsupportedLensError."""
    if rc == GL_EUNSUPPORTED:
        raise UnsupportedLensError(f"gigalens_hip error {rc}: {lib().gl_last_error().decode()}")
    _check(rc)


def deflection_scales(values, n, what):
    """``n`` deflection scales (``gigalens_amd.cosmology.deflection_scale``) as a float32 array; None = all 1.  ``ValueError`` on a
    length mismatch or a value that is not finite or not > 0."""
    if values is None:
        return np.ones(n, dtype=np.float32)
    arr = np.atleast_1d(np.asarray(values, dtype=np.float32))
    if arr.ndim != 1 or arr.size != n:
        raise ValueError(f"{what}: expected {n} scale(s), got {arr.size if arr.ndim == 1 else tuple(arr.shape)}")
    if not (np.all(np.isfinite(arr)) and np.all(arr > 0)):
        raise ValueError(f"{what}: every scale must be finite and > 0, got {arr.tolist()}")
    return arr


def _require_cuda(t, what):
    if not t.is_cuda:
        raise NativeLibraryError(f"{what} must live on the GPU (got device {t.device}); gigalens_amd has no CPU path")


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def lstsq_solve_stack_workspace_bytes(B, D, HW, workgroups=2048):
    return lib().gl_lstsq_solve_stack_workspace_bytes(int(B), int(D), int(HW), int(workgroups))


def lstsq_solve_stack(stack, obs, err, workgroups=2048, cholesky=True, coeffs=None, flags=None, normal=None, workspace=None):
    """gl_lstsq_solve_stack: the solve of ``lstsq_simulate`` on a caller's basis stack ``[B, D, HW]`` with ``obs`` / ``err``
    ``[HW]`` (float32, on the GPU; ``obs`` / ``err`` may be views at any float offset).  ``coeffs [B, D]``, ``flags [B]`` int32,
    ``normal [B, Dp, Dp]`` and ``workspace`` (uint8) are written into when given; returns ``coeffs``."""
    for t, what in ((stack, "stack"), (obs, "obs"), (err, "err")):
        _require_cuda(t, what)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise NativeLibraryError(f"lstsq_solve_stack: {what} must be contiguous float32, got {t.dtype} {tuple(t.shape)}")
    if stack.dim() != 3 or obs.numel() != stack.shape[2] or err.numel() != stack.shape[2]:
        raise NativeLibraryError(f"lstsq_solve_stack: stack [B,D,HW] with obs, err [HW], got {tuple(stack.shape)}, {tuple(obs.shape)}, {tuple(err.shape)}")
    B, D, HW = stack.shape
    if workspace is None:
        workspace = torch.empty(max(lstsq_solve_stack_workspace_bytes(B, D, HW, workgroups), 1), dtype=torch.uint8, device=stack.device)
    if coeffs is None:
        coeffs = torch.empty((B, D), dtype=torch.float32, device=stack.device)
    with torch.cuda.device(stack.device):
        _check(lib().gl_lstsq_solve_stack(_ptr(stack), _ptr(obs), _ptr(err), B, D, HW, int(workgroups), int(bool(cholesky)),
                                          _ptr(coeffs), _ptr(flags), _ptr(normal), _ptr(workspace), workspace.numel(), _stream()))
    return coeffs


def lstsq_last_kernels():
    """Mangled symbols (normal-matrix, Cholesky, eigenvalue kernel) of the most recent linear solve; '' = the stage did not run."""
    bufs = [ctypes.create_string_buffer(1024) for _ in range(3)]
    _check(lib().gl_lstsq_last_kernels(*bufs, 1024))
    return tuple(b.value.decode() for b in bufs)


def component_of(profile, bodies=None):
    """gl_component of a profile.  ``bodies``: the list a model under construction collects user-written bodies in (`hip_body`
    profiles become GL_USER_MASS / GL_USER_LIGHT components pointing into it); None outside a model."""
    kind, iparam, flags = profile._component()
    if not kind and bodies is not None and getattr(profile, "hip_body", ""):
        from gigalens_amd.profile import LightProfile
        n = len(profile._native_params())
        if n > 16:
            raise NativeLibraryError(f"profile {profile.name!r}: a user-written profile inside a model takes at most 16 parameters, got {n}")
        if profile.hip_body not in bodies:
            bodies.append(profile.hip_body)
        # reserved = 1: the LAST parameter of a user-written light is its linear amplitude (LightProfile._amp, profile.py:24-60) --
        # the column the linear-amplitude solve sets to 1 for the basis image and writes the solved coefficient into
        is_light = isinstance(profile, LightProfile)
        return gl_component(20 if is_light else 13, n, bodies.index(profile.hip_body), 1 if (is_light and getattr(profile, "_amp", "")) else 0)
    if not kind:
        raise NativeLibraryError(
            f"profile {getattr(profile, 'name', type(profile).__name__)!r} has no gl_kind: user-defined deriv / light bodies "
            "written in Python cannot run here.  Give the class a `hip_body` -- one HIP C++ function template over a number type "
            "that the library compiles at run time (include/gigalens_hip.h gl_user_profile_create / gl_model_create_user; see "
            "INTEGRATION.md) -- and it serves deriv / light on points as well as LensSimulator's pixel kernels")
    return gl_component(kind, iparam, flags, 0)


# --------------------------------------------------------------------------------------------------
# user-written profile bodies (profile.py: `hip_body`), compiled once per (body, kind, parameter count) by hiprtc
# --------------------------------------------------------------------------------------------------
class _UserProfile:
    def __init__(self, body, is_light, n_params):
        h = c_void_p()
        _check(lib().gl_user_profile_create(body.encode(), int(is_light), int(n_params), ctypes.byref(h)))
        self._h, self.is_light, self.n_params = h, bool(is_light), int(n_params)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().gl_user_profile_destroy(self._h)
        except Exception:
            pass


_USER_PROFILES = {}


def user_profile_of(profile):
    from gigalens_amd.profile import LightProfile
    body = getattr(profile, "hip_body", None)
    if not body:
        return None
    device()
    is_light = isinstance(profile, LightProfile)
    key = (body, is_light, len(profile.params))
    if key not in _USER_PROFILES:
        _USER_PROFILES[key] = _UserProfile(body, is_light, len(profile.params))
    return _USER_PROFILES[key]


def user_points_check(body, n_params):
    """Compile a mass body into the point kernels (image-position likelihood, lens maps: nested duals) without a GPU."""
    _check(lib().gl_user_points_check(body.encode(), int(n_params)))


def user_profile_check(body, is_light, n_params):
    """Compile a body without a GPU (gl_user_profile_check); raises NativeLibraryError with the compiler's message."""
    _check(lib().gl_user_profile_check(body.encode(), int(bool(is_light)), int(n_params)))


class _UserEval(torch.autograd.Function):
    """Values of a compiled user body on points [n_pts, B] with parameters [B, n]; when a gradient is wanted the same launch
    returns the Jacobian with respect to (x, y, parameters) from forward-mode duals, and backward contracts it."""

    @staticmethod
    def forward(ctx, up, xb, yb, P):
        n_pts, B = xb.shape
        n_out = 1 if up.is_light else 2
        out0 = torch.empty_like(xb)
        out1 = None if up.is_light else torch.empty_like(xb)
        need = any(ctx.needs_input_grad[1:])
        jac = torch.empty((n_out, up.n_params + 2, n_pts, B), dtype=torch.float32, device=xb.device) if need else None
        _check(lib().gl_user_profile_eval(up._h, _ptr(xb), _ptr(yb), n_pts, B, 1, _ptr(P), _ptr(out0), _ptr(out1), _ptr(jac),
                                          _stream()))
        ctx.jac = jac
        return (out0,) if up.is_light else (out0, out1)

    @staticmethod
    def backward(ctx, *gs):
        J = ctx.jac
        g = torch.stack([torch.zeros_like(J[0, 0]) if gi is None else gi for gi in gs], dim=0)  # [n_out, n_pts, B]
        full = (g[:, None] * J).sum(dim=0)                                                           # [n + 2, n_pts, B]
        gP = full[2:].sum(dim=1).transpose(0, 1).contiguous() if J.shape[1] > 2 else None            # [B, n]
        return None, full[0], full[1], gP


def _user_eval(up, profile, x, y, kwargs):
    xb, yb, P, B, out_shape = _broadcast_points(profile, x, y, kwargs, list(profile.params), device())
    return tuple(o.reshape(out_shape) for o in _UserEval.apply(up, xb, yb, P))


def device():
    if not torch.cuda.is_available():
        raise NativeLibraryError("no GPU visible: gigalens_amd's hot path only runs as HIP kernels on gfx950")
    return torch.device("cuda", torch.cuda.current_device())


# --------------------------------------------------------------------------------------------------
# plugin-level point evaluation (MassProfile.deriv / LightProfile.light)
# --------------------------------------------------------------------------------------------------
def _broadcast_points(profile, x, y, kwargs, names, dev, columns=None):
    """Points and parameters of a plugin-level call on their common shape ``(..., B)``: ``xb, yb`` [n_pts, B], the parameter rows
    ``P`` [B, len(columns)] (``columns``: the native parameter order, default ``names``; a column not among ``names`` is 1 -- the
    unit amplitudes of profile_basis), ``B`` and the broadcast shape."""
    missing = [n for n in names if n not in kwargs]
    if missing:
        raise TypeError(f"{profile.name}: missing parameters {missing}")
    x = torch.as_tensor(x, dtype=torch.float32, device=dev)
    y = torch.as_tensor(y, dtype=torch.float32, device=dev)
    vals = [torch.as_tensor(kwargs[n], dtype=torch.float32, device=dev) for n in names]
    out_shape = torch.broadcast_shapes(x.shape, y.shape, *[v.shape for v in vals])
    B = out_shape[-1] if len(out_shape) else 1
    for n, v in zip(names, vals):
        if v.dim() > 1 and any(s != 1 for s in v.shape[:-1]):
            raise NativeLibraryError(f"{profile.name}.{n}: parameters may only vary along the last (batch) axis")
    cols = {n: (v.reshape(-1)[-B:].expand(B) if v.numel() > 1 else v.reshape(()).expand(B)) for n, v in zip(names, vals)}
    one = torch.ones(B, dtype=torch.float32, device=dev)
    rows = [cols.get(n, one) for n in (names if columns is None else columns)]
    P = torch.stack(rows, dim=1).contiguous() if rows else torch.zeros((B, 0), dtype=torch.float32, device=dev)
    xb = x.expand(out_shape).reshape(-1, B).contiguous()
    yb = y.expand(out_shape).reshape(-1, B).contiguous()
    return xb, yb, P, B, out_shape


def scaled_eval(profile, x, y, scales):
    """ScalingRelation.deriv (scaling_relation.py:61-70) through gl_scaled_eval."""
    dev = device()
    xb, yb, P, B, out_shape = _broadcast_points(profile, x, y, scales, list(profile.params), dev)
    base_kind, cols, table = profile._catalogue()
    if profile._dev_table is None or profile._dev_table.device != dev:
        profile._dev_table = torch.from_numpy(table).to(dev)
    col_arr = (c_int32 * 3)(*cols)
    out0, out1 = torch.empty_like(xb), torch.empty_like(xb)
    _check(lib().gl_scaled_eval(base_kind, table.shape[0], col_arr, _ptr(profile._dev_table), _ptr(xb), _ptr(yb),
                                xb.shape[0], B, 1, _ptr(P), P.shape[1], _ptr(out0), _ptr(out1), _stream()))
    return out0.reshape(out_shape), out1.reshape(out_shape)


def series_precompute(series, hessian=False):
    """MassSeries.set_deriv / set_hessian (series_profile.py:61-65) through gl_series_precompute[_hessian]: device
    ``[2, order+1, n_points]`` (alpha_x, alpha_y) or ``[3, order+1, n_points]`` (f_xx, f_xy, f_yy)."""
    dev = device()
    base_kind, cols, table, scales = series._series_inputs()
    x = torch.as_tensor(series.x, dtype=torch.float32, device=dev).reshape(-1).contiguous()
    y = torch.as_tensor(series.y, dtype=torch.float32, device=dev).reshape(-1).contiguous()
    tab = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32)).to(dev)
    sc = (c_float * len(scales))(*[float(v) for v in scales])
    out = torch.empty((3 if hessian else 2, series.order + 1, x.numel()), dtype=torch.float32, device=dev)
    fn = lib().gl_series_precompute_hessian if hessian else lib().gl_series_precompute
    _check(fn(int(base_kind), tab.shape[0], (c_int32 * 3)(*cols), _ptr(tab), sc, len(scales), series.order, _ptr(x),
              _ptr(y), x.numel(), _ptr(out), _stream()))
    return out


def series_hessian_eval(series, amplitude, var):
    """MassSeries.hessian (series_profile.py:83-89): ``(f_xx, f_xy, f_xy, f_yy)``, field shape + trailing batch axis."""
    dev = device()
    a = torch.as_tensor(amplitude, dtype=torch.float32, device=dev).reshape(-1)
    v = torch.as_tensor(var, dtype=torch.float32, device=dev).reshape(-1)
    B = max(a.numel(), v.numel())
    a, v = a.expand(B).contiguous(), v.expand(B).contiguous()
    n = series._hcoefs.shape[-1]
    out = torch.empty((3, n, B), dtype=torch.float32, device=dev)
    _check(lib().gl_series_hessian_eval(_ptr(series._hcoefs), series.order, n, B, _ptr(a), _ptr(v),
                                        float(series.series_var_0), _ptr(out), _stream()))
    shape = tuple(torch.as_tensor(series.x).shape)
    if shape and shape[-1] == B and len(shape) > 1:
        shape = shape[:-1]
        out = out.reshape(3, -1, B, B).diagonal(dim1=2, dim2=3)
    out = out.reshape((3,) + shape + (B,))
    return out[0], out[1], out[1], out[2]


def series_eval(series, amplitude, var):
    """MassSeries.deriv (series_profile.py:76-81): field shape + trailing batch axis."""
    dev = device()
    a = torch.as_tensor(amplitude, dtype=torch.float32, device=dev).reshape(-1)
    v = torch.as_tensor(var, dtype=torch.float32, device=dev).reshape(-1)
    B = max(a.numel(), v.numel())
    a, v = a.expand(B).contiguous(), v.expand(B).contiguous()
    n = series._coefs.shape[-1]
    o0 = torch.empty((n, B), dtype=torch.float32, device=dev)
    o1 = torch.empty_like(o0)
    _check(lib().gl_series_eval(_ptr(series._coefs), series.order, n, B, _ptr(a), _ptr(v), float(series.series_var_0),
                                _ptr(o0), _ptr(o1), _stream()))
    shape = tuple(torch.as_tensor(series.x).shape)
    if shape and shape[-1] == B and len(shape) > 1:  # grid given per batch element, as the reference's (N, bs) grids
        shape = shape[:-1]
        o0, o1 = o0.reshape(-1, B, B).diagonal(dim1=1, dim2=2), o1.reshape(-1, B, B).diagonal(dim1=1, dim2=2)
    return o0.reshape(shape + (B,)), o1.reshape(shape + (B,))


def scaled_hessian(profile, x, y, scales):
    """ScalingRelation.hessian (scaling_relation.py:72-83) through gl_scaled_hessian."""
    dev = device()
    xb, yb, P, B, out_shape = _broadcast_points(profile, x, y, scales, list(profile.params), dev)
    base_kind, cols, table = profile._catalogue()
    if profile._dev_table is None or profile._dev_table.device != dev:
        profile._dev_table = torch.from_numpy(table).to(dev)
    out = torch.empty((4,) + tuple(xb.shape), dtype=torch.float32, device=dev)
    _check(lib().gl_scaled_hessian(base_kind, table.shape[0], (c_int32 * 3)(*cols), _ptr(profile._dev_table), _ptr(xb),
                                   _ptr(yb), xb.shape[0], B, 1, _ptr(P), P.shape[1], _ptr(out), _stream()))
    return tuple(out[k].reshape(out_shape) for k in range(4))


def profile_hessian(profile, x, y, kwargs):
    """MassProfile.hessian (tf/profile.py:9-27): ``(f_xx, f_xy, f_yx, f_yy)``."""
    dev = device()
    up = user_profile_of(profile) if not profile._component()[0] else None
    if up is not None:  # a user-written body: the derivative of its deflection from the same duals (d fx / d(x, y), d fy / d(x, y))
        xb, yb, P, B, out_shape = _broadcast_points(profile, x, y, kwargs, list(profile.params), dev)
        n_pts = xb.shape[0]
        out0, out1 = torch.empty_like(xb), torch.empty_like(xb)
        jac = torch.empty((2, up.n_params + 2, n_pts, B), dtype=torch.float32, device=dev)
        _check(lib().gl_user_profile_eval(up._h, _ptr(xb), _ptr(yb), n_pts, B, 1, _ptr(P), _ptr(out0), _ptr(out1), _ptr(jac), _stream()))
        return tuple(jac[i, j].reshape(out_shape) for i, j in ((0, 0), (0, 1), (1, 0), (1, 1)))
    comp = component_of(profile)
    xb, yb, P, B, out_shape = _broadcast_points(profile, x, y, kwargs, list(profile.params), dev)
    out = torch.empty((4,) + tuple(xb.shape), dtype=torch.float32, device=dev)
    _check(lib().gl_profile_hessian(ctypes.byref(comp), _ptr(xb), _ptr(yb), xb.shape[0], B, 1, _ptr(P), _ptr(out),
                                    _stream()))
    return tuple(out[k].reshape(out_shape) for k in range(4))


def profile_potential(profile, x, y, kwargs):
    """MassProfile.potential (beyond the reference): psi on points, free-standing built-in mass kinds only (gl_profile_potential)."""
    if any(torch.is_tensor(v) and v.requires_grad for v in (x, y, *kwargs.values())):
        raise NotImplementedError("potential is forward-only (no gradient)")
    if not profile._component()[0]:
        raise UnsupportedLensError(f"profile {profile.name!r}: a user-written body defines a deflection only, no potential")
    dev = device()
    comp = component_of(profile)
    xb, yb, P, B, out_shape = _broadcast_points(profile, x, y, kwargs, list(profile.params), dev)
    out = torch.empty_like(xb)
    _check_potential(lib().gl_profile_potential(ctypes.byref(comp), _ptr(xb), _ptr(yb), xb.shape[0], B, 1, _ptr(P), _ptr(out),
                                                _stream()))
    return out.reshape(out_shape)


def profile_eval(profile, x, y, kwargs):
    up = user_profile_of(profile) if not profile._component()[0] else None
    if up is not None:
        return _user_eval(up, profile, x, y, kwargs)
    dev = device()
    comp = component_of(profile)
    xb, yb, P, B, out_shape = _broadcast_points(profile, x, y, kwargs, list(profile.params), dev)
    n_pts = xb.shape[0]
    out0 = torch.empty_like(xb)
    is_mass = comp.kind <= 12 or comp.kind == GL_MULTIPOLE
    out1 = torch.empty_like(xb) if is_mass else None
    _check(lib().gl_profile_eval(ctypes.byref(comp), _ptr(xb), _ptr(yb), n_pts, B, 1, _ptr(P), _ptr(out0),
                                 _ptr(out1), _stream()))
    if is_mass:
        return out0.reshape(out_shape), out1.reshape(out_shape)
    return (out0.reshape(out_shape),)


def adam_update(x, grad, m, v, grad_scale, lr, b1, b2, eps, t, t_dev=None):
    """gl_adam_update: one fused optimiser step in place on ``x``, ``m``, ``v`` (contiguous float32 CUDA tensors)."""
    for name, a in (("x", x), ("grad", grad), ("m", m), ("v", v)):
        _require_cuda(a, name)
        if a.dtype != torch.float32 or not a.is_contiguous():
            raise NativeLibraryError(f"adam_update: {name} must be a contiguous float32 tensor")
    if not (x.numel() == grad.numel() == m.numel() == v.numel()):
        raise NativeLibraryError("adam_update: size mismatch")
    _check(lib().gl_adam_update(_ptr(x), _ptr(grad), _ptr(m), _ptr(v), x.numel(), float(grad_scale), float(lr),
                                float(b1), float(b2), float(eps), int(t), _ptr(t_dev), _stream()))


def svi_sample(mu, l_packed, eps, full_rank, diag_shift=1e-6):
    """gl_svi_sample: ``z = mu + L eps`` for the packed surrogate (float32 CUDA tensors)."""
    n, d = eps.shape
    z = torch.empty_like(eps)
    _check(lib().gl_svi_sample(_ptr(mu), _ptr(l_packed), d, int(bool(full_rank)), _ptr(eps), n, float(diag_shift), _ptr(z),
                               _stream()))
    return z


def svi_grad(l_packed, eps, logp, grad_z, full_rank, diag_shift=1e-6):
    """gl_svi_grad: the fused ``[ELBO, dELBO/dmu, dELBO/dl_packed]`` buffer."""
    n, d = eps.shape
    buf = torch.empty(1 + d + l_packed.numel(), dtype=torch.float32, device=eps.device)
    _check(lib().gl_svi_grad(_ptr(l_packed), d, int(bool(full_rank)), _ptr(eps), _ptr(logp), _ptr(grad_z), n,
                             float(diag_shift), _ptr(buf), _stream()))
    return buf


def hmc_kick_drift(p_in, grad, kick, z_in, sigma, eps, p_out, z_out):
    """gl_hmc_kick_drift on contiguous float32 CUDA tensors ``[n, d]`` (``sigma`` ``[d, d]``)."""
    n, d = p_in.shape
    _check(lib().gl_hmc_kick_drift(_ptr(p_in), _ptr(grad), float(kick), _ptr(z_in), _ptr(sigma), float(eps), n, d,
                                   _ptr(p_out), _ptr(z_out), _stream()))


def hmc_accept(z, g, lp, zn, gn, lpn, p0, pn, kick, scale_tril, uniforms, accept_prob):
    """gl_hmc_accept: Metropolis step of one transition, state updated in place."""
    n, d = z.shape
    _check(lib().gl_hmc_accept(_ptr(z), _ptr(g), _ptr(lp), _ptr(zn), _ptr(gn), _ptr(lpn), _ptr(p0), _ptr(pn), float(kick),
                               _ptr(scale_tril), _ptr(uniforms), n, d, _ptr(accept_prob), _stream()))


def profile_basis(profile, x, y, kwargs):
    """``light`` of a ``use_lstsq`` profile (gl_profile_basis): ``(depth,) + broadcast shape`` unit-amplitude images."""
    dev = device()
    comp = component_of(profile)
    # profile.params: without the amplitudes (profile.py:40-41), which the native row holds as unit columns
    xb, yb, P, B, out_shape = _broadcast_points(profile, x, y, kwargs, list(profile.params), dev, columns=profile._native_params())
    out = torch.empty((int(profile.depth),) + tuple(xb.shape), dtype=torch.float32, device=dev)
    _check(lib().gl_profile_basis(ctypes.byref(comp), _ptr(xb), _ptr(yb), xb.shape[0], B, 1, _ptr(P), _ptr(out),
                                  _stream()))
    return out.reshape((int(profile.depth),) + tuple(out_shape))


def interpol_eval(profile, x, y, kwargs):
    """``Interpolated.light`` on points (gl_interpol_eval): the surface brightness, or with ``use_lstsq`` the unit-amplitude basis
    image with a leading axis of 1.  Forward only."""
    dev = device()
    comp = component_of(profile)
    basis = bool(profile.use_lstsq)
    xb, yb, P, B, out_shape = _broadcast_points(profile, x, y, kwargs, list(profile.params), dev, columns=profile._native_params())
    if profile._dev_table is None or profile._dev_table.device != dev:  # the image with its two-pixel zero apron
        profile._dev_table = torch.nn.functional.pad(torch.from_numpy(profile.image), (2, 2, 2, 2)).to(dev).contiguous()
    h, w = profile.image.shape
    out = torch.empty_like(xb)
    _check(lib().gl_interpol_eval(ctypes.byref(comp), h, w, _ptr(profile._dev_table), _ptr(xb), _ptr(yb), xb.shape[0], B, 1, _ptr(P),
                                  _ptr(out), int(basis), _stream()))
    return out.reshape((1,) + tuple(out_shape)) if basis else out.reshape(out_shape)


def interpol_mass_eval(profile, x, y, kwargs, hessian):
    """``Interpolated.deriv`` / ``.hessian`` of the mass profile on points (gl_interpol_mass_eval).  Forward only."""
    dev = device()
    comp = component_of(profile)
    xb, yb, P, B, out_shape = _broadcast_points(profile, x, y, kwargs, list(profile.params), dev)
    if profile._dev_table is None or profile._dev_table.device != dev:  # both maps, each with its two-pixel zero apron
        maps = torch.from_numpy(np.stack([profile.alpha_x, profile.alpha_y]))
        profile._dev_table = torch.nn.functional.pad(maps, (2, 2, 2, 2)).to(dev).contiguous()
    h, w = profile.alpha_x.shape
    out = torch.empty((4 if hessian else 2,) + tuple(xb.shape), dtype=torch.float32, device=dev)
    _check(lib().gl_interpol_mass_eval(ctypes.byref(comp), h, w, _ptr(profile._dev_table[0]), _ptr(profile._dev_table[1]),
                                       float(profile.pitch), _ptr(xb), _ptr(yb), xb.shape[0], B, 1, _ptr(P), _ptr(out[0]),
                                       None if hessian else _ptr(out[1]), int(bool(hessian)), _stream()))
    return tuple(out[k].reshape(out_shape) for k in range(out.shape[0]))


# --------------------------------------------------------------------------------------------------
# model handle
# --------------------------------------------------------------------------------------------------
class Model:
    """Owns one ``gl_model`` (immutable descriptor + grid on the current device)."""

    def __init__(self, components, n_lens, n_lens_light, n_src, height, width, supersample, grid_x, grid_y,
                 pix_index, conversion_factor, psf=None, bodies=None):
        self.device = device()
        L = lib()
        n = len(components)
        arr = (gl_component * max(n, 1))(*components)
        gx = np.ascontiguousarray(grid_x, dtype=np.float32)
        gy = np.ascontiguousarray(grid_y, dtype=np.float32)
        g = gl_grid()
        g.height, g.width, g.supersample, g.n_region = int(height), int(width), int(supersample), int(gx.size)
        g.grid_x = gx.ctypes.data_as(POINTER(c_float))
        g.grid_y = gy.ctypes.data_as(POINTER(c_float))
        if pix_index is not None:
            pi = np.ascontiguousarray(pix_index, dtype=np.int32)
            g.pix_index = pi.ctypes.data_as(POINTER(c_int32))
        g.conversion_factor = float(conversion_factor)
        if psf is not None:
            pk = np.ascontiguousarray(psf, dtype=np.float32)
            g.psf = pk.ctypes.data_as(POINTER(c_float))
            g.psf_h, g.psf_w = pk.shape
        h = c_void_p()
        with torch.cuda.device(self.device):
            if bodies:  # user-written profiles: the interpreter kernel is compiled with them now (seconds, once)
                barr = (ctypes.c_char_p * len(bodies))(*[b.encode() for b in bodies])
                # (GL_EUNSUPPORTED -- user-written profiles beside an Interpolated light or lens -- raises UnsupportedLensError)
                _check_potential(L.gl_model_create_user(arr, n_lens, n_lens_light, n_src, ctypes.byref(g), barr, len(bodies), ctypes.byref(h)))
            else:
                _check(L.gl_model_create(arr, n_lens, n_lens_light, n_src, ctypes.byref(g), ctypes.byref(h)))
        self._h = h
        self.P = L.gl_model_num_params(h)
        self.N = L.gl_model_num_pixels(h)
        self.offsets = [L.gl_model_param_offset(h, i) for i in range(n)]
        self.out_h, self.out_w = height // supersample, width // supersample
        self.ss_h, self.ss_w = int(height), int(width)
        self.n_planes = 1  # lens planes (set_lens_planes)
        # what others bind to this model, and how they tell that it still holds
        self.prior_owner = None  # the probabilistic model whose prior set_prior last took (the binder sets it)
        self.positions_owner = None  # ... whose image positions set_positions last took
        self.generation = 0  # bumped by every set_*: a HIP graph captured at another generation holds stale device pointers
        self._ws = {}  # {B: workspace} of the latest batch size
        self._scratch_bufs = {}  # {name: workspace} of the calls that size their own (_scratch)
        self._timing_slots = 0

    def _changed(self, layout):
        """Every set_* ends here once the library has taken the new state.  ``layout``: the workspace layout follows it."""
        self.generation += 1
        if layout:
            self._ws = {}

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.gl_model_destroy(h)

    def set_catalogue(self, component, base_kind, cols, table):
        """Attach the galaxy catalogue of a GL_SCALED lens (gl_model_set_catalogue)."""
        t = np.ascontiguousarray(table, dtype=np.float32)
        col_arr = (c_int32 * 3)(*[int(c) for c in cols])
        with torch.cuda.device(self.device):
            _check(lib().gl_model_set_catalogue(self._h, int(component), int(base_kind), int(t.shape[0]), col_arr,
                                                t.ctypes.data_as(POINTER(c_float))))
        self._changed(True)  # the workspace grows with the catalogue

    def set_light_image(self, component, image):
        """Attach the image of a GL_INTERPOL light (gl_model_set_light_image): ``image`` a 2-D float32 host array."""
        img = np.ascontiguousarray(image, dtype=np.float32)
        with torch.cuda.device(self.device):
            _check(lib().gl_model_set_light_image(self._h, int(component), int(img.shape[0]), int(img.shape[1]),
                                                  img.ctypes.data_as(POINTER(c_float))))
        self._changed(False)

    def set_lens_maps(self, component, alpha_x, alpha_y, pitch):
        """Attach the deflection maps of a GL_INTERPOL_MASS lens (gl_model_set_lens_maps): 2-D float32 host arrays of one shape."""
        ax, ay = np.ascontiguousarray(alpha_x, dtype=np.float32), np.ascontiguousarray(alpha_y, dtype=np.float32)
        if ax.ndim != 2 or ax.shape != ay.shape:
            raise NativeLibraryError(f"set_lens_maps: alpha_x {ax.shape} and alpha_y {ay.shape} must be 2-D arrays of one shape")
        with torch.cuda.device(self.device):
            _check(lib().gl_model_set_lens_maps(self._h, int(component), int(ax.shape[0]), int(ax.shape[1]),
                                                ax.ctypes.data_as(POINTER(c_float)), ay.ctypes.data_as(POINTER(c_float)), float(pitch)))
        self._changed(False)

    def _points(self, x, y, B):
        """``x, y`` broadcastable to ``(..., B)`` as contiguous ``[n_pts, B]`` tensors, and that shape."""
        x = torch.as_tensor(x, dtype=torch.float32, device=self.device)
        y = torch.as_tensor(y, dtype=torch.float32, device=self.device)
        shape = torch.broadcast_shapes(x.shape, y.shape, (B,))
        return x.expand(shape).reshape(-1, B).contiguous(), y.expand(shape).reshape(-1, B).contiguous(), shape

    def _scratch(self, name, nbytes):
        """The scratch workspace ``name`` of at least ``nbytes`` bytes, grown on demand."""
        ws = self._scratch_bufs.get(name)
        if ws is None or ws.numel() < nbytes:
            ws = self._scratch_bufs[name] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
        return ws

    def lens_maps(self, params, x, y):
        """gl_lens_maps: ``x, y`` broadcastable to ``(..., B)``; returns ``(6, ...)`` = beta_x, beta_y, f_xx, f_xy, f_yx, f_yy."""
        self._single_plane("lens_maps")
        params = self._params(params)
        B = params.shape[0]
        if x is None and y is None:  # the model's own grid (the only form series-expansion lenses accept)
            out = torch.empty((6, self.N, B), dtype=torch.float32, device=self.device)
            _check(lib().gl_lens_maps(self._h, _ptr(params), B, None, None, self.N, 0, _ptr(out), _stream()))
            return out
        xb, yb, shape = self._points(x, y, B)
        out = torch.empty((6,) + tuple(xb.shape), dtype=torch.float32, device=self.device)
        _check(lib().gl_lens_maps(self._h, _ptr(params), B, _ptr(xb), _ptr(yb), xb.shape[0], 1, _ptr(out), _stream()))
        return out.reshape((6,) + tuple(shape))

    def lens_maps_vjp(self, params, x, y, cot_x, cot_y):
        """gl_lens_maps_vjp: the cotangents ``cot_x, cot_y`` on ``lens_maps``' beta_x, beta_y (with ``x, y`` broadcastable to
        ``(..., B)``) -> the gradient on the packed rows ``[B, P]``; columns of no lens are 0.  Points whose cotangents are both
        exactly 0, or not finite, are skipped.  ``UnsupportedLensError``: series and user-written lenses, lens planes."""
        return self._vjp("gl_lens_maps_vjp", "lens_maps_vjp", params, x, y, (cot_x, cot_y))

    def lens_hessian_vjp(self, params, x, y, cot_xx, cot_xy, cot_yx, cot_yy):
        """gl_lens_hessian_vjp: the cotangents on ``lens_maps``' f_xx, f_xy, f_yx, f_yy (with ``x, y`` broadcastable to
        ``(..., B)``) -> the gradient on the packed rows ``[B, P]``; columns of no lens are 0.  Points whose four cotangents are all
        exactly 0, or one of which is not finite, are skipped.  ``UnsupportedLensError``: series and user-written lenses, lens
        planes."""
        return self._vjp("gl_lens_hessian_vjp", "lens_hessian_vjp", params, x, y, (cot_xx, cot_xy, cot_yx, cot_yy))

    def _vjp(self, symbol, name, params, x, y, cots):
        """The library's ``symbol`` (and its ``symbol_workspace_bytes``) on the cotangents ``cots``, each broadcastable to the points
        ``x, y``, with the scratch workspace ``name`` -> ``[B, P]``."""
        self._single_plane(name)
        params = self._params(params)
        B = params.shape[0]
        xb, yb, shape = self._points(x, y, B)
        cot = torch.stack([torch.as_tensor(c, dtype=torch.float32, device=self.device).expand(shape).reshape(-1, B)
                           for c in cots]).contiguous()
        n_pts = xb.shape[0]
        ws = self._scratch(name, getattr(lib(), symbol + "_workspace_bytes")(self._h, B, n_pts))
        out = torch.empty((B, self.P), dtype=torch.float32, device=self.device)
        _check_potential(getattr(lib(), symbol)(self._h, _ptr(params), B, _ptr(xb), _ptr(yb), n_pts, 1, _ptr(cot), _ptr(out), _ptr(ws),
                                                ws.numel(), _stream()))
        return out

    def shear_loglike(self, params, x, y, e1, e2, sigma, scales=None, want_grad=True, want_model=True):
        """gl_shear_loglike: the reduced-shear likelihood of the galaxies ``x, y, e1, e2, sigma`` (and ``scales`` or None: all 1),
        float32 ``[n_gal]`` device tensors.  Returns ``(log_like [B], chi2 [B], model_g [2, n_gal, B] or None, grad [B, P] or
        None)``.  ``UnsupportedLensError`` as ``lens_hessian_vjp``."""
        self._single_plane("shear_loglike")
        params = self._params(params)
        B = params.shape[0]
        tabs = [None if t is None else torch.as_tensor(t, dtype=torch.float32, device=self.device).contiguous()
                for t in (x, y, scales, e1, e2, sigma)]
        n_gal = int(tabs[0].numel())
        if any(t is not None and (t.dim() != 1 or t.numel() != n_gal) for t in tabs):
            raise ValueError(f"shear_loglike: x, y, e1, e2, sigma and scales must be 1-D arrays of one length ({n_gal})")
        ll = torch.empty(B, dtype=torch.float32, device=self.device)
        chi2 = torch.empty(B, dtype=torch.float32, device=self.device)
        model = torch.empty((2, n_gal, B), dtype=torch.float32, device=self.device) if want_model else None
        grad = torch.empty((B, self.P), dtype=torch.float32, device=self.device) if want_grad else None
        ws = self._scratch("shear_loglike", lib().gl_shear_loglike_workspace_bytes(self._h, B, n_gal, 1 if want_grad else 0))
        _check_potential(lib().gl_shear_loglike(self._h, _ptr(params), B, _ptr(tabs[0]), _ptr(tabs[1]), _ptr(tabs[2]), _ptr(tabs[3]),
                                                _ptr(tabs[4]), _ptr(tabs[5]), n_gal, _ptr(ll), _ptr(chi2), _ptr(model), _ptr(grad),
                                                _ptr(ws), ws.numel(), _stream()))
        return ll, chi2, model, grad

    def imgplane_loglike(self, params, image_table, family_table, family_offsets, source=None, tol=1e-6, max_iter=30, want_grad=True):
        """gl_imgplane_loglike: the image-plane position likelihood of the families whose tables are ``image_table`` (float32
        ``[5, J]`` device: x, y, sigma, cap, scale), ``family_table`` (int32 ``[3, J]`` device: family, first image, count) and
        ``family_offsets`` (int32 ``[F + 1]`` host); ``source`` None (the barycentre of every family) or ``[2, B, F]``.  Returns
        ``(log_like [B], chi2 [B], n_lost [B] int32, predicted [2, J, B], grad [B, P] or None, grad_source [2, B, F] or None)``.
        ``UnsupportedLensError`` as ``lens_maps_vjp``."""
        self._single_plane("imgplane_loglike")
        params = self._params(params)
        B = params.shape[0]
        off = np.ascontiguousarray(family_offsets, dtype=np.int32)
        J, F = int(image_table.shape[1]), int(off.size) - 1
        if tuple(image_table.shape) != (5, J) or tuple(family_table.shape) != (3, J) or image_table.dtype != torch.float32 or \
                family_table.dtype != torch.int32 or F < 1:
            raise ValueError("imgplane_loglike: image_table is float32 [5, J], family_table int32 [3, J], family_offsets [F + 1]")
        if source is not None:
            source = torch.as_tensor(source, dtype=torch.float32, device=self.device).contiguous()
            if tuple(source.shape) != (2, B, F):
                raise ValueError(f"imgplane_loglike: source has shape {tuple(source.shape)}, expected {(2, B, F)}")
        ll = torch.empty(B, dtype=torch.float32, device=self.device)
        chi2 = torch.empty(B, dtype=torch.float32, device=self.device)
        n_lost = torch.empty(B, dtype=torch.int32, device=self.device)
        pred = torch.empty((2, J, B), dtype=torch.float32, device=self.device)
        grad = torch.empty((B, self.P), dtype=torch.float32, device=self.device) if want_grad else None
        grad_src = torch.empty((2, B, F), dtype=torch.float32, device=self.device) if want_grad and source is not None else None
        ws = self._scratch("imgplane_loglike", lib().gl_imgplane_loglike_workspace_bytes(self._h, B, J, 0 if source is None else 1,
                                                                                        1 if want_grad else 0))
        _check_potential(lib().gl_imgplane_loglike(self._h, _ptr(params), B, _ptr(image_table.contiguous()), _ptr(family_table.contiguous()),
                                                   off.ctypes.data_as(POINTER(c_int32)), J, F, _ptr(source), float(tol), int(max_iter),
                                                   _ptr(ll), _ptr(chi2), _ptr(n_lost), _ptr(pred), _ptr(grad), _ptr(grad_src), _ptr(ws),
                                                   ws.numel(), _stream()))
        return ll, chi2, n_lost, pred, grad, grad_src

    def lens_potential(self, params, x, y):
        """gl_lens_potential: ``x, y`` broadcastable to ``(..., B)`` (or both None: the model's own grid, ``(N, B)``); returns psi."""
        self._single_plane("lens_potential")
        params = self._params(params)
        B = params.shape[0]
        if x is None and y is None:
            out = torch.empty((self.N, B), dtype=torch.float32, device=self.device)
            _check_potential(lib().gl_lens_potential(self._h, _ptr(params), B, None, None, self.N, 0, _ptr(out), _stream()))
            return out
        xb, yb, shape = self._points(x, y, B)
        out = torch.empty(tuple(xb.shape), dtype=torch.float32, device=self.device)
        _check_potential(lib().gl_lens_potential(self._h, _ptr(params), B, _ptr(xb), _ptr(yb), xb.shape[0], 1, _ptr(out), _stream()))
        return out.reshape(tuple(shape))

    def set_source_scales(self, scales):
        """One deflection scale per source light (gl_model_set_source_scales); a model with user-written profiles refuses
        scales != 1 with ``UnsupportedLensError``."""
        s = np.ascontiguousarray(scales, dtype=np.float32)
        with torch.cuda.device(self.device):
            _check_potential(lib().gl_model_set_source_scales(self._h, s.ctypes.data_as(POINTER(c_float)), int(s.size)))
        self._changed(True)  # the launch plan, and with it the workspace layout, follows the kernels that serve a scaled model

    def set_lens_planes(self, plane_of_lens, lens_scales, source_scales):
        """Lens planes at redshifts of their own (gl_model_set_lens_planes): ``plane_of_lens`` one int per lens, ``lens_scales``
        ``[K, K]``, ``source_scales`` ``[K, n_src]`` (``gigalens_amd.cosmology.MultiPlane``).  From here on the model is served by
        ``multiplane_maps`` / ``multiplane_simulate`` / ``multiplane_loglike`` and the gradients ``multiplane_simulate_bwd`` /
        ``multiplane_loglike_grad`` / ``multiplane_logprob`` / ``multiplane_positions``; the single-plane calls raise
        ``UnsupportedLensError``."""
        pl = np.ascontiguousarray(plane_of_lens, dtype=np.int32).reshape(-1)
        C = np.ascontiguousarray(lens_scales, dtype=np.float32)
        S = np.ascontiguousarray(source_scales, dtype=np.float32)
        if C.ndim != 2 or C.shape[0] != C.shape[1] or S.ndim != 2 or S.shape[0] != C.shape[0]:
            raise ValueError(f"lens_scales must be [K, K] and source_scales [K, n_src], got {C.shape} and {S.shape}")
        with torch.cuda.device(self.device):
            _check_potential(lib().gl_model_set_lens_planes(self._h, pl.ctypes.data_as(POINTER(c_int32)), int(pl.size), int(C.shape[0]),
                                                            C.ctypes.data_as(POINTER(c_float)), S.ctypes.data_as(POINTER(c_float)),
                                                            int(S.shape[1])))
        self.n_planes = int(C.shape[0])
        self._changed(True)  # the workspace holds the materialised image of the pixel statistics

    def _single_plane(self, what):
        if self.n_planes >= 2:
            raise UnsupportedLensError(f"{what} does not serve a model with {self.n_planes} lens planes: they are served by the "
                                       "multiplane_* calls alone (lens maps, renders, pixel statistics and their gradients)")

    def multiplane_maps(self, params, x, y, target_scales, shared_points=False):
        """gl_multiplane_maps: ``lens_maps`` of the target plane with couplings ``target_scales`` ``[K]``; ``(6, ...)`` = beta_x, beta_y
        and ``f = I - A`` (f_xx, f_xy, f_yx, f_yy).  ``shared_points``: ``x, y`` are ``[n]`` points every sample shares (not replicated
        per sample on the device); the result is ``(6, n, B)``."""
        params = self._params(params)
        B = params.shape[0]
        t = np.ascontiguousarray(target_scales, dtype=np.float32).reshape(-1)
        if shared_points:
            xs = torch.as_tensor(x, dtype=torch.float32, device=self.device).reshape(-1).contiguous()
            ys = torch.as_tensor(y, dtype=torch.float32, device=self.device).reshape(-1).contiguous()
            if xs.numel() != ys.numel() or xs.numel() == 0:
                raise NativeLibraryError(f"multiplane_maps: x and y must hold the same number of points, got {xs.numel()} and {ys.numel()}")
            out = torch.empty((6, xs.numel(), B), dtype=torch.float32, device=self.device)
            _check_potential(lib().gl_multiplane_maps(self._h, _ptr(params), B, _ptr(xs), _ptr(ys), xs.numel(), 0,
                                                      t.ctypes.data_as(POINTER(c_float)), int(t.size), _ptr(out), _stream()))
            return out
        xb, yb, shape = self._points(x, y, B)
        out = torch.empty((6,) + tuple(xb.shape), dtype=torch.float32, device=self.device)
        _check_potential(lib().gl_multiplane_maps(self._h, _ptr(params), B, _ptr(xb), _ptr(yb), xb.shape[0], 1,
                                                  t.ctypes.data_as(POINTER(c_float)), int(t.size), _ptr(out), _stream()))
        return out.reshape((6,) + tuple(shape))

    def multiplane_simulate(self, params, parts=7):
        """gl_multiplane_simulate: the image ``[B, H, W]`` of ``parts`` (1 deflect, 2 lens light, 4 source light)."""
        return self._render(lib().gl_multiplane_simulate, _check_potential, params, parts)

    def multiplane_loglike(self, params, obs, err, mask, bg_rms, exp_time):
        """gl_multiplane_loglike: ``(loglike, chi2)`` ``[B]`` of the multi-plane image, forward only."""
        return self._loglike(lib().gl_multiplane_loglike, _check_potential, params, obs, err, mask, bg_rms, exp_time, None)[:2]

    def multiplane_simulate_bwd(self, params, grad_img):
        """gl_multiplane_simulate_bwd: the VJP of ``multiplane_simulate`` (every part), ``grad_img`` ``[B, H, W]`` -> ``[B, P]``."""
        return self._render_bwd(lib().gl_multiplane_simulate_bwd, _check_potential, params, grad_img)

    def multiplane_loglike_grad(self, params, obs, err, mask, bg_rms, exp_time):
        """gl_multiplane_loglike_fwd_bwd: ``(loglike, chi2, d loglike / d params)``; the first two are ``multiplane_loglike``'s bits."""
        return self._loglike(lib().gl_multiplane_loglike_fwd_bwd, _check_potential, params, obs, err, mask, bg_rms, exp_time, True)

    def multiplane_logprob(self, z, obs, err, mask, bg_rms, exp_time, want_grad, chi2_divisor=1.0, terms=1):
        """gl_multiplane_logprob_fwd_bwd: ``(logprob, loglike, red_chi2, d logprob / d z or None)`` of ``terms`` (1 pixels, 2 image
        positions -- after ``set_positions`` and ``set_position_targets`` --, 3 both)."""
        return self._logprob(lib().gl_multiplane_logprob_fwd_bwd, _check_potential, z, obs, err, mask, bg_rms, exp_time, want_grad,
                             chi2_divisor, terms)

    def set_position_targets(self, targets):
        """The couplings ``[F, K]`` of every image family's plane (gl_model_set_position_targets; after ``set_positions`` and
        ``set_lens_planes``, either of which resets them): row f = ``MultiPlane.target_scales(z_f)``."""
        t = np.ascontiguousarray(targets, dtype=np.float32)
        if t.ndim != 2:
            raise ValueError(f"targets must be [n_families, n_planes], got {t.shape}")
        with torch.cuda.device(self.device):
            _check_potential(lib().gl_model_set_position_targets(self._h, t.ctypes.data_as(POINTER(c_float)), int(t.shape[0]),
                                                                 int(t.shape[1])))
        self._changed(False)

    def multiplane_positions(self, params, want_grad):
        """gl_multiplane_positions_fwd_bwd: ``(loglike, chi2, d loglike / d params or None)`` of the image-position likelihood with
        every family traced through the lens planes in front of it."""
        return self._positions(lib().gl_multiplane_positions_fwd_bwd, _check_potential, params, want_grad)

    def set_position_scales(self, scales):
        """One deflection scale per image family (gl_model_set_position_scales; after ``set_positions``, which resets them)."""
        s = np.ascontiguousarray(scales, dtype=np.float32)
        with torch.cuda.device(self.device):
            _check(lib().gl_model_set_position_scales(self._h, s.ctypes.data_as(POINTER(c_float)), int(s.size)))
        self._changed(False)

    def set_position_fluxes(self, fluxes, errors):
        """The measured fluxes of the images and their errors (gl_model_set_position_fluxes; after ``set_positions``, which clears
        them): ``[J]`` arrays in the concatenated image order, NaN for an image without a measurement; ``None``: no fluxes."""
        fp = lambda a: a.ctypes.data_as(POINTER(c_float))
        with torch.cuda.device(self.device):
            if fluxes is None:
                _check(lib().gl_model_set_position_fluxes(self._h, None, None, 0))
            else:
                F = np.ascontiguousarray(fluxes, dtype=np.float32).reshape(-1)
                s = np.ascontiguousarray(errors, dtype=np.float32).reshape(-1)
                if F.size != s.size:
                    raise NativeLibraryError("fluxes and their errors must have the same length")
                _check(lib().gl_model_set_position_fluxes(self._h, fp(F), fp(s), int(F.size)))
        self._changed(False)

    def position_fluxes(self, params, want_grad, want_model=False):
        """gl_position_fluxes_fwd_bwd: ``(loglike, chi2, d loglike / d params or None)`` of the flux-ratio term on one plane or on
        lens planes; with ``want_model`` also ``(amplitude [B, F], model_flux [B, J])``."""
        return self._positions(lib().gl_position_fluxes_fwd_bwd, _check_potential, params, want_grad,
                               (self.n_families, self.n_images), want_model)

    def set_position_delays(self, delays, errors, scales):
        """The measured arrival times of the images (days) and their errors (gl_model_set_position_delays; after ``set_positions``,
        which clears them): ``[J]`` arrays in the concatenated image order, NaN for an image without a measurement; ``scales`` ``[F]``:
        ``lambda_f`` in days / arcsec^2, NaN to profile it out.  ``delays`` None: no delays.  Lens planes, a scaled family, series
        and user-written lenses raise ``UnsupportedLensError`` and leave the model as it was."""
        fp = lambda a: a.ctypes.data_as(POINTER(c_float))
        with torch.cuda.device(self.device):
            if delays is None:
                _check(lib().gl_model_set_position_delays(self._h, None, None, 0, None, 0))
            else:
                t = np.ascontiguousarray(delays, dtype=np.float32).reshape(-1)
                s = np.ascontiguousarray(errors, dtype=np.float32).reshape(-1)
                lam = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1)
                if t.size != s.size:
                    raise NativeLibraryError("arrival times and their errors must have the same length")
                _check_potential(lib().gl_model_set_position_delays(self._h, fp(t), fp(s), int(t.size), fp(lam), int(lam.size)))
        self._changed(False)

    def position_delays(self, params, want_grad, want_model=False):
        """gl_position_delays_fwd_bwd: ``(loglike, chi2, d loglike / d params or None)`` of the time-delay term; with ``want_model``
        also ``(scale [B, F], offset [B, F], model_delay [B, J])`` = ``lambda_f``, ``T_f`` and ``lambda_f phi_j + T_f`` in days."""
        return self._positions(lib().gl_position_delays_fwd_bwd, _check_potential, params, want_grad,
                               (self.n_families, self.n_families, self.n_images), want_model)

    def set_position_plane_delays(self, delays, errors, geom, pot, scales):
        """The measured arrival times of the images of a model with lens planes (gl_model_set_position_plane_delays; after
        ``set_positions``, ``set_lens_planes`` and ``set_position_targets``, each of which clears them): ``delays``, ``errors`` ``[J]``
        and ``scales`` ``[F]`` as ``set_position_delays`` -- ``lambda_f`` in days per (arcsec^2 c / H0), NaN to profile it out --,
        ``geom`` ``[F, K]`` and ``pot`` ``[K]`` float64: the weights of ``MultiPlane.delay_weights``.  ``delays`` None: no delays.  The
        workspace grows while the model holds plane delays: the cached workspaces are dropped.  A lens without a potential raises
        ``UnsupportedLensError`` and leaves the model as it was."""
        fp, dp = (lambda a: a.ctypes.data_as(POINTER(c_float))), (lambda a: a.ctypes.data_as(POINTER(c_double)))
        with torch.cuda.device(self.device):
            if delays is None:
                _check(lib().gl_model_set_position_plane_delays(self._h, None, None, 0, None, None, None, 0, 0))
            else:
                t = np.ascontiguousarray(delays, dtype=np.float32).reshape(-1)
                s = np.ascontiguousarray(errors, dtype=np.float32).reshape(-1)
                lam = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1)
                g, v = np.ascontiguousarray(geom, dtype=np.float64), np.ascontiguousarray(pot, dtype=np.float64).reshape(-1)
                if t.size != s.size:
                    raise NativeLibraryError("arrival times and their errors must have the same length")
                if g.ndim != 2 or g.shape != (lam.size, v.size):
                    raise NativeLibraryError(f"geom must be [n_families = {lam.size}, n_planes = {v.size}], got {g.shape}")
                _check_potential(lib().gl_model_set_position_plane_delays(self._h, fp(t), fp(s), int(t.size), dp(g), dp(v), fp(lam),
                                                                          int(lam.size), int(v.size)))
        self._changed(True)  # the workspace grows with the plane delays

    def multiplane_position_delays(self, params, want_grad, want_model=False):
        """gl_multiplane_position_delays_fwd_bwd: ``position_delays`` on lens planes -- ``(loglike, chi2, d loglike / d params or
        None)`` of the time-delay term; with ``want_model`` also ``(scale [B, F], offset [B, F], model_delay [B, J])`` = ``lambda_f``
        in days per (arcsec^2 c / H0), ``T_f`` and ``lambda_f phi_j + T_f`` in days."""
        return self._positions(lib().gl_multiplane_position_delays_fwd_bwd, _check_potential, params, want_grad,
                               (self.n_families, self.n_families, self.n_images), want_model)

    def position_family_terms(self, B):
        """gl_position_family_terms: ``[B, F, 2]`` = (log_like, chi2) of every (sample, family) as the most recent point-likelihood call
        on ``B`` samples (any of the position / flux / delay entries, or the fused log-prob with its position term) left them in the
        workspace.  A copy, no launch."""
        ws = self._workspace(B)
        out = torch.empty((B, self.n_families, 2), dtype=torch.float32, device=self.device)
        _check(lib().gl_position_family_terms(self._h, _ptr(ws), ws.numel(), B, _ptr(out), _stream()))
        return out

    def image_positions(self, params, src_x, src_y, window, n_cells, max_images, tol, max_iter, scales=None):
        """gl_image_positions[_scaled]: ``src_x, src_y`` [B, S] on the device, ``window`` = (x_lo, x_hi, y_lo, y_hi), ``scales``
        [S] on the host or None.  Returns
        ``out`` [B, S, max_images, 3] (x, y, mu; NaN-padded), ``n_images`` and ``n_dropped`` [B, S] (int32)."""
        self._single_plane("image_positions")
        params = self._params(params)
        B = params.shape[0]
        src_x = src_x.to(device=self.device, dtype=torch.float32).contiguous()
        src_y = src_y.to(device=self.device, dtype=torch.float32).contiguous()
        if src_x.shape != src_y.shape or src_x.dim() != 2 or src_x.shape[0] != B:
            raise NativeLibraryError(f"source positions must be [B={B}, S], got {tuple(src_x.shape)} / {tuple(src_y.shape)}")
        S = src_x.shape[1]
        nbytes = lib().gl_image_positions_workspace_bytes(self._h, B, S, int(n_cells), int(max_images))
        ws = self._scratch("image_positions", nbytes)
        out = torch.empty((B, S, max(int(max_images), 1), 3), dtype=torch.float32, device=self.device)
        n_images = torch.empty((B, S), dtype=torch.int32, device=self.device)
        n_dropped = torch.empty_like(n_images)
        x_lo, x_hi, y_lo, y_hi = (float(v) for v in window)
        if scales is None:
            _check(lib().gl_image_positions(self._h, _ptr(params), B, _ptr(src_x), _ptr(src_y), S, x_lo, x_hi, y_lo, y_hi,
                                            int(n_cells), int(max_images), float(tol), int(max_iter), _ptr(out), _ptr(n_images),
                                            _ptr(n_dropped), _ptr(ws), ws.numel(), _stream()))
        else:
            sc = np.ascontiguousarray(scales, dtype=np.float32)
            _check(lib().gl_image_positions_scaled(self._h, _ptr(params), B, _ptr(src_x), _ptr(src_y), S,
                                                   sc.ctypes.data_as(POINTER(c_float)), x_lo, x_hi, y_lo, y_hi, int(n_cells),
                                                   int(max_images), float(tol), int(max_iter), _ptr(out), _ptr(n_images),
                                                   _ptr(n_dropped), _ptr(ws), ws.numel(), _stream()))
        return out, n_images, n_dropped

    def multiplane_image_positions(self, params, src_x, src_y, targets, window, n_cells, max_images, tol, max_iter):
        """gl_multiplane_image_positions: ``image_positions`` on lens planes, source s on the plane with the couplings ``targets[s]``
        (``[S, K]`` on the host: ``MultiPlane.target_scales(z_s)``).  Returns ``out`` [B, S, max_images, 3] (x, y, mu on the source's
        plane; NaN-padded), ``n_images`` and ``n_dropped`` [B, S] (int32)."""
        params = self._params(params)
        B = params.shape[0]
        src_x = src_x.to(device=self.device, dtype=torch.float32).contiguous()
        src_y = src_y.to(device=self.device, dtype=torch.float32).contiguous()
        if src_x.shape != src_y.shape or src_x.dim() != 2 or src_x.shape[0] != B:
            raise NativeLibraryError(f"source positions must be [B={B}, S], got {tuple(src_x.shape)} / {tuple(src_y.shape)}")
        S = src_x.shape[1]
        t = np.ascontiguousarray(targets, dtype=np.float32)
        if t.ndim != 2 or t.shape[0] != S:
            raise NativeLibraryError(f"targets must be [S={S}, n_planes], got {t.shape}")
        nbytes = lib().gl_multiplane_image_positions_workspace_bytes(self._h, B, S, int(n_cells), int(max_images))
        ws = self._scratch("multiplane_image_positions", nbytes)
        out = torch.empty((B, S, max(int(max_images), 1), 3), dtype=torch.float32, device=self.device)
        n_images = torch.empty((B, S), dtype=torch.int32, device=self.device)
        n_dropped = torch.empty_like(n_images)
        x_lo, x_hi, y_lo, y_hi = (float(v) for v in window)
        _check_potential(lib().gl_multiplane_image_positions(self._h, _ptr(params), B, _ptr(src_x), _ptr(src_y), S,
                                                             t.ctypes.data_as(POINTER(c_float)), int(t.shape[1]), x_lo, x_hi, y_lo,
                                                             y_hi, int(n_cells), int(max_images), float(tol), int(max_iter), _ptr(out),
                                                             _ptr(n_images), _ptr(n_dropped), _ptr(ws), ws.numel(), _stream()))
        return out, n_images, n_dropped

    def multiplane_fermat(self, params, x, y, src_x, src_y, geom, pot):
        """gl_multiplane_fermat: the arrival time ``T`` of rays from the points ``x, y`` ``[B, S, M]`` (NaN = no point) to the sources
        ``src_x, src_y`` ``[B, S]`` behind lens planes, float64 ``[B, S, M]``.  ``geom`` ``[S, K]`` and ``pot`` ``[K]`` on the host
        (``MultiPlane.delay_weights(z_s)``); ``T`` is in arcsec^2 times their unit.  ``UnsupportedLensError``: a lens without a
        potential."""
        params = self._params(params)
        B = params.shape[0]
        x = torch.as_tensor(x).to(device=self.device, dtype=torch.float32).contiguous()
        y = torch.as_tensor(y).to(device=self.device, dtype=torch.float32).contiguous()
        src_x = torch.as_tensor(src_x).to(device=self.device, dtype=torch.float32).contiguous()
        src_y = torch.as_tensor(src_y).to(device=self.device, dtype=torch.float32).contiguous()
        if x.shape != y.shape or x.dim() != 3 or x.shape[0] != B or x.numel() == 0:
            raise NativeLibraryError(f"points must be [B={B}, S, M], got {tuple(x.shape)} / {tuple(y.shape)}")
        S, M = int(x.shape[1]), int(x.shape[2])
        if src_x.shape != (B, S) or src_y.shape != (B, S):
            raise NativeLibraryError(f"source positions must be [B={B}, S={S}], got {tuple(src_x.shape)} / {tuple(src_y.shape)}")
        g = np.ascontiguousarray(geom, dtype=np.float64)
        v = np.ascontiguousarray(pot, dtype=np.float64).reshape(-1)
        if g.ndim != 2 or g.shape[0] != S or g.shape[1] != v.size:
            raise NativeLibraryError(f"geom must be [S={S}, n_planes] and pot [n_planes], got {g.shape} and {v.shape}")
        ws = self._scratch("multiplane_fermat", lib().gl_multiplane_fermat_workspace_bytes(self._h, S))
        out = torch.empty((B, S, M), dtype=torch.float64, device=self.device)
        _check_potential(lib().gl_multiplane_fermat(self._h, _ptr(params), B, _ptr(x), _ptr(y), _ptr(src_x), _ptr(src_y), S, M,
                                                    g.ctypes.data_as(POINTER(c_double)), v.ctypes.data_as(POINTER(c_double)),
                                                    int(v.size), _ptr(out), _ptr(ws), ws.numel(), _stream()))
        return out

    def image_positions_stage_counts(self, B, n_src, n_cells):
        """gl_image_positions_stage_counts: ``n_cand``, ``n_over`` [B, n_src] (int32) of the scan stage, out of the workspace the
        last ``image_positions`` call of these sizes filled (read-only; for tests and diagnostics)."""
        ws = self._scratch_bufs.get("image_positions")
        if ws is None:
            raise NativeLibraryError("image_positions_stage_counts: no image_positions call has filled a workspace yet")
        n_cand = torch.empty((int(B), int(n_src)), dtype=torch.int32, device=self.device)
        n_over = torch.empty_like(n_cand)
        _check_potential(lib().gl_image_positions_stage_counts(self._h, int(B), int(n_src), int(n_cells), _ptr(ws), ws.numel(),
                                                               _ptr(n_cand), _ptr(n_over), _stream()))
        return n_cand, n_over

    def multiplane_image_positions_stage_counts(self, B, n_src, n_cells):
        """gl_multiplane_image_positions_stage_counts: ``n_cand``, ``n_over`` [B, n_src] (int32) of the scan stage, out of the
        workspace the last ``multiplane_image_positions`` call of these sizes filled (read-only; for tests and diagnostics)."""
        ws = self._scratch_bufs.get("multiplane_image_positions")
        if ws is None:
            raise NativeLibraryError("multiplane_image_positions_stage_counts: no multiplane_image_positions call has filled a "
                                     "workspace yet")
        n_cand = torch.empty((int(B), int(n_src)), dtype=torch.int32, device=self.device)
        n_over = torch.empty_like(n_cand)
        _check_potential(lib().gl_multiplane_image_positions_stage_counts(self._h, int(B), int(n_src), int(n_cells), _ptr(ws),
                                                                          ws.numel(), _ptr(n_cand), _ptr(n_over), _stream()))
        return n_cand, n_over

    def critical_curves(self, params, window, n_cells, max_segments, scale=None):
        """gl_critical_curves[_scaled]: ``scale`` the deflection scale of the source plane or None; ``window`` = (x_lo, x_hi, y_lo, y_hi).  Returns ``seg``, ``cau`` [B, max_segments, 2, 2] (NaN-padded),
        ``kind`` [B, max_segments] (int32; -1 padding), ``n_seg``, ``n_dropped``, ``n_flagged``, ``open`` [B] (int32) and the signed
        ``area`` [B, 4].  Series-expansion and user-written lenses raise ``UnsupportedLensError``."""
        self._single_plane("critical_curves")
        params = self._params(params)
        B, M = params.shape[0], int(max_segments)
        nbytes = lib().gl_critical_curves_workspace_bytes(self._h, B, int(n_cells), M)
        ws = self._scratch("critical_curves", nbytes)
        seg = torch.empty((B, max(M, 1), 2, 2), dtype=torch.float32, device=self.device)
        cau = torch.empty_like(seg)
        kind = torch.empty((B, max(M, 1)), dtype=torch.int32, device=self.device)
        n_seg, n_dropped, n_flagged, opened = (torch.empty((B,), dtype=torch.int32, device=self.device) for _ in range(4))
        area = torch.empty((B, 4), dtype=torch.float32, device=self.device)
        x_lo, x_hi, y_lo, y_hi = (float(v) for v in window)
        if scale is None:
            _check_potential(lib().gl_critical_curves(self._h, _ptr(params), B, x_lo, x_hi, y_lo, y_hi, int(n_cells), M, _ptr(seg),
                                                      _ptr(cau), _ptr(kind), _ptr(n_seg), _ptr(n_dropped), _ptr(n_flagged),
                                                      _ptr(opened), _ptr(area), _ptr(ws), ws.numel(), _stream()))
        else:
            _check_potential(lib().gl_critical_curves_scaled(self._h, _ptr(params), B, x_lo, x_hi, y_lo, y_hi, int(n_cells), M,
                                                             float(scale), _ptr(seg), _ptr(cau), _ptr(kind), _ptr(n_seg),
                                                             _ptr(n_dropped), _ptr(n_flagged), _ptr(opened), _ptr(area), _ptr(ws),
                                                             ws.numel(), _stream()))
        return seg, cau, kind, n_seg, n_dropped, n_flagged, opened, area

    def multiplane_critical_curves(self, params, targets, window, n_cells, max_segments):
        """gl_multiplane_critical_curves: ``critical_curves`` on lens planes, once per source plane with the couplings ``targets[s]``
        (``[S, K]`` on the host: ``MultiPlane.target_scales(z_s)``).  Returns ``seg``, ``cau`` [B, S, max_segments, 2, 2]
        (NaN-padded), ``kind`` [B, S, max_segments] (int32; -1 padding), ``n_seg``, ``n_dropped``, ``n_flagged``, ``open`` [B, S]
        (int32) and the signed ``area`` [B, S, 4]."""
        params = self._params(params)
        B, M = params.shape[0], int(max_segments)
        t = np.ascontiguousarray(targets, dtype=np.float32)
        if t.ndim != 2 or t.shape[0] < 1:
            raise NativeLibraryError(f"targets must be [S >= 1, n_planes], got {t.shape}")
        S = int(t.shape[0])
        nbytes = lib().gl_multiplane_critical_curves_workspace_bytes(self._h, B, S, int(n_cells), M)
        ws = self._scratch("multiplane_critical_curves", nbytes)
        seg = torch.empty((B, S, max(M, 1), 2, 2), dtype=torch.float32, device=self.device)
        cau = torch.empty_like(seg)
        kind = torch.empty((B, S, max(M, 1)), dtype=torch.int32, device=self.device)
        n_seg, n_dropped, n_flagged, opened = (torch.empty((B, S), dtype=torch.int32, device=self.device) for _ in range(4))
        area = torch.empty((B, S, 4), dtype=torch.float32, device=self.device)
        x_lo, x_hi, y_lo, y_hi = (float(v) for v in window)
        _check_potential(lib().gl_multiplane_critical_curves(self._h, _ptr(params), B, t.ctypes.data_as(POINTER(c_float)), S,
                                                             int(t.shape[1]), x_lo, x_hi, y_lo, y_hi, int(n_cells), M, _ptr(seg),
                                                             _ptr(cau), _ptr(kind), _ptr(n_seg), _ptr(n_dropped), _ptr(n_flagged),
                                                             _ptr(opened), _ptr(area), _ptr(ws), ws.numel(), _stream()))
        return seg, cau, kind, n_seg, n_dropped, n_flagged, opened, area

    def pixsrc_reconstruct(self, beta_x, beta_y, obs, sigma, lens_light, pix, n_src, pose, regularization, strength):
        """gl_pixsrc_reconstruct: ``beta_x, beta_y`` [B, Hs Ws], ``obs, sigma`` [B, n_used], ``lens_light`` [B, H, W] or None, ``pix``
        [n_used] int32, ``pose`` [B, 3] (pitch, cx, cy), ``strength`` [B, L], all on the device; ``regularization`` 0, 1 or 2.
        Returns ``source`` [B, L, ny, nx], ``model_image`` [B, L, H, W], ``scalars`` [B, L, 3] (float64: chi2, s^T R s, log det M)
        and ``ok`` [B, L] (int32)."""
        self._single_plane("pixsrc_reconstruct")
        ny, nx = (int(v) for v in n_src)
        B, L, n_used = int(beta_x.shape[0]), int(strength.shape[1]), int(pix.numel())
        f32 = lambda t, shape, what: self._pix_tensor(t, torch.float32, shape, what)
        beta_x, beta_y = f32(beta_x, (B, self.ss_h * self.ss_w), "beta_x"), f32(beta_y, (B, self.ss_h * self.ss_w), "beta_y")
        obs, sigma = f32(obs, (B, n_used), "obs"), f32(sigma, (B, n_used), "sigma")
        pose, strength = f32(pose, (B, 3), "pose"), f32(strength, (B, L), "strength")
        pix = self._pix_tensor(pix, torch.int32, (n_used,), "pix")
        if lens_light is not None:
            lens_light = f32(lens_light, (B, self.out_h, self.out_w), "lens_light")
        nbytes = lib().gl_pixsrc_workspace_bytes(self._h, B, L, ny, nx, n_used)
        ws = self._scratch("pixsrc", nbytes)
        source = torch.empty((B, L, ny, nx), dtype=torch.float32, device=self.device)
        image = torch.empty((B, L, self.out_h, self.out_w), dtype=torch.float32, device=self.device)
        scalars = torch.empty((B, L, 3), dtype=torch.float64, device=self.device)
        ok = torch.empty((B, L), dtype=torch.int32, device=self.device)
        _check(lib().gl_pixsrc_reconstruct(self._h, _ptr(beta_x), _ptr(beta_y), B, _ptr(obs), _ptr(sigma), _ptr(lens_light),
                                                     _ptr(pix), n_used, ny, nx, _ptr(pose), int(regularization), _ptr(strength), L,
                                                     _ptr(source), _ptr(image), _ptr(scalars), _ptr(ok), _ptr(ws), ws.numel(),
                                                     _stream()))
        return source, image, scalars, ok

    def pixsrc_evidence_grad(self, beta_x, beta_y, obs, sigma, lens_light, pix, n_src, pose, regularization, strength):
        """gl_pixsrc_evidence_grad: the arguments of ``pixsrc_reconstruct`` with ``strength`` [B].  Returns ``source`` [B, ny, nx],
        ``model_image`` [B, H, W], ``scalars`` [B, 3] and ``ok`` [B] (the bits of ``pixsrc_reconstruct``), ``grad_beta``
        [2, B, Hs Ws] (d E / d beta_x, beta_y) and ``grad_image`` [B, H, W] (d E / d lens-light image)."""
        self._single_plane("pixsrc_evidence_grad")
        ny, nx = (int(v) for v in n_src)
        B, n_used = int(beta_x.shape[0]), int(pix.numel())
        f32 = lambda t, shape, what: self._pix_tensor(t, torch.float32, shape, what)
        beta_x, beta_y = f32(beta_x, (B, self.ss_h * self.ss_w), "beta_x"), f32(beta_y, (B, self.ss_h * self.ss_w), "beta_y")
        obs, sigma = f32(obs, (B, n_used), "obs"), f32(sigma, (B, n_used), "sigma")
        pose, strength = f32(pose, (B, 3), "pose"), f32(strength, (B,), "strength")
        pix = self._pix_tensor(pix, torch.int32, (n_used,), "pix")
        if lens_light is not None:
            lens_light = f32(lens_light, (B, self.out_h, self.out_w), "lens_light")
        ws = self._scratch("pixsrc_grad", lib().gl_pixsrc_grad_workspace_bytes(self._h, B, ny, nx, n_used))
        dev = self.device
        source = torch.empty((B, ny, nx), dtype=torch.float32, device=dev)
        image = torch.empty((B, self.out_h, self.out_w), dtype=torch.float32, device=dev)
        scalars = torch.empty((B, 3), dtype=torch.float64, device=dev)
        ok = torch.empty((B,), dtype=torch.int32, device=dev)
        grad_beta = torch.empty((2, B, self.ss_h * self.ss_w), dtype=torch.float32, device=dev)
        grad_image = torch.empty((B, self.out_h, self.out_w), dtype=torch.float32, device=dev)
        _check(lib().gl_pixsrc_evidence_grad(self._h, _ptr(beta_x), _ptr(beta_y), B, _ptr(obs), _ptr(sigma), _ptr(lens_light), _ptr(pix),
                                             n_used, ny, nx, _ptr(pose), int(regularization), _ptr(strength), _ptr(source), _ptr(image),
                                             _ptr(scalars), _ptr(ok), _ptr(grad_beta), _ptr(grad_image), _ptr(ws), ws.numel(),
                                             _stream()))
        return source, image, scalars, ok, grad_beta, grad_image

    # -- point images in the pixel likelihood (gl_ptimg_*) -------------------------------------------------------------
    def _ptimg_inputs(self, what, transform, *rows):
        """``rows``: ``[B, J]`` float32 device tensors of one shape; returns them contiguous with ``B``, ``J``, the transform as six
        C doubles and the call's workspace."""
        self._single_plane(what)
        shape = tuple(rows[0].shape)
        out = []
        for t in rows:
            _require_cuda(t, what)
            if t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != shape:
                raise NativeLibraryError(f"{what}: positions and amplitudes must be float32 [B, J] of one shape, got {t.dtype} "
                                         f"{tuple(t.shape)} against {shape}")
            out.append(t.contiguous())
        B, J = shape
        xf = (ctypes.c_double * 6)(*[float(v) for v in transform])
        nbytes = lib().gl_ptimg_workspace_bytes(self._h, B, J)
        return out, B, J, xf, self._scratch("ptimg", nbytes)

    def _ptimg_image(self, t, B, what, name):
        """``[H, W]`` or ``[B, H, W]`` float32 on the device -> (contiguous tensor, batched flag)"""
        _require_cuda(t, name)
        if t.dtype != torch.float32 or tuple(t.shape) not in ((self.out_h, self.out_w), (B, self.out_h, self.out_w)):
            raise NativeLibraryError(f"{what}: {name} must be float32 [{self.out_h}, {self.out_w}] or [{B}, {self.out_h}, "
                                     f"{self.out_w}], got {t.dtype} {tuple(t.shape)}")
        return t.contiguous(), int(t.dim() == 3)

    def ptimg_render(self, x, y, amplitude, transform):
        """gl_ptimg_render: ``x, y, amplitude`` [B, J] on the device, ``transform`` = (x0, y0, m00, m01, m10, m11) on the host
        -> the image ``sum_j amplitude_j D_j`` [B, H, W]."""
        (x, y, amplitude), B, J, xf, ws = self._ptimg_inputs("ptimg_render", transform, x, y, amplitude)
        image = torch.empty((B, self.out_h, self.out_w), dtype=torch.float32, device=self.device)
        _check_potential(lib().gl_ptimg_render(self._h, _ptr(x), _ptr(y), _ptr(amplitude), B, J, xf, _ptr(image), _ptr(ws), ws.numel(),
                                               _stream()))
        return image

    def ptimg_render_bwd(self, x, y, amplitude, transform, grad_image):
        """gl_ptimg_render_bwd: the transpose of ``ptimg_render``; ``grad_image`` [B, H, W] -> ``grad_x, grad_y, grad_amplitude``
        [B, J]."""
        (x, y, amplitude), B, J, xf, ws = self._ptimg_inputs("ptimg_render_bwd", transform, x, y, amplitude)
        _require_cuda(grad_image, "grad_image")
        if grad_image.dtype != torch.float32 or tuple(grad_image.shape) != (B, self.out_h, self.out_w):
            raise NativeLibraryError(f"ptimg_render_bwd: grad_image must be float32 [{B}, {self.out_h}, {self.out_w}], got "
                                     f"{grad_image.dtype} {tuple(grad_image.shape)}")
        grad_image = grad_image.contiguous()
        gx, gy, ga = (torch.empty((B, J), dtype=torch.float32, device=self.device) for _ in range(3))
        _check_potential(lib().gl_ptimg_render_bwd(self._h, _ptr(x), _ptr(y), _ptr(amplitude), B, J, xf, _ptr(grad_image), _ptr(gx),
                                                   _ptr(gy), _ptr(ga), _ptr(ws), ws.numel(), _stream()))
        return gx, gy, ga

    def ptimg_fit(self, x, y, transform, extended, observed, weight, want_grad):
        """gl_ptimg_fit: ``x, y`` [B, J], ``extended`` [B, H, W], ``observed`` and ``weight`` [H, W] or [B, H, W] (``weight`` = 1 / err^2
        on the used pixels, 0 elsewhere).  Returns ``amplitude`` [B, J], ``model_image``, ``cotangent_image`` [B, H, W], ``chi2`` [B]
        (float64), ``ok`` [B] (int32) and, with ``want_grad``, ``grad_x, grad_y`` [B, J] (else None twice)."""
        (x, y), B, J, xf, ws = self._ptimg_inputs("ptimg_fit", transform, x, y)
        extended, _ = self._ptimg_image(extended, B, "ptimg_fit", "extended")
        if extended.dim() != 3:
            raise NativeLibraryError(f"ptimg_fit: extended must be [{B}, {self.out_h}, {self.out_w}], got {tuple(extended.shape)}")
        observed, obs_b = self._ptimg_image(observed, B, "ptimg_fit", "observed")
        weight, w_b = self._ptimg_image(weight, B, "ptimg_fit", "weight")
        dev = self.device
        amp = torch.empty((B, J), dtype=torch.float32, device=dev)
        model = torch.empty((B, self.out_h, self.out_w), dtype=torch.float32, device=dev)
        cot = torch.empty((B, self.out_h, self.out_w), dtype=torch.float32, device=dev)
        chi2 = torch.empty((B,), dtype=torch.float64, device=dev)
        ok = torch.empty((B,), dtype=torch.int32, device=dev)
        gx = torch.empty((B, J), dtype=torch.float32, device=dev) if want_grad else None
        gy = torch.empty((B, J), dtype=torch.float32, device=dev) if want_grad else None
        _check_potential(lib().gl_ptimg_fit(self._h, _ptr(x), _ptr(y), B, J, xf, _ptr(extended), _ptr(observed), obs_b, _ptr(weight), w_b,
                                            int(bool(want_grad)), _ptr(amp), _ptr(model), _ptr(cot), _ptr(chi2), _ptr(ok), _ptr(gx),
                                            _ptr(gy), _ptr(ws), ws.numel(), _stream()))
        return amp, model, cot, chi2, ok, gx, gy

    def pixsrc_grad_layout(self, B, n_src, n_used):
        """gl_pixsrc_grad_layout: ``dict(cb, pc, n_pad)`` -- samples per chunk, planes per post-processing launch and the padded row
        length of a ``pixsrc_evidence_grad`` call of these sizes (host only)."""
        out = (c_int32 * 3)()
        _check(lib().gl_pixsrc_grad_layout(self._h, int(B), int(n_src[0]), int(n_src[1]), int(n_used), out))
        return dict(zip(("cb", "pc", "n_pad"), (int(v) for v in out)))

    def pixsrc_layout(self, B, n_strength, n_src, n_used):
        """gl_pixsrc_layout: ``dict(cb, lch, pc, n_pad)`` -- samples per chunk, strengths per slice, basis planes per post-processing
        launch and the padded row length of a ``pixsrc_reconstruct`` call of these sizes (host only)."""
        out = (c_int32 * 4)()
        _check(lib().gl_pixsrc_layout(self._h, int(B), int(n_strength), int(n_src[0]), int(n_src[1]), int(n_used), out))
        return dict(zip(("cb", "lch", "pc", "n_pad"), (int(v) for v in out)))

    def _pix_tensor(self, t, dtype, shape, what):
        _require_cuda(t, what)
        if t.dtype != dtype or tuple(t.shape) != tuple(shape):
            raise NativeLibraryError(f"pixsrc_reconstruct: {what} must be {dtype} {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
        return t.contiguous()

    def num_linear(self):
        return lib().gl_model_num_linear(self._h)

    def lstsq(self, params, obs, err, parts, want):
        """gl_lstsq_fwd: ``want`` in {"coeffs", "stacked", "image"} -> 1-tuple with that tensor."""
        self._single_plane("lstsq")
        params = self._params(params)
        B, D = params.shape[0], self.num_linear()
        nbytes = lib().gl_lstsq_workspace_bytes(self._h, B)
        ws = self._scratch("lstsq", nbytes)
        dev = params.device
        coeffs = torch.empty((B, D), dtype=torch.float32, device=dev) if want == "coeffs" else None
        stacked = torch.empty((B, D, self.out_h, self.out_w), dtype=torch.float32, device=dev) if want == "stacked" else None
        image = torch.empty((B, self.out_h, self.out_w), dtype=torch.float32, device=dev) if want == "image" else None
        _check(lib().gl_lstsq_fwd(self._h, _ptr(params), _ptr(obs), _ptr(err), B, int(parts), _ptr(coeffs),
                                  _ptr(stacked), _ptr(image), _ptr(ws), ws.numel(), _stream()))
        return ({"coeffs": coeffs, "stacked": stacked, "image": image}[want],)

    def lstsq_solve_flags(self, B):
        """Per-sample flags of the most recent linear solve on ``B`` samples: 0 = solved by the Cholesky attempt, 1 = by the
        eigenvalue solve (a view into the workspace; measurement aid, ``gl_lstsq_solve_flags``)."""
        off = c_size_t()
        _check(lib().gl_lstsq_solve_flags(self._h, B, ctypes.byref(off)))
        return self._lstsq_ws[off.value:off.value + 4 * B].view(torch.int32)

    @property
    def _lstsq_ws(self):
        """The workspace of the most recent ``lstsq`` (measurement aid: the dispatch tests pre-fill it)."""
        return self._scratch_bufs["lstsq"]

    def set_series(self, component, r0, coeffs):
        """Attach the coefficient field of a GL_SERIES lens (gl_model_set_series)."""
        _require_cuda(coeffs, "series coefficients")
        if coeffs.shape[-1] != self.N:
            raise NativeLibraryError(f"series field has {coeffs.shape[-1]} points, the model grid {self.N}")
        with torch.cuda.device(self.device):
            _check(lib().gl_model_set_series(self._h, int(component), float(r0), _ptr(coeffs.contiguous())))
        self._changed(False)

    def set_series_hessian(self, component, coeffs):
        """Attach the Hessian field of a GL_SERIES lens (gl_model_set_series_hessian)."""
        _require_cuda(coeffs, "series Hessian coefficients")
        if coeffs.shape[-1] != self.N or coeffs.shape[0] != 3:
            raise NativeLibraryError(f"series Hessian field is {tuple(coeffs.shape)}, expected (3, order+1, {self.N})")
        with torch.cuda.device(self.device):
            _check(lib().gl_model_set_series_hessian(self._h, int(component), _ptr(coeffs.contiguous())))
        self._changed(False)

    def set_prior(self, columns, const_row):
        """columns: list of (param_col, bijector, prior, a, b, lo, hi, log_norm); const_row: [P] floats."""
        arr = (gl_zcolumn * max(len(columns), 1))(*[gl_zcolumn(*c) for c in columns])
        cr = np.ascontiguousarray(const_row, dtype=np.float32)
        with torch.cuda.device(self.device):
            _check(lib().gl_model_set_prior(self._h, arr, len(columns), cr.ctypes.data_as(POINTER(c_float))))
        self.d_z = len(columns)
        self.prior_owner = None
        self._changed(False)

    def set_positions(self, xs, ys, exs, eys):
        """xs, ys, exs, eys: lists (one entry per image family) of 1-D arrays of equal length."""
        sizes = np.asarray([len(np.atleast_1d(x)) for x in xs], dtype=np.int32)
        cat = lambda L: np.ascontiguousarray(np.concatenate([np.atleast_1d(np.asarray(v, dtype=np.float32)) for v in L]))
        x, y, ex, ey = cat(xs), cat(ys), cat(exs), cat(eys)
        if not (x.size == y.size == ex.size == ey.size == int(sizes.sum())):
            raise NativeLibraryError("centroids / errors of a family must have the same length")
        fp = lambda a: a.ctypes.data_as(POINTER(c_float))
        with torch.cuda.device(self.device):
            _check(lib().gl_model_set_positions(self._h, len(sizes), sizes.ctypes.data_as(POINTER(c_int32)), fp(x), fp(y),
                                                fp(ex), fp(ey)))
        self.n_images = int(sizes.sum())
        self.n_families = int(sizes.size)
        self.positions_owner = None
        self._changed(True)  # the workspace layout follows the number of images

    def positions(self, params, want_grad):
        self._single_plane("positions")
        return self._positions(lib().gl_positions_fwd_bwd, _check, params, want_grad)

    def _positions(self, fn, check, params, want_grad, extra=(), want_extra=False):
        """One point-likelihood entry ``fn`` -> ``(loglike, chi2, grad or None)``.  ``extra``: the width of every further output the
        entry takes between ``grad`` and the workspace; with ``want_extra`` they are allocated ``[B, width]`` and appended to the
        result, without they are null pointers."""
        params = self._params(params)
        B = params.shape[0]
        ws = self._workspace(B)
        ll = torch.empty(B, dtype=torch.float32, device=params.device)
        chi2 = torch.empty_like(ll)
        grad = torch.empty_like(params) if want_grad else None
        more = [torch.empty((B, n), dtype=torch.float32, device=params.device) if want_extra else None for n in extra]
        check(fn(self._h, _ptr(params), B, _ptr(ll), _ptr(chi2), _ptr(grad), *map(_ptr, more), _ptr(ws), ws.numel(), _stream()))
        return (ll, chi2, grad, *more) if want_extra else (ll, chi2, grad)

    def logprob(self, z, obs, err, mask, bg_rms, exp_time, want_grad, chi2_divisor=1.0, terms=1):
        self._single_plane("logprob")
        return self._logprob(lib().gl_logprob_fwd_bwd, _check, z, obs, err, mask, bg_rms, exp_time, want_grad, chi2_divisor, terms)

    def set_timing(self, slots=1, stride=1):
        """Ring of ``slots`` HIP-event pairs around every ``stride``-th main-kernel launch (0 / False: off)."""
        _check(lib().gl_model_set_timing(self._h, int(slots)))
        _check(lib().gl_model_set_timing_stride(self._h, max(int(stride), 1)))
        self._timing_slots = int(slots)
        self._changed(False)

    def timing_drain(self):
        """Durations [ms] of the main launches recorded since the last drain (oldest first)."""
        cap = max(self._timing_slots, 1)
        buf = (c_float * cap)()
        n = c_int()
        _check(lib().gl_model_timing_drain(self._h, buf, cap, ctypes.byref(n)))
        return list(buf[:n.value])

    def last_main_kernel(self):
        """Mangled symbol of the kernel the most recent main launch dispatched."""
        buf = ctypes.create_string_buffer(1024)
        _check(lib().gl_model_last_main_kernel(self._h, buf, len(buf)))
        return buf.value.decode()

    def last_post_kernel(self, transpose=False):
        """Mangled symbol of the kernel that served the most recent forward / transposed PSF + pooling launch."""
        buf = ctypes.create_string_buffer(1024)
        _check(lib().gl_model_last_post_kernel(self._h, int(bool(transpose)), buf, len(buf)))
        return buf.value.decode()

    def post_apply(self, inp, out=None, transpose=False, scale=1.0):
        """gl_post_apply: the model's PSF convolution + pooling (x ``scale``) on a stack ``inp`` of supersampled images
        ``[B, Hs, Ws]``, or its transpose on pooled images ``[B, H, W]``.  ``out``: a contiguous float32 tensor to write into
        (default: a new one)."""
        _require_cuda(inp, "inp")
        shape_in, shape_out = ((self.out_h, self.out_w), (self.ss_h, self.ss_w)) if transpose else ((self.ss_h, self.ss_w), (self.out_h, self.out_w))
        if inp.dtype != torch.float32 or inp.dim() != 3 or tuple(inp.shape[1:]) != shape_in or not inp.is_contiguous():
            raise NativeLibraryError(f"post_apply: inp must be contiguous float32 [B,{shape_in[0]},{shape_in[1]}], got {inp.dtype} {tuple(inp.shape)}")
        B = inp.shape[0]
        if out is None:
            out = torch.empty((B,) + shape_out, dtype=torch.float32, device=inp.device)
        _require_cuda(out, "out")
        if out.dtype != torch.float32 or tuple(out.shape) != (B,) + shape_out or not out.is_contiguous():
            raise NativeLibraryError(f"post_apply: out must be contiguous float32 {(B,) + shape_out}, got {out.dtype} {tuple(out.shape)}")
        _check(lib().gl_post_apply(self._h, B, _ptr(inp), _ptr(out), int(bool(transpose)), float(scale), _stream()))
        return out

    def partial_rows(self, B):
        """The per-(sample, chunk) partial rows ``[B, n_chunks, A]`` the most recent gradient call on ``B`` samples left in the
        workspace (a view; measurement aid, see ``gl_model_launch_shape``)."""
        chunk, nc, row, off = c_int(), c_int(), c_int(), c_size_t()
        _check(lib().gl_model_launch_shape(self._h, B, ctypes.byref(chunk), ctypes.byref(nc), ctypes.byref(row), ctypes.byref(off)))
        ws = self._workspace(B)
        n = B * nc.value * row.value
        return ws[off.value:off.value + 4 * n].view(torch.float32).view(B, nc.value, row.value)

    def workspace_layout(self, B, component=-1):
        """``gl_model_workspace_layout``: byte offsets / element counts of the ``params``, ``derived``, ``order`` and ``cost`` regions of
        the workspace of a call on ``B`` samples, the row lengths ``P`` / ``D`` and ``component``'s ``p_off`` / ``d_off`` (host only)."""
        out = gl_workspace_layout()
        _check(lib().gl_model_workspace_layout(self._h, int(B), int(component), ctypes.byref(out)))
        return out

    def workspace_rows(self, B):
        """Views into the workspace of the most recent call on ``B`` samples (measurement aid): ``params [B, P]`` and ``derived
        [B, D]`` float32, ``order [B]`` and ``cost [B]`` int32."""
        lay, ws = self.workspace_layout(B), self._workspace(B)
        view = lambda off, n, dt: ws[off:off + 4 * n].view(dt)
        return {"params": view(lay.params_offset, lay.params_count, torch.float32).view(B, lay.P),
                "derived": view(lay.derived_offset, lay.derived_count, torch.float32).view(B, lay.D),
                "order": view(lay.order_offset, lay.order_count, torch.int32),
                "cost": view(lay.cost_offset, lay.cost_count, torch.int32)}

    def last_main_ms(self):
        ms = c_float()
        _check(lib().gl_model_last_main_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def _workspace(self, B):
        ws = self._ws.get(B)
        if ws is None:
            nbytes = lib().gl_workspace_bytes(self._h, B)
            ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
            self._ws = {B: ws}  # keep only the latest batch size
        return ws

    def _params(self, params):
        _require_cuda(params, "params")
        if params.dtype != torch.float32 or params.dim() != 2 or params.shape[1] != self.P:
            raise NativeLibraryError(f"params must be float32 [B,{self.P}], got {params.dtype} {tuple(params.shape)}")
        return params.contiguous()

    def simulate_fwd(self, params):
        self._single_plane("simulate_fwd")
        params = self._params(params)
        B = params.shape[0]
        ws = self._workspace(B)
        img = torch.empty((B, self.out_h, self.out_w), dtype=torch.float32, device=params.device)
        _check(lib().gl_simulate_fwd(self._h, _ptr(params), B, _ptr(img), _ptr(ws), ws.numel(), _stream()))
        return img

    def simulate_parts(self, params, parts):
        self._single_plane("simulate_parts")
        return self._render(lib().gl_simulate_parts_fwd, _check, params, parts)

    def simulate_bwd(self, params, grad_img):
        self._single_plane("simulate_bwd")
        return self._render_bwd(lib().gl_simulate_bwd, _check, params, grad_img)

    def loglike(self, params, obs, err, mask, bg_rms, exp_time, want_grad):
        self._single_plane("loglike")
        return self._loglike(lib().gl_loglike_fwd_bwd, _check, params, obs, err, mask, bg_rms, exp_time, bool(want_grad))

    # behind the single-plane methods and their multiplane_* twins: `fn` the family's entry, `check` how it raises error codes
    def _render(self, fn, check, params, parts):
        params = self._params(params)
        B = params.shape[0]
        ws = self._workspace(B)
        img = torch.empty((B, self.out_h, self.out_w), dtype=torch.float32, device=params.device)
        check(fn(self._h, _ptr(params), B, int(parts), _ptr(img), _ptr(ws), ws.numel(), _stream()))
        return img

    def _render_bwd(self, fn, check, params, grad_img):
        params = self._params(params)
        B = params.shape[0]
        ws = self._workspace(B)
        grad_img = grad_img.to(device=params.device, dtype=torch.float32).expand(B, self.out_h, self.out_w).contiguous()
        grad = torch.empty_like(params)
        check(fn(self._h, _ptr(params), _ptr(grad_img), B, _ptr(grad), _ptr(ws), ws.numel(), _stream()))
        return grad

    def _loglike(self, fn, check, params, obs, err, mask, bg_rms, exp_time, want_grad):
        """``(loglike, chi2, gradient or None)``; ``want_grad`` None: ``fn`` is a forward-only entry without a gradient argument."""
        params = self._params(params)
        B = params.shape[0]
        ws = self._workspace(B)
        ll = torch.empty(B, dtype=torch.float32, device=params.device)
        chi2 = torch.empty_like(ll)
        grad = torch.empty_like(params) if want_grad else None
        grad_arg = () if want_grad is None else (_ptr(grad),)
        check(fn(self._h, _ptr(params), _ptr(obs), _ptr(err), _ptr(mask), float(bg_rms), float(exp_time), B, _ptr(ll), _ptr(chi2),
                 *grad_arg, _ptr(ws), ws.numel(), _stream()))
        return ll, chi2, grad

    def _logprob(self, fn, check, z, obs, err, mask, bg_rms, exp_time, want_grad, chi2_divisor, terms):
        _require_cuda(z, "z")
        if z.dtype != torch.float32 or z.dim() != 2 or z.shape[1] != self.d_z:
            raise NativeLibraryError(f"z must be float32 [B,{self.d_z}], got {z.dtype} {tuple(z.shape)}")
        z = z.contiguous()
        B = z.shape[0]
        ws = self._workspace(B)
        lp = torch.empty(B, dtype=torch.float32, device=z.device)
        ll = torch.empty_like(lp)
        chi2 = torch.empty_like(lp)
        grad = torch.empty_like(z) if want_grad else None
        check(fn(self._h, _ptr(z), _ptr(obs), _ptr(err), _ptr(mask), float(bg_rms), float(exp_time), B, _ptr(lp), _ptr(ll),
                 _ptr(chi2), _ptr(grad), float(chi2_divisor), int(terms), _ptr(ws), ws.numel(), _stream()))
        return lp, ll, chi2, grad
