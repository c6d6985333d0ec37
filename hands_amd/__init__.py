"""hands_amd -- MI355X-native forward path of the WildHands hand-mesh regressor.

Host side mirrors the reference's module API (``HandsLight``, ``xdict``); compute is
``libhands_hip.so`` (hand-written gfx950 HIP, see include/hands_hip.h).
"""
from .xdict import xdict, prefix_dict  # noqa: F401
from .hands_light import HandsLight, DEFAULT_ARGS, ManoHeadsPlan  # noqa: F401
from .hamer import HAMER, HAMER_DEFAULT_ARGS  # noqa: F401
from .handoccnet import HandOccNet, HANDOCC_DEFAULT_ARGS  # noqa: F401
from .mano import ManoAsset, synthetic_mano_asset, build_mano_asset  # noqa: F401
from .weights import apply_recipe, synthetic_inputs  # noqa: F401
from .frontend import HandsFrontEnd  # noqa: F401
from .graph import GraphedForward  # noqa: F401
from .wrapper import HandsWrapper, HaMeRWrapper, HandOccNetWrapper  # noqa: F401
from .render import MANORenderer, rasterize  # noqa: F401
from .rend_utils import Renderer, denormalize_images, sideview_transform  # noqa: F401
from .losses import compute_loss_light, mul_loss_dict, total_loss, epoch_end  # noqa: F401
from .metrics import evaluate_metrics, evaluate_mesh_metrics, evaluate_surface_metrics  # noqa: F401
from .metrics import evaluate_penetration_metrics  # noqa: F401
from .surface import closest_on_mesh, interhand_field  # noqa: F401
from .penetration import (seal_mesh, apply_seal, signed_distance_to_mesh, interhand_penetration, penetration_grid,  # noqa: F401
                          intersection_volume)
from .temporal import accel_error, evaluate_accel_metrics, AccelMetrics  # noqa: F401
from .smoothing import SmoothConfig, smooth_mano_params, smooth_predictions, TemporalSmoother  # noqa: F401
from .fitting import (FitConfig, fit_mano, fit_mano_hands, fit_targets, Fit2DConfig, fit_mano_2d, fit_mano_hands_2d,  # noqa: F401
                      fit_targets_2d, refine_predictions, fit_mano_verts, fit_mano_hands_verts, fit_targets_verts,
                      SurfaceFitConfig, fit_mano_surface, fit_mano_hands_surface, correspond_on_mesh, RegisterConfig,
                      register_mano, register_mano_hands, register_predictions)

__all__ = ["HandsLight", "DEFAULT_ARGS", "ManoHeadsPlan", "HAMER", "HAMER_DEFAULT_ARGS", "HandOccNet", "HANDOCC_DEFAULT_ARGS", "xdict", "prefix_dict", "ManoAsset", "synthetic_mano_asset",
           "build_mano_asset", "apply_recipe", "synthetic_inputs", "HandsFrontEnd", "GraphedForward", "HandsWrapper",
           "HaMeRWrapper", "HandOccNetWrapper", "MANORenderer", "rasterize", "Renderer", "denormalize_images", "sideview_transform",
           "compute_loss_light", "mul_loss_dict", "total_loss", "epoch_end", "evaluate_metrics", "evaluate_mesh_metrics",
           "evaluate_surface_metrics", "closest_on_mesh", "interhand_field", "evaluate_penetration_metrics", "seal_mesh", "apply_seal",
           "signed_distance_to_mesh", "interhand_penetration", "penetration_grid", "intersection_volume",
           "accel_error", "evaluate_accel_metrics", "AccelMetrics",
           "SmoothConfig", "smooth_mano_params", "smooth_predictions", "TemporalSmoother",
           "FitConfig", "fit_mano", "fit_mano_hands", "fit_targets",
           "Fit2DConfig", "fit_mano_2d", "fit_mano_hands_2d", "fit_targets_2d", "refine_predictions",
           "fit_mano_verts", "fit_mano_hands_verts", "fit_targets_verts", "SurfaceFitConfig", "fit_mano_surface",
           "fit_mano_hands_surface", "correspond_on_mesh", "RegisterConfig", "register_mano", "register_mano_hands",
           "register_predictions"]
