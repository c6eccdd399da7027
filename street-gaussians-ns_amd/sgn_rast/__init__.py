"""sgn_rast — MI355X-native differentiable Gaussian rasterizer (host side).

Only what the hot path needs: the ctypes binding of libsgnrast.so (``_lib``), the gsplat-compatible operator
surface (``ops``), the fused front ends (``fused``: activations / rigid transform / Fourier DC / sigmoid folded into
the kernels), the callers either side of the path that SURVEY.md §8f ranks next (``sky``: nvdiffrast cube-map lookup,
``loss``: L1 + SSIM, ``optim``: multi-tensor Adam, ``densify``: per-step statistics, ``knn``: k-nearest neighbours for the initial
scales, ``geometry``: nearest neighbours across two clouds and the LiDAR chamfer metric, ``seed``: the seed clouds from LiDAR
sweeps and the initial parameters), the data-parallel helpers
(``dp``), the ground-truth feed of the training loop (``feed``: the data set as pinned bytes, prefetched a step ahead), the
coarse-to-fine resolution schedule on those bytes (``pyramid``: one level of a batch's ground truth in one launch),
the outbound mirror of the feed (``frames``: a frame's eval outputs packed into writer bytes in one launch, carried to
pinned memory behind the next render), the feature channels composited over the RGB pass's depth list (``features``:
K per-Gaussian values in one walk per 16 channels with gradients, the differentiable expected depth, the semantic
cross-entropy), LiDAR depth supervision (``lidar``: sweeps splatted to a per-pixel target, the fused depth loss on the
expected depth, the evaluation depth metrics), per-image colour correction (``appearance``: bilateral grids of 3x4 affines
sliced by one fused kernel pair, the per-image affine as the 1 x 1 x 1 grid, the total-variation prior), the call-site replay used by bench/smoke/tests (``step``) and the deterministic synthetic scenes
(``scenes``).  Sub-modules are imported on demand; none of them has a CPU fallback.
"""
from .appearance import BilateralGrids, slice_image, total_variation  # noqa: F401
from .features import (  # noqa: F401
    expected_depth,
    rasterize_features,
    semantic_argmax,
    semantic_cross_entropy,
)
from .feed import Batch, ImageFeed  # noqa: F401
from .frames import FrameSink, Panel, byte_lut, colormap, pack  # noqa: F401
from .lidar import depth_loss, depth_metrics, splat_depth  # noqa: F401
from .ops import (  # noqa: F401
    bin_and_sort_gaussians,
    compute_cumulative_intersects,
    get_tile_bin_edges,
    map_gaussian_to_intersects,
    num_sh_bases,
    project_gaussians,
    quat_to_rotmat,
    rasterize_gaussians,
    set_alpha_clamp_bwd,
    spherical_harmonics,
)
from .pyramid import Level, downscale, downscale_factor, level_size, scaled_camera  # noqa: F401

__version__ = "0.1.0"
