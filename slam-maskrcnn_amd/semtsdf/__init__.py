"""semtsdf — MI355X-native semantic TSDF fusion (integrate + association + raycast).

Python host over the C ABI of libsemtsdf.so (include/semtsdf.h).  The compute runs in
hand-written HIP kernels for gfx950; this package only marshals arguments and mirrors the
reference's host interfaces (src/TSDF_Python/tsdf.py, src/SfM_CUDA/tsdf.cuh,
configuration.h, tsdf_cuda.tsdf_update).
"""
from . import _lib
from ._lib import PLACE_PYTHON, PLACE_SFM, RAY_ASSOC, RENDER_COLOR, RENDER_LABEL, SemTSDFError, load
from .config import Configuration, FusionConfig
from .export import (export_surface, extract_mesh, merge_meshes, read_mesh_ply, read_ply, write_mesh_ply,
                     write_ply)
from .instances import find_duplicates, instance_stats, merge_instance_stats, plan_remap
from . import bricks, follow, maps, track
from .bricks import BrickStore, shift_paged
from .follow import evicted_points, plan_shift
from .maps import pose_camera, shade_normals, z_depth
from .track import TrackingLost
from .tsdf import TSDF
from .volume import DeviceBuffer, Volume, default_params, orbit_camera, place_from_frame

__all__ = ["TSDF", "Volume", "DeviceBuffer", "Configuration", "FusionConfig", "SemTSDFError", "load",
           "default_params", "place_from_frame", "orbit_camera", "_lib", "export_surface", "write_ply", "read_ply",
           "extract_mesh", "merge_meshes", "write_mesh_ply", "read_mesh_ply",
           "instance_stats", "merge_instance_stats", "find_duplicates", "plan_remap",
           "maps", "pose_camera", "z_depth", "shade_normals", "track", "TrackingLost",
           "follow", "plan_shift", "evicted_points", "bricks", "BrickStore", "shift_paged",
           "RENDER_LABEL", "RENDER_COLOR", "RAY_ASSOC", "PLACE_SFM", "PLACE_PYTHON"]
