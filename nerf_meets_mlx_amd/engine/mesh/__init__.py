"""Mesh extraction from a trained field, and what is done with the mesh (include/nerf_hip.h "mesh extraction" and the sections
behind it, DESIGN.md section 14 onwards; the map of this package is DESIGN.md section 36).  The reference has no such export; this
is Instant-NGP's.  One module per stage, and every name of theirs is a name of this package:

  _checks (the three argument tests) <- _base (Mesh, the lattice arguments, the stage hook) <- surface (simplify, smooth) <- volume
  (density volume, marching cubes, components, opening, extract / mesh_volume); _base <- tsdf (TSDFVolume, tsdf_views); _base <-
  texture (atlas bake and lookup, mip pyramid) <- raster (rasterize, face_lod, render_mesh, render_mesh_mip) <- project
  (project_texture); _base <- decimate (decimate: edge collapse to a target face count); texture <- files (PLY, OBJ, PNG); _base <- distance (sample_surface, MeshIndex, mesh_distance).
  distance also holds the second index, MeshBVH (a bounding-volume hierarchy with the grid's answers bit for bit), and
  closest_points.  distance <- volume <- winding (MeshWinding, winding_number, winding_volume, remesh, signed_distance): the
  generalized winding number on MeshBVH's tree, the inside test the distance lacks.  distance, raster <- raycast (MeshRaycast,
  pack_rays, raycast_frame, render_mesh_rays): nearest hit and occlusion of rays on the same tree, and the rasteriser's frame by
  rays."""
from ._base import CHUNK, MAX_RES, MESH_MAX_ITEMS, Mesh, _box, _check_mesh_tensors, _mark, check_mesh_args
from .decimate import (DECIMATE_MAX_PASSES, DECIMATE_MAX_ROUNDS, DECIMATE_PLACEMENTS, DECIMATE_STOPS, DecimateStats, _decimate,
                       check_decimate_args, decimate)
from .distance import (DISTANCE_INDEXES, DISTANCE_MAX_ENTRIES, DISTANCE_MAX_GRID, DISTANCE_MAX_SAMPLES, DistanceStats, MeshBVH,
                       MeshDistance, MeshIndex, check_distance_args, check_distance_index, closest_points, default_distance_grid,
                       mesh_distance, point_mesh_distance, sample_surface)
from .files import _PNG_MAGIC, _png_chunk, _replace_file, png_array, png_bytes, read_obj, read_ply, write_obj, write_ply
from .project import PROJECT_COS_MIN, PROJECT_DEPTH_TOL_CELLS, PROJECT_MAX_VIEWS, PROJECT_MODES, check_project_args, project_texture
from .raster import (RASTER_MAX_SIDE, RASTER_NEAR, RASTER_SMALL_MAX, MeshFrame, _raster_background, _raster_view, check_lod_scale,
                     check_raster_args, face_lod, rasterize, render_mesh, render_mesh_mip)
from .raycast import (RAY_STRIDE, RAYCAST_SLACK, RAYCAST_SORTED_QUERY, MeshRaycast, RayHits, check_raycast_args, pack_rays,
                      raycast_frame, render_mesh_rays)
from .surface import (PLACEMENTS, SIMPLIFY_MAX_CLUSTERS, SMOOTH_MAX_ITERATIONS, _simplify, _smooth, check_simplify_args,
                      check_simplify_grid, check_smooth_args, check_smooth_params, check_surface_options, simplify, smooth)
from .texture import (MIP_MAX_LEVELS, TEXTURE_MAX_SIDE, TEXTURE_MAX_TEXELS, Texture, TexturePyramid, _check_pyramid, _check_texture,
                      bake_texture, build_mipmaps, check_texture_args, mip_levels, sample_texture, sample_texture_mip, texture_layout)
from .tsdf import TSDF_MAX_VIEWS, TSDFVolume, _k_of, check_tsdf_args, tsdf_views
from .volume import (EXP, MAX_OPENING_RADIUS, RELU, Components, _check_radius, _check_volume, _marching_cubes, _open_components,
                     _rows_into, check_component_args, check_opening_args, check_volume_options, connected_components, density_volume,
                     erode, extract, filter_components, filter_volume, lattice_rows, marching_cubes, mesh_volume, open_components,
                     reconstruct, vertex_colors)
from .winding import (WINDING_INSIDE, WINDING_NODE_DOUBLES, MeshWinding, check_winding_args, remesh, signed_distance, winding_number,
                      winding_volume)
