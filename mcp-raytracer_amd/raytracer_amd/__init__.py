"""raytracer_amd - MI355X-native path-tracing core for df07/mcp-raytracer.

The hot path (camera rays, BVH traversal, sphere/quad/plane hits, material
scatter with mixture-PDF light sampling, spp accumulation) runs as HIP
kernels for gfx950 in librt_amd.so, behind the C ABI in include/rt_amd.h.
This package is the host-side mirror of the reference's TypeScript surface:

    generate_scene_data / create_camera_from_scene_data / generate_scene  (src/scenes/scenes.ts)
    Camera.render_region / Camera.render -> RenderStats                  (src/camera.ts)
    generate_image_buffer                                                (src/raytracer.ts)

plus progressive rendering, which the reference lacks: Camera.progressive / Camera.resume ->
ProgressiveRender (resumable sample steps with a preview and checkpoints), and first-hit
guide buffers with a guided edge-avoiding a-trous filter for low-sample frames:
Camera.render_guides / Camera.denoise / denoise / ProgressiveRender.denoised; a session's
per-pixel variance map (ProgressiveRender.variance, progressive_blob_variance) guides that filter
when `variance=` is passed to any of them, and `guides="specular"` /
render_guides(through_specular=True) take the guides behind mirrors and glass. A previous view's frame is reprojected into a moved
camera's view by Camera.reproject / reproject / ProgressiveRender.reprojected (Camera.view,
Camera.reusable_objects), so the first frames of a new view start from the last view's history;
with `guides="specular"` (reproject_specular, Camera.through_objects) what a mirror or glass shows
finds its history too. A History follows a camera
along a path on the device: ProgressiveRender.accumulated blends each view's frame onto it by
per-pixel history lengths and carries a variance the variance-guided filter consumes
(temporal_accumulate: the same with explicit buffers); with `guides="specular"`
(temporal_accumulate_specular, History.chain_guides) the history follows mirrors and glass to the
surface they show. Vary `seed` per view.
"""
from ._lib import RtError, build_id, device_count, progressive_blob_info, progressive_blob_variance
from .camera import Camera, History, ProgressiveRender, RenderStats, rng_stream
from .passes import denoise, reproject, reproject_specular, temporal_accumulate, temporal_accumulate_specular
from .raytracer import divide_into_regions, divideIntoRegions, generate_image_buffer, generateImageBuffer
from .scenes import (create_camera_from_scene_data, createCameraFromSceneData, generate_scene,
                     generate_scene_data, generateScene, generateSceneData)

__all__ = [
    "Camera", "ProgressiveRender", "RenderStats", "RtError", "build_id", "device_count", "rng_stream",
    "progressive_blob_info", "progressive_blob_variance", "denoise", "reproject", "reproject_specular", "History",
    "temporal_accumulate", "temporal_accumulate_specular",
    "generate_scene_data", "create_camera_from_scene_data", "generate_scene",
    "generate_image_buffer", "divide_into_regions",
    "generateSceneData", "createCameraFromSceneData", "generateScene", "generateImageBuffer",
    "divideIntoRegions",
]
