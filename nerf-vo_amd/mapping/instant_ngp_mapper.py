"""Drop-in counterpart of the reference's second mapping method ``InstantNGP``
(/root/reference/nerf_vo/mapping/instant_ngp.py:19-117) and of ``InstantNGPRenderer`` /
``NeRFSLAMNGPRenderer`` (/root/reference/evaluation/nerf_renderer.py:221-344).  Both drive the testbed facade
``nerf_vo_amd.pyngp`` through exactly the calls the reference makes on NVlabs' ``pyngp`` -- the facade, not these
classes, is the drop-in boundary: the reference's own two files run against it unchanged.

Same constructor, attributes (``is_initialized``, ``is_shut_down``, ``step``, ``ngp``) and methods
(``__call__``, ``update``, ``train``, ``shut_down``, ``save_snapshot``); same ingest transformations
(NCHW -> NHWC, sRGB -> linear colours + unit alpha at :64-74, unit depth covariance, intrinsics of the first
frame of the packet, poses taken as camera-to-world 3x4 in the NeRF / OpenGL convention the enhancement stage
emits, nerf_scale 1 / nerf_offset 0, aabb_scale 4, extrinsics optimisation on, L2 depth loss).  One difference:
keyframe data is handed to the facade as device tensors (the reference round-trips every packet through host
numpy lists, :87-100; the facade accepts both)."""
from __future__ import annotations

import argparse
import math
import os

import numpy as np
import torch

from .. import pyngp
from .nerfstudio_mapper import step_check
from .renderer import NeRFRenderer

file_instant_ngp_config = "nerf_vo/thirdparty/nerf_slam/thirdparty/instant-ngp/configs/nerf/base.json"


class InstantNGP:
    def __init__(self, args: argparse.Namespace, device: torch.device = torch.device("cuda:0")) -> None:
        self.args = args
        self.device = torch.device(device)
        self.is_initialized = False
        self.is_shut_down = False
        self.step = 0

        self.ngp = pyngp.Testbed(pyngp.TestbedMode.Nerf, self.device.index or 0)
        bounding_box = pyngp.BoundingBox(np.array([-np.inf, -np.inf, -np.inf]), np.array([np.inf, np.inf, np.inf]))
        self.ngp.create_empty_nerf_dataset(n_images=args.num_keyframes, nerf_scale=1.0,
                                           nerf_offset=np.array([0.0, 0.0, 0.0]), aabb_scale=4,
                                           render_aabb=bounding_box)
        self.ngp.nerf.training.n_images_for_training = 0
        self.ngp.reload_network_from_file(file_instant_ngp_config)
        self.ngp.shall_train = True
        self.ngp.nerf.training.optimize_extrinsics = True
        self.ngp.nerf.training.depth_loss_type = pyngp.LossType.L2
        self.ngp.frame()

    def __call__(self, input: dict | None) -> None:
        if self.step == self.args.mapping_iterations:
            self.shut_down()
        else:
            if input is not None:
                self.update(input=input)
            if self.is_initialized:
                self.train()

    def update(self, input: dict) -> None:
        color = input["frames_color"].to(self.device).permute(0, 2, 3, 1)
        # sRGB -> linear, exactly as the reference does before handing images to the testbed
        color = torch.where(color > 0.04045, torch.pow((color + 0.055) / 1.055, 2.4), color / 12.92)
        color = torch.cat((color, torch.ones_like(color[..., :1])), dim=3)
        depth = input["frames_depth"].to(self.device).permute(0, 2, 3, 1)
        if "frames_depth_covariance" in input:
            depth_cov = input["frames_depth_covariance"].to(self.device).permute(0, 2, 3, 1)
        else:
            depth_cov = torch.ones_like(depth)
        self.ngp.nerf.training.update_training_images(
            frame_ids=input["keyframe_indices"].contiguous().cpu().numpy().tolist(),
            poses=input["camera_extrinsics"].to(self.device)[:, :3].contiguous(),
            images=color.contiguous(), depths=depth.contiguous(), depths_cov=depth_cov.contiguous(),
            resolution=np.array([self.args.frame_width, self.args.frame_height]),
            principal_point=input["camera_intrinsics"][0, 2:].cpu().numpy(),
            focal_length=input["camera_intrinsics"][0, :2].cpu().numpy(),
            depth_scale=1.0, depth_cov_scale=1.0)
        self.is_initialized = True  # (no torch.cuda.empty_cache(): allocator churn)

    def train(self) -> None:
        self.ngp.frame()
        if step_check(self.step, self.args.mapping_snapshot_iterations):
            self.save_snapshot()
        self.step += 1

    def shut_down(self) -> None:
        self.save_snapshot()
        self.is_shut_down = True

    def save_snapshot(self) -> None:
        self.ngp.save_snapshot(self.args.dir_prediction + f"/snapshots/snapshot{self.step:06d}.msgpack", False)


class InstantNGPRenderer(NeRFRenderer):
    """render_frame(intrinsics, extrinsics) -> (uint8 sRGB colour, z-depth): linear render -> un-premultiply ->
    sRGB transfer -> clip -> *255 + 0.5, through the same testbed calls as the reference."""

    def load_nerf_from_snapshot(self, dir_prediction: str) -> None:
        dir_snapshots = dir_prediction + "/snapshots"
        files = sorted(f for f in os.listdir(dir_snapshots) if ".msgpack" in f) if os.path.exists(dir_snapshots) else []
        if not files:
            raise FileNotFoundError(f"Could not find snapshot in {dir_snapshots}")
        self.load_ngp_from_snapshot(file_snapshot=os.path.join(dir_snapshots, files[-1]))

    def load_ngp_from_snapshot(self, file_snapshot: str) -> None:
        self.ngp = pyngp.Testbed(pyngp.TestbedMode.Nerf, 0)
        self.ngp.load_snapshot(path=file_snapshot)

    def load_nerf_from_mapping_model(self, mapping_model) -> None:
        self.ngp = mapping_model.ngp

    def get_camera_extrinsics(self, frame_index: int) -> np.ndarray:
        m = np.eye(4)
        m[:3] = self.ngp.nerf.training.get_camera_extrinsics(frame_idx=frame_index)
        m = m[[1, 2, 0, 3]]   # NGP row order -> NeRF
        m[0:3, 1:3] *= -1     # NeRF (y up, -z forward) -> standard (y down, z forward)
        return m

    def render_frame(self, camera_intrinsics: dict, camera_extrinsics: np.ndarray) -> tuple:
        color = self.render_frame_color(camera_intrinsics=camera_intrinsics, camera_extrinsics=camera_extrinsics.copy())
        depth = self.render_frame_depth(camera_intrinsics=camera_intrinsics, camera_extrinsics=camera_extrinsics.copy())
        return color, depth

    def render_frame_color(self, camera_intrinsics: dict, camera_extrinsics: np.ndarray) -> np.ndarray:
        self._set_rendering_defaults(camera_intrinsics)
        self._set_camera_extrinsics(camera_extrinsics)
        self.ngp.render_mode = pyngp.Shade
        color = self.ngp.render(width=camera_intrinsics["width"], height=camera_intrinsics["height"], spp=1, linear=True)
        color[..., 0:3] = np.divide(color[..., 0:3], color[..., 3:4], out=np.zeros_like(color[..., 0:3]),
                                    where=color[..., 3:4] != 0)
        lin = color[..., 0:3]
        srgb = np.where(lin > 0.0031308, 1.055 * (np.maximum(lin, 1e-12) ** (1.0 / 2.4)) - 0.055, 12.92 * lin)
        return (np.clip(srgb, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)

    def render_frame_depth(self, camera_intrinsics: dict, camera_extrinsics: np.ndarray) -> np.ndarray:
        self._set_rendering_defaults(camera_intrinsics)
        self._set_camera_extrinsics(camera_extrinsics)
        self.ngp.render_mode = pyngp.Depth
        return self.ngp.render(width=camera_intrinsics["width"], height=camera_intrinsics["height"], spp=1,
                               linear=True)[..., 0]

    def render_mesh(self, file_mesh: str, resolution, lower_bound, upper_bound, vertex_attributes: bool = False) -> None:
        """ref: evaluation/nerf_renderer.py:296-300.  ``vertex_attributes``: the file also carries vertex normals and
        colours (pyngp.Testbed.compute_and_save_marching_cubes_mesh)."""
        from .. import pyngp

        bounding_box = pyngp.BoundingBox(lower_bound, upper_bound)
        if vertex_attributes:
            self.ngp.compute_and_save_marching_cubes_mesh(file_mesh, resolution, bounding_box, vertex_attributes=True)
        else:
            self.ngp.compute_and_save_marching_cubes_mesh(file_mesh, resolution, bounding_box)

    def render_frame_normal(self, camera_intrinsics: dict, camera_extrinsics: np.ndarray) -> np.ndarray:
        """float32 [H, W, 3]: the rendered unit density-gradient normal of every pixel in world axes (``camera_extrinsics``
        in the standard convention of ``render_frame``), zero where the accumulation is 0.  From the testbed's Normals
        mode: un-premultiplied, ``2 x - 1``, re-normalised.  Parity with upstream's picture of that mode is unpinned."""
        self._set_rendering_defaults(camera_intrinsics)
        self._set_camera_extrinsics(camera_extrinsics)
        self.ngp.render_mode = pyngp.Normals
        out = self.ngp.render(width=camera_intrinsics["width"], height=camera_intrinsics["height"], spp=1, linear=True)
        acc = out[..., 3:4]
        hit = acc > 0
        n = 2.0 * np.divide(out[..., 0:3], acc, out=np.full_like(out[..., 0:3], 0.5), where=hit) - 1.0
        n = n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-20)
        return np.where(hit, n, 0.0).astype(np.float32)

    @torch.no_grad()
    def _generate_point_cloud(self, lower_bound, upper_bound, num_points: int, min_accumulation, seed: int) -> dict:
        """``renderer.generate_point_cloud``'s rule over the occupancy-grid engine: random pixels
        ``floor(rand(R, 3) * [n_active, H, W])`` of the active training frames from a generator of its own seeded with
        ``seed``, through the testbed's training poses with the learnt corrections (``get_camera_extrinsics``); every batch
        goes through ``NgpEngine.render_rays(normals=True)``.  ``point = origin + direction * depth`` per component in
        float32 (unit directions, depth = the distance along them), mapped from the engine's frame to the dataset's;
        colour by ``render_frame_color``'s rule (un-premultiply, sRGB transfer, clip, ``* 255 + 0.5``); ``normal = 2 n - 1``
        re-normalised.  A point is kept when ``accumulation > min_accumulation`` and ``lower < point < upper`` strictly on
        every axis; batches are appended in order until ``num_points`` are kept, the last one cut to fit, with the
        nerfstudio path's give-up rules."""
        from .cameras import Cameras, CameraType
        from .renderer import POINT_CLOUD_EMPTY_BATCHES, POINT_CLOUD_MIN_SHARE

        num_points = int(num_points)
        if num_points < 1:
            raise ValueError("render_point_cloud: num_points must be positive")
        tb = self.ngp
        eng = tb._engine
        if eng is None:
            raise RuntimeError("render_point_cloud: no network has been trained or loaded")
        dev = tb.device
        n_active = int(tb.nerf.training.n_images_for_training)
        if n_active < 1:
            raise ValueError("render_point_cloud: no active training frames")
        poses = np.stack([self.get_camera_extrinsics(i) for i in range(n_active)])[:, :3, :4].copy()
        poses[:, 0:3, 1:3] *= -1  # standard -> NeRF / OpenGL, the engine's camera convention (translation in its frame)
        H, W = tb._resolution
        intr = tb._intrinsics[:n_active]
        cameras = Cameras(camera_to_worlds=torch.tensor(poses, dtype=torch.float32, device=dev), fx=intr[:, 0].contiguous(),
                          fy=intr[:, 1].contiguous(), cx=intr[:, 2].contiguous(), cy=intr[:, 3].contiguous(), width=W, height=H, camera_type=CameraType.PERSPECTIVE)
        rays_per_batch = min(pyngp._MAX_BUNDLE_RAYS, max(4096, 1 << (num_points - 1).bit_length()))
        scale_n, off_n = float(tb._nerf_scale), torch.as_tensor(np.asarray(tb._nerf_offset), dtype=torch.float32, device=dev)
        lower = torch.as_tensor(np.asarray(lower_bound, dtype=np.float64).reshape(3)).to(dev, torch.float32)
        upper = torch.as_tensor(np.asarray(upper_bound, dtype=np.float64).reshape(3)).to(dev, torch.float32)
        generator = torch.Generator(device=dev)
        generator.manual_seed(int(seed))
        scale = torch.tensor([n_active, H, W], device=dev)
        parts = {"points": [], "normals": [], "view_directions": [], "colors": []}
        kept_total, rays_total, empty = 0, 0, 0
        while kept_total < num_points:
            pixels = torch.floor(torch.rand((rays_per_batch, 3), device=dev, generator=generator) * scale).long()
            bundle = cameras.generate_rays(camera_indices=pixels)
            origins, directions = bundle.origins.reshape(-1, 3).contiguous(), bundle.directions.reshape(-1, 3).contiguous()
            out = eng.render_rays(origins, directions, bundle.metadata["directions_norm"].reshape(-1).contiguous(), 1e-4, True)
            points = ((origins + directions * out["depth"]) - off_n) / scale_n
            keep = ((points > lower) & (points < upper)).all(dim=1)
            if min_accumulation is not None:
                keep &= out["accumulation"][:, 0] > float(min_accumulation)
            index = keep.nonzero().flatten()[:num_points - kept_total]
            rays_total += rays_per_batch
            if index.numel() == 0:
                empty += 1
                if empty >= POINT_CLOUD_EMPTY_BATCHES:
                    raise RuntimeError(
                        f"render_point_cloud: {empty} consecutive batches of {rays_per_batch} rays left no point inside the box "
                        f"{lower.tolist()} .. {upper.tolist()}; {kept_total} of {rays_total} rays were kept so far -- the field "
                        "is empty there (train longer), or the box is not in the dataset's frame")
                continue
            empty = 0
            if rays_total >= POINT_CLOUD_EMPTY_BATCHES * rays_per_batch and (kept_total + int(index.numel())) * POINT_CLOUD_MIN_SHARE < rays_total:
                raise RuntimeError(
                    f"render_point_cloud: only {kept_total + int(index.numel())} of {rays_total} rays gave a point inside the box "
                    f"{lower.tolist()} .. {upper.tolist()} (fewer than 1 in {POINT_CLOUD_MIN_SHARE}): check the box, or ask for "
                    "fewer points")
            normal = 2.0 * out["normals"][index] - 1.0
            acc = out["accumulation"][index]
            lin = torch.where(acc != 0, out["rgb"][index] / acc, torch.zeros_like(acc))
            srgb = torch.where(lin > 0.0031308, 1.055 * lin.clamp_min(1e-12) ** (1.0 / 2.4) - 0.055, 12.92 * lin)
            parts["points"].append(points[index])
            parts["normals"].append(normal / torch.linalg.norm(normal, dim=1, keepdim=True).clamp_min(1e-20))
            parts["view_directions"].append(directions[index])
            parts["colors"].append((srgb.clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8))
            kept_total += int(index.numel())
        return {k: torch.cat(v) for k, v in parts.items()}

    def render_point_cloud(self, file_point_cloud: str, lower_bound, upper_bound, num_points: int = 33554432,
                           remove_outliers: bool = True, std_ratio: float = 10.0, min_accumulation: float | None = 0.5,
                           seed: int = 0) -> dict:
        """``NerfstudioRenderer.render_point_cloud`` for this back-end -- same contract, file layout (binary .ply with
        ``x y z nx ny nz red green blue`` and no faces) and return value: the cloud of ``_generate_point_cloud`` with the
        field's rendered density-gradient normals, cleaned by ``remove_statistical_outlier(nb_neighbors=20, std_ratio)``,
        normals turned towards the cameras (``orient_normals_towards_cameras``)."""
        from ..meshing import write_mesh
        from ..pointcloud import remove_statistical_outlier
        from .renderer import orient_normals_towards_cameras

        cloud = self._generate_point_cloud(lower_bound, upper_bound, num_points, min_accumulation, seed)
        points, normals, colors, views = cloud["points"], cloud["normals"], cloud["colors"], cloud["view_directions"]
        generated = int(points.shape[0])
        if remove_outliers:
            points, index = remove_statistical_outlier(points, nb_neighbors=20, std_ratio=std_ratio)
            normals, colors, views = normals[index], colors[index], views[index]
        normals = orient_normals_towards_cameras(normals, views)
        out = {"points": points.cpu(), "normals": normals.cpu(), "colors": colors.cpu(), "view_directions": views.cpu(),
               "generated": generated, "kept": int(points.shape[0])}
        write_mesh(file_point_cloud, out["points"], torch.zeros(0, 3, dtype=torch.int64), colors=out["colors"],
                   normals=out["normals"])
        return out

    def _set_rendering_defaults(self, camera_intrinsics: dict) -> None:
        self.ngp.nerf.sharpen = 0.0
        self.ngp.exposure = 0.0
        self.ngp.fov_axis = 0
        self.ngp.fov = (2 * math.atan(0.5 * camera_intrinsics["width"] / camera_intrinsics["fx"])) * 180 / np.pi
        self.ngp.nerf.render_with_lens_distortion = True
        self.ngp.nerf.render_min_transmittance = 1e-4

    def _set_camera_extrinsics(self, camera_extrinsics: np.ndarray) -> None:
        camera_extrinsics = np.array(camera_extrinsics, dtype=np.float64, copy=True)
        camera_extrinsics[0:3, 1:3] *= -1              # standard -> NeRF convention
        self.ngp.set_nerf_camera_matrix(camera_extrinsics[[2, 0, 1]])  # NeRF -> NGP row order


class NeRFSLAMNGPRenderer(InstantNGPRenderer):
    """Same renderer; the reference's subclass only locates the NeRF-SLAM build of pyngp (nerf_renderer.py:322-344)."""
