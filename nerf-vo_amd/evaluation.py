"""2-D evaluation loop around the native renderer: prediction<->ground-truth
alignment, rendering of evaluation frames to disk, and the depth / colour metrics computed from those files.

Mirrors the behaviour of the reference's
  * ``Renderer._calculate_pred2gt_transformation`` / ``transform_camera_extrinsics_gt2pred`` /
    ``transform_matrices_pred2gt`` / ``render_frames`` / ``_render_frame``
    (/root/reference/evaluation/renderer.py:79-124, 239-298),
  * ``calculate_depth_metrics_2d`` / ``calculate_psnr_color`` / ``calculate_mssim`` /
    ``calculate_color_metrics_2d`` (/root/reference/evaluation/evaluation_utils.py:289-443),
  * ``Evaluator.calculate_metrics_2d`` (/root/reference/evaluation/evaluator.py:88-146),
over ``nerf_vo_amd.mapping.renderer.NeRFRenderer`` objects.  Images are written with PIL (JPEG quality 95 is
OpenCV's ``imwrite`` default; 16-bit PNG depth) because OpenCV is not part of this image.  LPIPS needs
pretrained AlexNet weights that are not shipped and never fetched: ``lpips_loss`` is an optional callable --
``nerf_vo_amd.lpips.LPIPS.from_files(...)`` for the network in HIP, or any other -- and the ``lpips`` column is omitted
without it.

3-D (mesh) metrics: ``EvaluationRenderer.render_mesh`` produces the meshes (``source='frames'``: TSDF fusion of the rendered
frames, tsdf.py; ``source='nerf'``: the model's density iso-surface cropped to the ground-truth mesh's box, meshing.py) and
``calculate_metrics_3d`` / ``Evaluator3D`` score it against the ground-truth mesh the way the reference's
``calculate_metrics_3d`` (evaluation_utils.py:447-512) and ``Evaluator.calculate_metrics_3d`` (evaluator.py:148-174) do:
200 000 surface samples per mesh, voxel down-sampling at 1/64, point-to-point ICP of the prediction onto the ground
truth, nearest-neighbour distances both ways, ``accuracy / completion / precision / recall / f1score`` at 0.05.  The
reference uses Open3D and scipy on the CPU; here pointcloud.py does the cloud operations and the nearest-neighbour search
is a HIP kernel (csrc/nn.hip).  For the nerfstudio back-end, whose density mesh in the reference is a point cloud
followed by Open3D's Poisson reconstruction, ``EvaluationRenderer.render_point_cloud`` produces the cloud
(``pointcloud/pointcloud_from_nerf.ply``; mapping/renderer.py, the k-NN kernel csrc/knn.hip under its outlier removal) and
``calculate_metrics_3d_cloud`` / ``Evaluator3D.calculate_metrics_3d_clouds`` score it as a cloud; ``render_mesh(source='nerf')``
reconstructs the mesh from the same cloud (poisson.py: the project's dense-lattice Poisson rule, csrc/poisson.hip; parity with
Open3D's octree solver unpinned).

The 2-D table can also be computed on the GPU, on batches of frames (``Evaluator2D(device=...)``, metrics2d.py,
csrc/metrics2d.hip); the host functions below stay the default.  The trajectory table (``metrics_trajectory.csv``,
evaluator.py:55-83) is ``EvaluatorTrajectory`` over ``kabsch_umeyama_alignment`` / ``calculate_absolute_trajectory_error``
(evaluation_utils.py:230-286), float64 on the host, pinned by tests/golden/make_golden_trajectory.py.

The numeric functions are pinned by the reference's own outputs: tests/golden/make_golden_evaluation.py and
make_golden_metrics3d.py execute the reference's definitions on seeded inputs and tests/test_evaluation_cpu.py /
test_metrics3d_cpu.py compare.  For the 3-D table that covers the five formulae and the nearest-neighbour distances;
parity of the sampling, the down-sampling and the ICP with Open3D is UNPINNED (pointcloud.py).
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from .mapping.renderer import calculate_psnr_reference

DEPTH_VALID_MAX = 5.0  # metres; both the alignment and the metrics ignore depths outside (0, 5)


def _valid(depth_gt: np.ndarray, depth_pred: np.ndarray) -> np.ndarray:
    return (depth_gt > 0) & (depth_pred > 0) & (depth_gt < DEPTH_VALID_MAX) & (depth_pred < DEPTH_VALID_MAX)


def depth_scale_pred2gt(depth_gt: np.ndarray, depth_pred: np.ndarray) -> float:
    """Ratio of mean ground-truth to mean predicted depth over jointly valid pixels (renderer.py:88-93)."""
    m = _valid(depth_gt, depth_pred)
    return depth_gt[m].mean() / depth_pred[m].mean()


def estimate_pred2gt(depths_gt, depths_pred, extrinsics_gt0: np.ndarray, extrinsics_pred0: np.ndarray) -> dict:
    """Median per-keyframe depth scale + the rigid / scaled transforms anchored on frame 0
    (renderer.py:79-111).  Returns the reference's dictionary."""
    scale = np.median([depth_scale_pred2gt(g, p) for g, p in zip(depths_gt, depths_pred)])
    inv_pred0 = np.linalg.inv(extrinsics_pred0)
    return {
        "scale_pred2gt": scale,
        "matrix_pred2gt": extrinsics_gt0 @ inv_pred0,
        "matrix_pred2gt_scaled": extrinsics_gt0 @ np.diag([scale, scale, scale, 1]) @ inv_pred0,
    }


def _compose(rotation_from: np.ndarray, translation_from: np.ndarray, extrinsics: np.ndarray) -> np.ndarray:
    """Rotation block taken from ``rotation_from @ E``, translation column from ``translation_from @ E``.
    (The reference spells M @ E as ``(M @ E.T).T`` on the [n,4,4] stack, which is the same product.)"""
    extrinsics = np.asarray(extrinsics)
    out = np.tile(np.eye(4), (extrinsics.shape[0], 1, 1))
    out[:, :3, 3] = (translation_from @ extrinsics)[:, :3, 3]
    out[:, :3, :3] = (rotation_from @ extrinsics)[:, :3, :3]
    return out


def transform_camera_extrinsics_gt2pred(camera_extrinsics: np.ndarray, pred2gt_transformation: dict) -> np.ndarray:
    """Ground-truth poses -> the model's (normalised, unscaled) world (renderer.py:276-287)."""
    return _compose(np.linalg.inv(pred2gt_transformation["matrix_pred2gt"]),
                    np.linalg.inv(pred2gt_transformation["matrix_pred2gt_scaled"]), camera_extrinsics)


def transform_matrices_pred2gt(camera_extrinsics: np.ndarray, pred2gt_transformation: dict) -> np.ndarray:
    """Model-world poses -> ground-truth world (renderer.py:289-298)."""
    return _compose(pred2gt_transformation["matrix_pred2gt"], pred2gt_transformation["matrix_pred2gt_scaled"],
                    camera_extrinsics)


def calculate_depth_metrics_2d(frame_depth_gt: np.ndarray, frame_depth_pred: np.ndarray, with_scale: bool = True) -> dict:
    """evaluation_utils.py:380-415.  Relative errors are relative to the PREDICTION, like the reference."""
    m = _valid(frame_depth_gt, frame_depth_pred)
    gt = frame_depth_gt[m]
    pred = frame_depth_pred[m]
    if with_scale:
        pred = pred * (gt.mean() / pred.mean())
    diff = np.abs(pred - gt)
    ratio = np.maximum(gt / pred, pred / gt)
    return {
        "absolute_relative": np.mean(diff / pred),
        "absolute_difference": np.mean(diff),
        "square_relative": np.mean(diff ** 2 / pred),
        "square_difference": np.sqrt(np.mean(diff ** 2)),
        "square_log_difference": np.sqrt(np.mean((np.log(pred) - np.log(gt)) ** 2)),
        "delta1": np.mean((ratio < 1.25).astype("float")),
        "delta2": np.mean((ratio < 1.25 ** 2).astype("float")),
        "delta3": np.mean((ratio < 1.25 ** 3).astype("float")),
    }


ATE_METRICS = ("absolute_trajectory_error_rmse", "absolute_trajectory_error_mean", "absolute_trajectory_error_median",
               "absolute_trajectory_error_std", "absolute_trajectory_error_max", "absolute_trajectory_error_min")


def kabsch_umeyama_alignment(points_target: np.ndarray, points_source: np.ndarray, with_scale: bool = True) -> tuple:
    """Least-squares similarity ``target ~ scale * rotation @ source + translation`` of two [N, D] point sets (Umeyama 1991;
    evaluation_utils.py:230-252): SVD of the cross-covariance, the last singular direction flipped when the two bases
    disagree in handedness (a reflection is never returned), scale = target variance over the signed singular-value sum.
    Returns ``(rotation [D, D], translation [D, 1], scale)``; float64 on the host."""
    points_target, points_source = np.asarray(points_target), np.asarray(points_source)
    assert points_target.shape == points_source.shape
    n, dims = points_target.shape
    mean_target, mean_source = points_target.mean(axis=0), points_source.mean(axis=0)
    variance_target = np.mean(np.linalg.norm(points_target - mean_target, axis=1) ** 2)
    covariance = ((points_target - mean_target).T @ (points_source - mean_source)) / n
    u, d, vt = np.linalg.svd(covariance)
    s = np.diag([1] * (dims - 1) + [np.sign(np.linalg.det(u) * np.linalg.det(vt))])
    rotation = u @ s @ vt
    scale = variance_target / np.trace(np.diag(d) @ s) if with_scale else 1.0
    translation = mean_target - scale * rotation @ mean_source
    return rotation, translation.reshape(dims, 1), scale


def calculate_absolute_trajectory_error(matrices_origin2frame_gt: np.ndarray, matrices_origin2frame_pred: np.ndarray,
                                        with_scale: bool = True) -> dict:
    """The six absolute-trajectory-error statistics of the predicted camera centres after their Kabsch-Umeyama alignment
    onto the ground truth's (evaluation_utils.py:255-286).  [N, 4, 4] camera-to-world matrices each."""
    trajectory_gt = np.asarray(matrices_origin2frame_gt)[:, :3, 3]
    trajectory_pred = np.asarray(matrices_origin2frame_pred)[:, :3, 3]
    rotation, translation, scale = kabsch_umeyama_alignment(trajectory_gt, trajectory_pred, with_scale=with_scale)
    aligned = (scale * rotation @ trajectory_pred.T + translation).T
    residual = aligned - trajectory_gt
    error = np.sqrt(np.sum(np.multiply(residual, residual), axis=1))
    values = (np.sqrt(np.dot(error, error) / len(error)), np.mean(error), np.median(error), np.std(error), np.max(error),
              np.min(error))
    return dict(zip(ATE_METRICS, values))


def calculate_mssim(image1: torch.Tensor, image2: torch.Tensor) -> float:
    """Mean SSIM of two [1,3,H,W] tensors with an 11-tap Gaussian window (sigma 1.5), zero padding,
    C1 = 0.01^2, C2 = 0.03^2 (evaluation_utils.py:321-377).  The window is applied as two 1-D passes
    (same operator as the reference's 11x11 depth-wise convolution)."""
    taps, sigma = 11, 1.5
    x = torch.arange(taps, dtype=torch.float32) - taps // 2
    g = torch.exp(-(x ** 2) / (2 * sigma ** 2))
    g = g / g.sum()
    channels = image1.shape[1]
    row = g.view(1, 1, 1, taps).expand(channels, 1, 1, taps).contiguous()
    col = g.view(1, 1, taps, 1).expand(channels, 1, taps, 1).contiguous()

    def blur(t: torch.Tensor) -> torch.Tensor:
        t = torch.nn.functional.conv2d(t, row, padding=(0, taps // 2), groups=channels)
        return torch.nn.functional.conv2d(t, col, padding=(taps // 2, 0), groups=channels)

    with torch.no_grad():
        a, b = image1.float(), image2.float()
        mu_a, mu_b = blur(a), blur(b)
        var_a = blur(a * a) - mu_a ** 2
        var_b = blur(b * b) - mu_b ** 2
        cov = blur(a * b) - mu_a * mu_b
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        ssim = ((2 * mu_a * mu_b + c1) * (2 * cov + c2)) / ((mu_a ** 2 + mu_b ** 2 + c1) * (var_a + var_b + c2))
        return ssim.mean().item()


def calculate_color_metrics_2d(frame_color_gt: np.ndarray, frame_color_pred: np.ndarray, lpips_loss=None) -> dict:
    """PSNR (the reference's uint8-wrapping per-channel definition), MSSIM on [-1,1]-scaled images and --
    when a callable is supplied -- LPIPS on the twice-rescaled tensors the reference feeds it
    (evaluation_utils.py:418-443)."""
    def to_tensor(img: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).unsqueeze(0).float().div(255.0) * 2 - 1

    gt, pred = to_tensor(frame_color_gt), to_tensor(frame_color_pred)
    out = {"psnr": calculate_psnr_reference(frame_color_gt, frame_color_pred), "mssim": calculate_mssim(gt, pred)}
    if lpips_loss is not None:
        out["lpips"] = float(lpips_loss(gt * 2 - 1, pred * 2 - 1))
    return out


# ---------------------------------------------------------------------------------------------------------------
# rendering of evaluation frames to disk
# ---------------------------------------------------------------------------------------------------------------
def write_color_jpeg(path: str, rgb: np.ndarray) -> None:
    from PIL import Image

    Image.fromarray(rgb, mode="RGB").save(path, format="JPEG", quality=95)


def read_color(path: str) -> np.ndarray:
    from PIL import Image

    return np.asarray(Image.open(path).convert("RGB"))


def write_depth_png16(path: str, depth_units: np.ndarray) -> None:
    from PIL import Image

    Image.fromarray(depth_units.astype(np.uint16)).save(path, format="PNG")


def read_depth_png16(path: str) -> np.ndarray:
    from PIL import Image

    return np.asarray(Image.open(path)).astype(np.uint16)


class EvaluationRenderer:
    """``dataset`` provides ``camera_intrinsics`` (dict with fx, fy, cx, cy, height, width, depth_scale),
    ``camera_extrinsics`` ([N,4,4] ground-truth c2w, standard axes), ``evaluation_frames``, ``num_frames`` and
    ``frames_depth(mode=, keyframes=)``; ``nerf`` is a ``NeRFRenderer``; ``keyframes`` the dataset indices of the
    training keyframes (renderer.py:33-63)."""

    def __init__(self, dataset, nerf, keyframes, dir_prediction: str) -> None:
        self.dataset = dataset
        self.nerf = nerf
        self.keyframes = list(keyframes)
        self.dir_prediction = dir_prediction
        self._calculate_pred2gt_transformation()

    def _process_mode(self, mode: str) -> tuple:
        if mode == "evaluation_frames":
            return "evaluation_frames", list(self.dataset.evaluation_frames)
        if mode == "keyframes":
            return "keyframes", list(self.keyframes)
        if mode == "all":
            return "all_frames", list(range(self.dataset.num_frames))  # (the reference's len(int) would raise)
        raise NotImplementedError(mode)

    def _calculate_pred2gt_transformation(self) -> None:
        depths_gt = self.dataset.frames_depth(mode="keyframes", keyframes=self.keyframes)
        depths_pred = [self.nerf.render_frame_depth_from_training_frame(
            camera_intrinsics=self.dataset.camera_intrinsics, frame_index=i) for i in range(len(depths_gt))]
        self.pred2gt_transformation = estimate_pred2gt(
            depths_gt, depths_pred, np.asarray(self.dataset.camera_extrinsics[0], dtype=np.float64),
            self.nerf.get_camera_extrinsics(frame_index=0))

    def _render_frame(self, camera_extrinsics: np.ndarray, file_color: str, file_depth: str) -> None:
        color, depth = self.nerf.render_frame(camera_intrinsics=self.dataset.camera_intrinsics,
                                              camera_extrinsics=camera_extrinsics)
        units = depth * self.pred2gt_transformation["scale_pred2gt"] * self.dataset.camera_intrinsics["depth_scale"]
        write_color_jpeg(file_color, color)
        write_depth_png16(file_depth, units)

    def render_frames(self, mode: str = "evaluation_frames") -> list:
        folder, indices = self._process_mode(mode)
        os.makedirs(f"{self.dir_prediction}/{folder}/color", exist_ok=True)
        os.makedirs(f"{self.dir_prediction}/{folder}/depth", exist_ok=True)
        gt = np.stack([np.asarray(self.dataset.camera_extrinsics[i], dtype=np.float64) for i in indices])
        for index, pose in zip(indices, transform_camera_extrinsics_gt2pred(gt, self.pred2gt_transformation)):
            self._render_frame(pose, f"{self.dir_prediction}/{folder}/color/{index:06d}.jpg",
                               f"{self.dir_prediction}/{folder}/depth/{index:06d}.png")
        return indices

    def render_mesh(self, source: str = "frames", mode: str = "evaluation_frames", volume: str = "dense", **kwargs) -> str:
        """``source='frames'``: ``mesh/mesh_from_<mode>.ply`` fused from the colour / depth files ``render_frames(mode)``
        wrote (rendered first when their folder is absent) at the ground-truth poses of those frames (renderer.py:126-164,
        265-273): TSDF fusion on the GPU, nerf_vo_amd/tsdf.py, into a dense volume (``volume='dense'``) or a block-sparse one
        as the reference's (``volume='blocks'``).  ``source='nerf'``: ``mesh/mesh_from_nerf.ply``, the
        mesh of the model's field cropped to the ground-truth mesh's box (``_render_mesh_from_nerf``; ``kwargs`` go to the
        model renderer's ``render_mesh``).  Returns the file's path."""
        if source == "nerf":
            if volume != "dense":
                raise TypeError("render_mesh(source='nerf') takes no volume")
            return self._render_mesh_from_nerf(**kwargs)
        if kwargs:
            raise TypeError(f"render_mesh(source={source!r}) takes no further arguments, got {sorted(kwargs)}")
        if source != "frames":
            raise NotImplementedError(source)
        from .tsdf import integrate_mesh

        folder, indices = self._process_mode(mode)
        os.makedirs(f"{self.dir_prediction}/mesh", exist_ok=True)
        if not os.path.exists(f"{self.dir_prediction}/{folder}"):
            self.render_frames(mode=mode)
        file_mesh = f"{self.dir_prediction}/mesh/mesh_from_{mode}.ply"
        color_dir, depth_dir = f"{self.dir_prediction}/{folder}/color", f"{self.dir_prediction}/{folder}/depth"
        colors = [read_color(os.path.join(color_dir, f)) for f in sorted(os.listdir(color_dir)) if f.endswith(".jpg")]
        depths = [read_depth_png16(os.path.join(depth_dir, f)) / self.dataset.camera_intrinsics["depth_scale"]
                  for f in sorted(os.listdir(depth_dir)) if f.endswith(".png")]
        extrinsics = np.stack([np.asarray(self.dataset.camera_extrinsics[i], dtype=np.float64) for i in indices])
        integrate_mesh(file_mesh=file_mesh, camera_intrinsics=self.dataset.camera_intrinsics, camera_extrinsics=extrinsics,
                       frames_color=colors, frames_depth=depths, volume=volume)
        return file_mesh

    def _ground_truth_box_in_model_frame(self) -> tuple:
        """``(lower_gt, upper_gt, matrix, lower, upper)``: the box of the ground-truth mesh's vertices, matrix_pred2gt_scaled,
        and the box of that box's eight corners mapped into the model's frame by its inverse (float64) -- shared by the
        density mesh and the point cloud."""
        mesh_gt, _ = self.dataset.mesh()
        points_gt = np.asarray(torch.as_tensor(mesh_gt[0]).detach().cpu().numpy(), dtype=np.float64)
        lower_gt, upper_gt = points_gt.min(axis=0), points_gt.max(axis=0)
        corners = np.array([[x, y, z, 1.0] for x in (lower_gt[0], upper_gt[0]) for y in (lower_gt[1], upper_gt[1])
                            for z in (lower_gt[2], upper_gt[2])])
        matrix = np.asarray(self.pred2gt_transformation["matrix_pred2gt_scaled"], dtype=np.float64)
        corners_pred = np.linalg.inv(matrix) @ corners.T  # [4, 8]
        lower, upper = np.min(corners_pred, axis=1)[:3], np.max(corners_pred, axis=1)[:3]
        return lower_gt, upper_gt, matrix, lower, upper

    def _render_mesh_from_nerf(self, **kwargs) -> str:
        """The reference's ``_render_mesh_from_nerf`` (renderer.py:166-210): the box of the ground-truth mesh's vertices is
        mapped into the model's frame by inv(matrix_pred2gt_scaled), the model's renderer writes its mesh over the box of
        the mapped corners (``mesh/mesh_from_nerf_raw.ply``: the density iso-surface at 1/64 m for the occupancy-grid
        back-end, the Poisson reconstruction of the oriented cloud for the nerfstudio back-end, which takes ``kwargs``), and
        that mesh, mapped back by matrix_pred2gt_scaled and cropped to the ground-truth box, is ``mesh/mesh_from_nerf.ply``;
        vertex colours of the raw file, when it has them, are kept, and so are its vertex normals (the occupancy-grid
        renderer's ``vertex_attributes=True``), rotated by ``rotate_normals``.  Open3D's transform and crop are
        meshing.transform_mesh / crop_mesh here (parity with Open3D unpinned)."""
        from .meshing import crop_mesh, read_mesh, transform_mesh, write_mesh

        if not callable(getattr(self.nerf, "render_mesh", None)):
            raise NotImplementedError(
                f"render_mesh(source='nerf'): {type(self.nerf).__name__} has no render_mesh(file_mesh, resolution, lower_bound, "
                "upper_bound).  The occupancy-grid back-end has one (InstantNGPRenderer.render_mesh -> "
                "pyngp.Testbed.compute_and_save_marching_cubes_mesh), and so has the nerfstudio back-end "
                "(NerfstudioRenderer.render_mesh: the oriented point cloud and its Poisson reconstruction, poisson.py)")
        voxel_size = 1 / 64
        os.makedirs(f"{self.dir_prediction}/mesh", exist_ok=True)
        lower_gt, upper_gt, matrix, lower, upper = self._ground_truth_box_in_model_frame()
        resolution = ((upper - lower) * self.pred2gt_transformation["scale_pred2gt"] / voxel_size).astype(int)
        file_raw = f"{self.dir_prediction}/mesh/mesh_from_nerf_raw.ply"
        self.nerf.render_mesh(file_mesh=file_raw, resolution=resolution, lower_bound=lower, upper_bound=upper, **kwargs)
        vertices, faces, colors, normals = read_mesh(file_raw)
        vertices, faces, keep = crop_mesh(transform_mesh(vertices, matrix), faces, lower_gt, upper_gt)
        if vertices.shape[0] == 0 or faces.shape[0] == 0:
            raise RuntimeError(
                f"render_mesh(source='nerf'): nothing of {file_raw} lies inside the ground-truth mesh's box "
                f"{lower_gt.tolist()} .. {upper_gt.tolist()}, so mesh_from_nerf.ply is not written: the density never crosses the "
                "iso-surface threshold there (thresh of compute_and_save_marching_cubes_mesh, 2.5 by default) -- train longer or "
                "extract at a lower thresh (a Poisson mesh: every vertex was trimmed, or the cloud is empty there)")
        file_mesh = f"{self.dir_prediction}/mesh/mesh_from_nerf.ply"
        if normals is not None:  # (a raw file written with vertex_attributes: rotated the way the cloud's normals are)
            normals = rotate_normals(normals[keep], matrix, self.pred2gt_transformation["scale_pred2gt"])
        write_mesh(file_mesh, vertices, faces, colors=None if colors is None else colors[keep], normals=normals)
        return file_mesh

    def render_point_cloud(self, num_points: int = 33554432, **kwargs) -> str:
        """``pointcloud/pointcloud_from_nerf.ply``: the first half of the reference's nerfstudio ``render_mesh``
        (evaluation/nerf_renderer.py:170-209 there), wrapped the way ``_render_mesh_from_nerf`` wraps the density mesh.  The
        ground-truth mesh's box is mapped into the model's frame by inv(matrix_pred2gt_scaled); the model's renderer writes
        its oriented, coloured cloud over the box of the mapped corners to ``pointcloud/pointcloud_from_nerf_raw.ply``
        (``NerfstudioRenderer.render_point_cloud``; ``kwargs`` go to it); the points are mapped back by
        ``transform_mesh``'s rule, the normals by the rotation part alone (the linear part divided by ``scale_pred2gt``,
        float64 row by row, re-normalised), and the cloud cropped to the ground-truth box is written with ``x y z nx ny nz
        red green blue`` and no faces.  Its own folder, because ``Evaluator3D.calculate_metrics_3d`` reads every
        ``mesh/*.ply`` as a mesh.  Returns the file's path."""
        from .meshing import crop_mesh, read_mesh, transform_mesh, write_mesh

        if not callable(getattr(self.nerf, "render_point_cloud", None)):
            raise NotImplementedError(
                f"render_point_cloud: {type(self.nerf).__name__} has no render_point_cloud(file_point_cloud, lower_bound, "
                "upper_bound, num_points).  Both back-ends have one (NerfstudioRenderer.render_point_cloud: predicted normals; "
                "InstantNGPRenderer.render_point_cloud: rendered density-gradient normals); a renderer that predicts no normals "
                "cannot orient a cloud, and estimating them from neighbours is not built")
        os.makedirs(f"{self.dir_prediction}/pointcloud", exist_ok=True)
        lower_gt, upper_gt, matrix, lower, upper = self._ground_truth_box_in_model_frame()
        file_raw = f"{self.dir_prediction}/pointcloud/pointcloud_from_nerf_raw.ply"
        self.nerf.render_point_cloud(file_point_cloud=file_raw, lower_bound=lower, upper_bound=upper, num_points=int(num_points),
                                     **kwargs)
        points, _, colors, normals = read_mesh(file_raw)
        if normals is None or colors is None:
            raise RuntimeError(f"render_point_cloud: {file_raw} has no normals or no colours")
        no_faces = torch.zeros(0, 3, dtype=torch.int64)
        points, _, keep = crop_mesh(transform_mesh(points, matrix), no_faces, lower_gt, upper_gt)
        if points.shape[0] == 0:
            raise RuntimeError(f"render_point_cloud: nothing of {file_raw} lies inside the ground-truth mesh's box "
                               f"{lower_gt.tolist()} .. {upper_gt.tolist()}, so pointcloud_from_nerf.ply is not written")
        normals = rotate_normals(normals[keep], matrix, self.pred2gt_transformation["scale_pred2gt"])
        file_cloud = f"{self.dir_prediction}/pointcloud/pointcloud_from_nerf.ply"
        write_mesh(file_cloud, points, no_faces, colors=colors[keep], normals=normals)
        return file_cloud

    def export_keyframe_poses(self) -> np.ndarray:
        """matrices/matrices_origin2frame_keyframes_mapping.json: training poses with the translation in
        ground-truth metres (renderer.py:225-236)."""
        poses = np.stack([self.nerf.get_camera_extrinsics(frame_index=i) for i in range(len(self.keyframes))])
        poses[:, :3, 3] *= self.pred2gt_transformation["scale_pred2gt"]
        os.makedirs(f"{self.dir_prediction}/matrices", exist_ok=True)
        with open(f"{self.dir_prediction}/matrices/matrices_origin2frame_keyframes_mapping.json", "w") as file:
            json.dump(poses.tolist(), file)
        return poses


class Evaluator2D:
    """Per-frame depth + colour metrics of the frames ``EvaluationRenderer.render_frames`` wrote
    (evaluator.py:88-146): ``metrics_2d_<folder>.csv`` (one row per frame) and ``.json`` (column means)."""

    def __init__(self, dataset, keyframes, dir_prediction: str, dir_result: str, lpips_loss=None, device=None,
                 frames_per_launch: int = 8) -> None:
        """``device``: None computes every frame on the host (the functions above); a CUDA device uploads the decoded
        frames ``frames_per_launch`` at a time and computes the same columns there (metrics2d.py, csrc/metrics2d.hip):
        ``psnr`` is equal, the others agree to the bounds of DESIGN.md section 16.  ``lpips_loss``: a
        ``nerf_vo_amd.lpips.LPIPS`` model computes the ``lpips`` column on the device, from the batch already uploaded for
        the colour metrics (host path: frame by frame through the model, same values); any other callable is fed on the
        host, frame by frame."""
        self.dataset = dataset
        self.keyframes = list(keyframes)
        self.dir_prediction = dir_prediction
        self.dir_result = dir_result
        self.lpips_loss = lpips_loss
        self.device = None if device is None else torch.device(device)
        self.frames_per_launch = max(int(frames_per_launch), 1)
        if self.device is not None and self.device.type != "cuda":
            raise ValueError(f"Evaluator2D: device must be None (host) or a CUDA device, got {device!r}")

    def _rows_on_device(self, depths_gt, depths_pred, colors_gt, colors_pred) -> list:
        from . import metrics2d

        def depth_array(d):  # (the kernel takes float32 and float64 and computes in float64 either way)
            d = np.asarray(d)
            return d if d.dtype in (np.float32, np.float64) else d.astype(np.float64)

        def key(frame):  # a launch takes frames of one shape and type
            return tuple((x.shape, x.dtype) for x in frame)

        def upload(arrays):
            return torch.from_numpy(np.stack(arrays)).to(self.device)

        def to_tensor(img):
            return torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).unsqueeze(0).float().div(255.0) * 2 - 1

        from .lpips import LPIPS

        lpips_model = self.lpips_loss if isinstance(self.lpips_loss, LPIPS) else None
        frames = [(depth_array(dg), depth_array(dp), np.asarray(cg), np.asarray(cp))
                  for dg, dp, cg, cp in zip(depths_gt, depths_pred, colors_gt, colors_pred)]
        rows, lo = [], 0
        while lo < len(frames):
            hi = lo + 1
            while hi < len(frames) and hi - lo < self.frames_per_launch and key(frames[hi]) == key(frames[lo]):
                hi += 1
            d_gt, d_pred, c_gt, c_pred = (list(column) for column in zip(*frames[lo:hi]))
            depth_rows = metrics2d.depth_metrics(upload(d_gt), upload(d_pred))
            color_rows = metrics2d.color_metrics(upload(c_gt), upload(c_pred), lpips=lpips_model)
            for k, (depth_row, color_row) in enumerate(zip(depth_rows, color_rows)):
                row = {**depth_row, **color_row}
                if self.lpips_loss is not None and lpips_model is None:  # on the host, fed as calculate_color_metrics_2d feeds it
                    row["lpips"] = float(self.lpips_loss(to_tensor(c_gt[k]) * 2 - 1, to_tensor(c_pred[k]) * 2 - 1))
                rows.append(row)
            lo = hi
        return rows

    def calculate_metrics_2d(self, mode: str = "evaluation_frames") -> dict:
        import pandas as pd

        folder = {"evaluation_frames": "evaluation_frames", "keyframes": "keyframes", "all": "all_frames"}[mode]
        colors_gt = self.dataset.frames_color(mode=mode, keyframes=self.keyframes)
        depths_gt = self.dataset.frames_depth(mode=mode, keyframes=self.keyframes)
        color_dir, depth_dir = f"{self.dir_prediction}/{folder}/color", f"{self.dir_prediction}/{folder}/depth"
        colors_pred = [read_color(os.path.join(color_dir, f)) for f in sorted(os.listdir(color_dir)) if f.endswith(".jpg")]
        depths_pred = [read_depth_png16(os.path.join(depth_dir, f)) / self.dataset.camera_intrinsics["depth_scale"]
                       for f in sorted(os.listdir(depth_dir)) if f.endswith(".png")]
        rows = []
        if self.device is not None:
            rows = self._rows_on_device(depths_gt, depths_pred, colors_gt, colors_pred)
        else:
            for d_gt, d_pred, c_gt, c_pred in zip(depths_gt, depths_pred, colors_gt, colors_pred):
                row = dict(calculate_depth_metrics_2d(frame_depth_gt=d_gt, frame_depth_pred=d_pred))
                row.update(calculate_color_metrics_2d(frame_color_gt=c_gt, frame_color_pred=c_pred,
                                                      lpips_loss=self.lpips_loss))
                rows.append(row)
        table = pd.DataFrame(rows)
        os.makedirs(self.dir_result, exist_ok=True)
        table.to_csv(f"{self.dir_result}/metrics_2d_{folder}.csv", index=False)
        means = table.mean().to_dict()
        with open(f"{self.dir_result}/metrics_2d_{folder}.json", "w") as file:
            json.dump(means, file)
        return means


class EvaluatorTrajectory:
    """``Evaluator.calculate_metrics_trajectory`` (evaluator.py:55-83): the keyframe trajectories under
    ``<dir_prediction>/matrices/matrices_origin2frame_keyframes_{tracking,mapping}.json`` against the ground-truth poses
    of the keyframes, aligned with scale -> ``<dir_result>/metrics_trajectory.csv``, one row per file: the six ATE
    statistics and ``trajectory``.  The reference reads both files; tracking is not part of this project, so a file that
    is absent is left out, and only the absence of both is an error.  ``EvaluationRenderer.export_keyframe_poses``
    writes the mapping file."""

    TRAJECTORIES = ("keyframes_tracking", "keyframes_mapping")

    def __init__(self, dataset, keyframes, dir_prediction: str, dir_result: str) -> None:
        self.dataset = dataset
        self.keyframes = list(keyframes)
        self.dir_prediction = dir_prediction
        self.dir_result = dir_result

    def calculate_metrics_trajectory(self) -> dict:
        import pandas as pd

        poses_gt = np.stack([np.asarray(self.dataset.camera_extrinsics[i], dtype=np.float64) for i in self.keyframes])
        rows = []
        for trajectory in self.TRAJECTORIES:
            path = f"{self.dir_prediction}/matrices/matrices_origin2frame_{trajectory}.json"
            if not os.path.exists(path):
                continue
            with open(path) as file:
                poses_pred = np.array(json.load(file))
            if poses_pred.shape != poses_gt.shape:
                raise ValueError(f"{path} holds poses of shape {poses_pred.shape}, the {len(self.keyframes)} keyframes need "
                                 f"{poses_gt.shape}")
            row = calculate_absolute_trajectory_error(poses_gt, poses_pred, with_scale=True)
            row["trajectory"] = trajectory
            rows.append(row)
        if not rows:
            raise FileNotFoundError(f"{self.dir_prediction}/matrices holds neither matrices_origin2frame_keyframes_tracking.json "
                                    "nor matrices_origin2frame_keyframes_mapping.json (EvaluationRenderer.export_keyframe_poses "
                                    "writes the latter)")
        table = pd.DataFrame(rows, columns=list(ATE_METRICS) + ["trajectory"])
        os.makedirs(self.dir_result, exist_ok=True)
        table.to_csv(f"{self.dir_result}/metrics_trajectory.csv", index=False)
        return table[list(ATE_METRICS)].squeeze().to_dict()


def rotate_normals(normals, matrix, scale: float) -> torch.Tensor:
    """Unit normals under the scaled rigid transform ``matrix`` (4 x 4, linear part = ``scale`` * rotation): mapped by the
    rotation ``matrix[:3, :3] / scale`` alone, row r as ``(m[r][0]*x + m[r][1]*y) + m[r][2]*z`` in float64 (one product or sum
    per step, like ``transform_mesh``), re-normalised, float32."""
    n = torch.as_tensor(normals).to(torch.float64)
    m = np.asarray(matrix, dtype=np.float64)[:3, :3] / float(scale)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    rows = [(float(m[r, 0]) * x + float(m[r, 1]) * y) + float(m[r, 2]) * z for r in range(3)]
    out = torch.stack(rows, dim=1)
    return (out / torch.linalg.norm(out, dim=1, keepdim=True).clamp_min(1e-300)).to(torch.float32)


# ---------------------------------------------------------------------------------------------------------------
# 3-D (mesh) metrics
# ---------------------------------------------------------------------------------------------------------------
METRIC_THRESHOLD_3D = 0.05     # the reference's constants (calculate_metrics_3d)
NUM_SAMPLE_POINTS_3D = 200000
VOXEL_SIZE_3D = 1.0 / 64.0
METRICS_3D = ("accuracy", "completion", "precision", "recall", "f1score")


def metrics_3d_from_distances(distances_gt_to_pred, distances_pred_to_gt) -> dict:
    """The tail of the reference's ``calculate_metrics_3d`` (evaluation_utils.py:496-510), with its names:
    ``distances_gt_to_pred`` holds, for every PREDICTED point, the distance to its nearest ground-truth point (the query
    of the ground truth's tree), ``distances_pred_to_gt`` the reverse.  So "accuracy" is prediction -> ground truth and
    "completion" ground truth -> prediction; precision / recall are the shares below 0.05 (strictly)."""
    d_gt_to_pred = np.asarray(distances_gt_to_pred, dtype=np.float64)
    d_pred_to_gt = np.asarray(distances_pred_to_gt, dtype=np.float64)
    precision = np.mean((d_gt_to_pred < METRIC_THRESHOLD_3D).astype(float))
    recall = np.mean((d_pred_to_gt < METRIC_THRESHOLD_3D).astype(float))
    return {"accuracy": float(np.mean(d_gt_to_pred)), "completion": float(np.mean(d_pred_to_gt)),
            "precision": float(precision), "recall": float(recall),
            "f1score": float(2 * precision * recall / (precision + recall))}


def sample_metric_clouds(mesh_gt, mesh_pred, seed: int = 0, device="cuda", number_of_points: int = NUM_SAMPLE_POINTS_3D,
                         voxel_size: float = VOXEL_SIZE_3D) -> tuple:
    """The two clouds the metrics are computed from: ``number_of_points`` uniform surface samples of each mesh (one CPU
    generator seeded with ``seed``: ground truth first), voxel down-sampled.  float32 [K, 3] tensors on ``device``."""
    from .pointcloud import sample_points_uniformly, voxel_down_sample

    gen = torch.Generator().manual_seed(int(seed))
    clouds = []
    for vertices, faces in (mesh_gt, mesh_pred):
        v = torch.as_tensor(vertices).to(device)
        pts = sample_points_uniformly(v, torch.as_tensor(faces).to(device), number_of_points, generator=gen)
        clouds.append(voxel_down_sample(pts, voxel_size))
    return clouds[0], clouds[1]


def metrics_3d_from_clouds(points_gt: torch.Tensor, points_pred: torch.Tensor, cell_size=None) -> dict:
    """ICP of the predicted cloud onto the ground-truth cloud (the reference's settings), then the two nearest-neighbour
    tables and ``metrics_3d_from_distances``.  Both clouds on the GPU."""
    from .pointcloud import DEFAULT_CELL_SIZE, NeighbourGrid, icp_point_to_point

    cell_size = DEFAULT_CELL_SIZE if cell_size is None else cell_size
    grid_gt = NeighbourGrid(points_gt, cell_size)
    transformation, _, _, _ = icp_point_to_point(points_pred, grid_gt)
    t = torch.from_numpy(transformation).to(points_pred.device)
    moved = (points_pred.double() @ t[:3, :3].T + t[:3, 3]).float()
    d2_pred_to_gt, _ = NeighbourGrid(moved, cell_size).query(points_gt)   # for every ground-truth point
    d2_gt_to_pred, _ = grid_gt.query(moved)                               # for every predicted point
    return metrics_3d_from_distances(d2_gt_to_pred.double().sqrt().cpu().numpy(), d2_pred_to_gt.double().sqrt().cpu().numpy())


def calculate_metrics_3d(mesh_gt, mesh_pred, seed: int = 0, device="cuda") -> dict:
    """The reference's ``calculate_metrics_3d(mesh_gt, mesh_pred)`` (evaluation_utils.py:466-512); each mesh is a
    ``(vertices [V, 3], faces [F, 3])`` pair.  ``seed`` fixes the surface samples (Open3D draws them from its global
    generator)."""
    points_gt, points_pred = sample_metric_clouds(mesh_gt, mesh_pred, seed=seed, device=device)
    return metrics_3d_from_clouds(points_gt, points_pred)


def calculate_metrics_3d_cloud(mesh_gt, points_pred, seed: int = 0, device="cuda") -> dict:
    """``calculate_metrics_3d`` for a prediction that already is a cloud (``EvaluationRenderer.render_point_cloud``): the
    ground-truth cloud as there -- ``NUM_SAMPLE_POINTS_3D`` surface samples from a CPU generator seeded with ``seed``, voxel
    down-sampled at 1/64 -- the predicted points voxel down-sampled at 1/64 directly, then ``metrics_3d_from_clouds``."""
    from .pointcloud import sample_points_uniformly, voxel_down_sample

    gen = torch.Generator().manual_seed(int(seed))
    v = torch.as_tensor(mesh_gt[0]).to(device)
    points_gt = voxel_down_sample(sample_points_uniformly(v, torch.as_tensor(mesh_gt[1]).to(device), NUM_SAMPLE_POINTS_3D,
                                                          generator=gen), VOXEL_SIZE_3D)
    cloud = voxel_down_sample(torch.as_tensor(points_pred).to(device), VOXEL_SIZE_3D)
    return metrics_3d_from_clouds(points_gt, cloud)


class Evaluator3D:
    """``Evaluator.calculate_metrics_3d`` (evaluator.py:148-174): every ``<dir_prediction>/mesh/*.ply`` except
    ``mesh_from_nerf_raw`` against ``dataset.mesh()`` -> ``<dir_result>/metrics_3d.csv`` (the five metrics and ``mesh``,
    one row per file, files in sorted order).  ``calculate_metrics_3d_clouds`` does the same for the point clouds under
    ``<dir_prediction>/pointcloud`` -> ``metrics_3d_pointcloud.csv``."""

    def __init__(self, dataset, dir_prediction: str, dir_result: str, seed: int = 0, device="cuda") -> None:
        self.dataset = dataset
        self.dir_prediction = dir_prediction
        self.dir_result = dir_result
        self.seed = seed
        self.device = device

    def calculate_metrics_3d(self) -> dict:
        import pandas as pd

        from .meshing import read_mesh

        mesh_gt, _ = self.dataset.mesh()
        rows = []
        for name in sorted(os.listdir(f"{self.dir_prediction}/mesh")):
            stem, ext = os.path.splitext(name)
            if ext != ".ply" or stem == "mesh_from_nerf_raw":
                continue
            vertices, faces = read_mesh(f"{self.dir_prediction}/mesh/{name}")[:2]
            row = calculate_metrics_3d(mesh_gt=mesh_gt[:2], mesh_pred=(vertices, faces), seed=self.seed, device=self.device)
            row["mesh"] = stem
            rows.append(row)
        table = pd.DataFrame(rows, columns=list(METRICS_3D) + ["mesh"])
        os.makedirs(self.dir_result, exist_ok=True)
        table.to_csv(f"{self.dir_result}/metrics_3d.csv", index=False)
        return table[list(METRICS_3D)].squeeze().to_dict()

    def calculate_metrics_3d_clouds(self) -> dict:
        """Every ``<dir_prediction>/pointcloud/*.ply`` except ``*_raw`` against ``dataset.mesh()`` ->
        ``<dir_result>/metrics_3d_pointcloud.csv`` with the columns of ``metrics_3d.csv`` (the file's name goes into
        ``mesh``), one row per file in sorted order (``calculate_metrics_3d_cloud``)."""
        import pandas as pd

        from .meshing import read_mesh

        mesh_gt, _ = self.dataset.mesh()
        rows = []
        for name in sorted(os.listdir(f"{self.dir_prediction}/pointcloud")):
            stem, ext = os.path.splitext(name)
            if ext != ".ply" or stem.endswith("_raw"):
                continue
            points = read_mesh(f"{self.dir_prediction}/pointcloud/{name}")[0]
            row = calculate_metrics_3d_cloud(mesh_gt=mesh_gt[:2], points_pred=points, seed=self.seed, device=self.device)
            row["mesh"] = stem
            rows.append(row)
        table = pd.DataFrame(rows, columns=list(METRICS_3D) + ["mesh"])
        os.makedirs(self.dir_result, exist_ok=True)
        table.to_csv(f"{self.dir_result}/metrics_3d_pointcloud.csv", index=False)
        return table[list(METRICS_3D)].squeeze().to_dict()
