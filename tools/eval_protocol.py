#!/usr/bin/env python3
"""The reference's PUBLISHED evaluation protocol on a natively trained model.

Train through the Nerfstudio mapper interface (incremental keyframe ingest), then evaluate exactly as
/root/reference/run.py:57-79 does: ``Renderer`` (evaluation/renderer.py) aligns prediction and ground truth through
FRAME 0's pose and the MEDIAN per-keyframe depth scale (:79-111), keyframe views are rendered at the model's own
(optimised) training poses (evaluation/nerf_renderer.py:125-130), evaluation frames at ground-truth poses carried into
the model's world (renderer.py:276-287), everything goes through JPEG / 16-bit PNG files (:118-124), and ``Evaluator``
scores the files (evaluator.py:88-146; PSNR = the reference's uint8-wrapping definition).  Here: nerf_vo_amd.evaluation's
EvaluationRenderer / Evaluator2D, whose numerics are pinned by the reference's own functions (tests/golden/
make_golden_evaluation.py).

``pose_noise = (sigma_rot [rad], sigma_trans)``: the ingested keyframe poses are perturbed the way a tracker's would be
(frame 0 exact: it anchors the world) -- BASELINE configs[2], where the SE3 camera optimiser has something to recover.
Reports, next to the 2-D metrics, the pose error of the exported keyframe trajectory after the protocol's frame-0
alignment (translation RMSE, mean rotation angle) with and without the optimiser's corrections.

    python tools/eval_protocol.py --keyframes 48 --height 120 --width 160 --iterations 1500 --camera-optimizer-mode SE3 \\
        --pose-noise 5e-3 5e-3
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402


def _so3_exp(w: torch.Tensor) -> torch.Tensor:
    th = w.norm()
    k = torch.tensor([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=w.dtype)
    if th < 1e-12:
        return torch.eye(3, dtype=w.dtype) + k
    return torch.eye(3, dtype=w.dtype) + torch.sin(th) / th * k + (1 - torch.cos(th)) / th ** 2 * (k @ k)


def _pose_errors(pred: np.ndarray, gt: np.ndarray) -> dict:
    dt = pred[:, :3, 3] - gt[:, :3, 3]
    rr = np.einsum("nij,nkj->nik", pred[:, :3, :3], gt[:, :3, :3])  # R_pred R_gt^T
    ang = np.arccos(np.clip((np.trace(rr, axis1=1, axis2=2) - 1) / 2, -1, 1))
    return {"translation_rmse": float(np.sqrt((dt ** 2).sum(1).mean())), "rotation_mean_rad": float(ang.mean())}


def _gauge_split(pred: np.ndarray, gt: np.ndarray) -> dict:
    """The pose error split into what a common rigid motion of ALL cameras explains (a gauge: the field absorbs it, and
    the protocol's alignment pins it on frame 0 alone) and what is left.  D_i = pred_i gt_i^-1 is camera i's error as a
    world-frame motion; G = their mean (rotation vectors and translations averaged: the errors are ~1e-3); the residual of
    camera i is G^-1 D_i."""
    n = pred.shape[0]
    P4, G4 = np.tile(np.eye(4), (n, 1, 1)), np.tile(np.eye(4), (n, 1, 1))
    P4[:, :3, :4], G4[:, :3, :4] = pred[:, :3, :4], gt[:, :3, :4]
    D = P4 @ np.linalg.inv(G4)

    def log_so3(R):
        ang = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
        w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        return w * (0.5 if ang < 1e-8 else ang / (2 * np.sin(ang)))

    def exp_so3(w):
        th = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        return np.eye(3) + K if th < 1e-8 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)

    w = np.stack([log_so3(D[i, :3, :3]) for i in range(n)])
    Gm = np.eye(4)
    Gm[:3, :3], Gm[:3, 3] = exp_so3(w.mean(0)), D[:, :3, 3].mean(0)
    Res = np.linalg.inv(Gm)[None] @ D
    res_ang = np.array([np.linalg.norm(log_so3(Res[i, :3, :3])) for i in range(n)])
    return {"mean_rigid_rotation_rad": float(np.linalg.norm(w.mean(0))), "mean_rigid_translation": float(np.linalg.norm(Gm[:3, 3])),
            "residual_rotation_mean_rad": float(res_ang.mean()),
            "residual_translation_rmse": float(np.sqrt((Res[:, :3, 3] ** 2).sum(1).mean())),
            "raw_rotation_mean_rad": float(np.linalg.norm(w, axis=1).mean())}


def _log(mapper):
    every = int(os.environ.get("NVO_PROTO_LOG", "0"))
    lo, hi = int(os.environ.get("NVO_PROTO_LOG_FROM", "0")), int(os.environ.get("NVO_PROTO_LOG_TO", "1000000000"))
    if every and mapper.step % every == 0 and lo <= mapper.step <= hi:
        eng = mapper.trainer.pipeline.model.engine
        torch.cuda.synchronize()
        if os.environ.get("NVO_PROTO_LOG_GRADS"):
            bad = {n: int((~torch.isfinite(eng.grads[o:o + sz])).sum()) for n, (o, sz, _) in eng.segments.items()}
            ws = eng._workspace(eng.cfg.num_rays, True)
            extra = {k: int((~torch.isfinite(ws[k].float())).sum()) for k in ("drgb", "dout2", "dout0", "dout1", "out2", "rgb", "weights2", "x2")}
            mx = {n: float(eng.params[o:o + sz].abs().max()) for n, (o, sz, _) in eng.segments.items()}
            gmax = {n: float((eng.grads[o:o + sz] / eng.current_loss_scale()).abs().max()) for n, (o, sz, _) in eng.segments.items() if sz}
            print(f"   max|grad| {gmax}", file=sys.stderr, flush=True)
            pre = ws["out2"][:, 0].float()
            d2 = ws["dout2"].float()
            rows = (~torch.isfinite(d2)).any(dim=1).nonzero().flatten()[:4]
            detail = [(int(r), [float(v) for v in d2[r][:3]], float(pre[r]), float(ws["weights2"][r]),
                       [float(v) for v in ws["tbins2"].view(-1, 49)[r // 48, (r % 48):(r % 48) + 2]]) for r in rows.tolist()]
            print(f"   nonfinite grads {bad} ws {extra} max pre {float(pre.max()):.2f} n(pre>14) {int((pre > 14).sum())} bad rows {detail}", file=sys.stderr, flush=True)
        print(f"it {mapper.step} scale {eng.current_loss_scale()} tracker {int(eng.dev_growth_tracker.item())} flags "
              f"{eng.skip_flag.tolist()} applied {eng.opt_steps} finite {bool(torch.isfinite(eng.params).all())} "
              f"half_finite {bool(torch.isfinite(eng.working_copy_float()).all())} losses {eng.loss_dict()}", file=sys.stderr, flush=True)


def _mesh_nerf_defaults(points, depth, training_pixels):
    """Points and depth of the nerfstudio density mesh where the command line leaves them open.  The reference asks for
    33 554 432 points at depth 9 from some 1e8 training pixels.  The protocol's frames are small: rays are drawn with
    replacement, a pixel drawn 20 times is 20 identical points, whose mean neighbour distance is 0, and the outlier rule
    drops points at 0 -- so at most a quarter of the training pixels; and a lattice whose surface cells hold fewer than
    about four points has densities below the trim's floor -- so at most floor(log4(points / 24)), a cube's 6 * 4^depth
    surface cells.  Both constants, the quarter and the four points per cell, are reasoned, not tuned: each was tried in
    one run of this tool (EXPERIMENTS.md section 19) and nothing else was measured."""
    import math

    if points is None:
        points = min(33554432, max(int(training_pixels) // 4, 1))
    if depth is None:
        depth = max(2, min(9, int(math.floor(math.log(max(points / 24.0, 16.0), 4.0)))))
    return int(points), int(depth)


def run(keyframes=48, height=120, width=160, iterations=1500, frame_stride=2, eval_frames=8, chunk=8, device="cuda:0",
        camera_optimizer_mode=None, pose_noise=None, deterministic=False, seed=42, dynamic_loss_scale=None, out_dir=None,
        quiet=True, keyframe_views=True, method="nerfstudio", scene_scale=None, mesh=False, metrics_3d=False,
        mesh_nerf=False, pointcloud=False, pointcloud_points=33554432, poisson_depth=None, mesh_nerf_points=None,
        mesh_nerf_attributes=False, mesh_volume="dense", metrics_device="cpu", lpips_weights=None):
    """``lpips_weights``: weight files of AlexNet and of the LPIPS linear layers (``nerf_vo_amd.lpips.LPIPS.from_files``);
    with them metrics_2d_*.csv has the reference's ``lpips`` column, without them it is left out as before.
    ``metrics_device``: 'cpu' computes metrics_2d_*.csv on the host, 'cuda' on the GPU (``Evaluator2D(device=...)``,
    nerf_vo_amd/metrics2d.py).  The trajectory table results/metrics_trajectory.csv (run.py:78) is always written: its
    ``keyframes_mapping`` row scores the exported (optimised) keyframe poses, its ``keyframes_tracking`` row the poses as
    ingested, written with the same translation scaling -- the place the reference's tracker output takes.
    ``mesh_volume``: the volume ``render_mesh(source='frames')`` fuses into, 'dense' or 'blocks' (nerf_vo_amd/tsdf.py).
    ``method``: 'nerfstudio' (the default mapper) or 'instant-ngp' (the occupancy-grid back-end through the pyngp facade,
    /root/reference/nerf_vo/mapping/instant_ngp.py + evaluation/nerf_renderer.py:221-320; the room is shrunk by
    ``scene_scale``, default 0.5, so that it lies inside that back-end's scene box: it takes poses as they come).
    ``mesh_nerf``: also ``render_mesh(source='nerf')`` cropped to the ground-truth mesh's box (run.py:72) -- the density
    iso-surface of the occupancy-grid back-end, the Poisson reconstruction (at ``poisson_depth``) of a cloud of
    ``mesh_nerf_points`` points for the nerfstudio back-end; with ``metrics_3d`` the table gains its row.  Their defaults
    are the reference's 33 554 432 points and depth 9 brought down to the protocol's small frames (``_mesh_nerf_defaults``).
    ``mesh_nerf_attributes`` (instant-ngp): the density mesh carries vertex normals and colours (``vertex_attributes``).
    ``pointcloud`` (both back-ends): also ``render_point_cloud(num_points=pointcloud_points)`` -- the oriented, coloured cloud
    of the field, outliers removed, cropped to the ground-truth mesh's box -- and its score, results/metrics_3d_pointcloud.csv."""
    entry.build()
    from nerf_vo_amd.evaluation import (EvaluationRenderer, Evaluator2D, Evaluator3D, EvaluatorTrajectory, read_color,
                                        transform_matrices_pred2gt)

    if metrics_device not in ("cpu", "cuda"):
        raise SystemExit(f"--metrics-device must be cpu or cuda, got {metrics_device!r}")
    from nerf_vo_amd.mapping.dataset import opencv_to_opengl
    from nerf_vo_amd.mapping.nerfstudio_mapper import Nerfstudio
    from nerf_vo_amd.mapping.renderer import NerfstudioRenderer, calculate_psnr_float
    from nerf_vo_amd.synthetic import SyntheticEvaluationDataset

    torch.manual_seed(int(seed))
    dev = torch.device(device)
    own_dir = out_dir is None  # (a directory of our own making is removed again: 1.1 GB of frames and snapshots per run)
    out_dir = out_dir or tempfile.mkdtemp(prefix="nvo_eval_")
    n_frames = keyframes * frame_stride  # dataset frames; every frame_stride-th one is a keyframe (configs: frame_stride 2)
    ngp = method == "instant-ngp"
    if mesh_nerf_attributes and not ngp:
        raise SystemExit("--mesh-nerf-attributes needs --method instant-ngp (the nerfstudio mesh carries its colours already)")
    if ngp and abs(width / height - 1200.0 / 680.0) > 0.01:
        # (the testbed's free camera has ONE focal length, evaluation/nerf_renderer.py:152: Replica's intrinsics have square
        # pixels only at its own aspect -- 160 x 120 renders with fx != fy come out at 13 dB)
        raise SystemExit("--method instant-ngp needs Replica's aspect ratio (e.g. --width 240 --height 136)")
    ds = SyntheticEvaluationDataset(num_frames=n_frames, height=height, width=width, device=dev,
                                    scene_scale=float(scene_scale) if scene_scale else (0.5 if ngp else 1.0),
                                    dir_dataset=out_dir + "/dataset/synthetic_room")
    mesh = mesh or metrics_3d  # the 3-D table is computed from the mesh
    kf = list(range(0, n_frames, frame_stride))
    held_out = [i for i in range(n_frames) if i % frame_stride != 0]
    ds.evaluation_frames = [held_out[int(j * len(held_out) / eval_frames)] for j in range(eval_frames)]
    args = argparse.Namespace(experiment="protocol", dir_prediction=out_dir + "/pred", mapping_snapshot_iterations=iterations,
                              mapping_iterations=iterations, num_keyframes=keyframes, frame_height=height, frame_width=width,
                              enhancement_module="depth", deterministic=deterministic, dynamic_loss_scale=dynamic_loss_scale,
                              camera_optimizer_mode=camera_optimizer_mode)
    if ngp:
        from nerf_vo_amd.mapping.instant_ngp_mapper import InstantNGP, InstantNGPRenderer
        mapper = InstantNGP(args, device=dev)
    else:
        mapper = Nerfstudio(args, device=dev)
    ci = ds.camera_intrinsics
    intr = torch.tensor([ci["fx"], ci["fy"], ci["cx"], ci["cy"]])
    poses = torch.from_numpy(ds.camera_extrinsics[kf]).float()
    if pose_noise is not None:  # tracker-like errors on every pose but the first (which anchors the world)
        g = torch.Generator().manual_seed(int(seed) + 1)
        for i in range(1, keyframes):
            poses[i, :3, :3] = _so3_exp(torch.randn(3, generator=g) * pose_noise[0]) @ poses[i, :3, :3]
            poses[i, :3, 3] += torch.randn(3, generator=g) * pose_noise[1]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    per_kf = max(int(iterations / keyframes), 1)
    for lo in range(0, keyframes, chunk):
        hi = min(keyframes, lo + chunk)
        frames = [ds.render(ds.camera_extrinsics[i]) for i in kf[lo:hi]]
        color = torch.stack([torch.from_numpy(c) for c, _ in frames]).permute(0, 3, 1, 2).float() / 255.0
        depth = torch.stack([torch.from_numpy(d) for _, d in frames])[:, None].float().clamp(0.0, 5.0)
        gl = opencv_to_opengl(poses[lo:hi].to(dev))
        mapper(input={"keyframe_indices": torch.arange(lo, hi), "camera_intrinsics": intr.repeat(hi - lo, 1).to(dev),
                      "camera_extrinsics": gl, "frames_color": color.to(dev),
                      "frames_depth": depth.to(dev), "last_frame": hi == keyframes})
        for _ in range(per_kf * (hi - lo) - 1):
            if mapper.step < iterations:
                mapper(input=None)
                _log(mapper)
    while mapper.step < iterations:
        mapper(input=None)
        _log(mapper)
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    mapper(input=None)
    assert mapper.is_shut_down

    nerf = InstantNGPRenderer(mapping_model=mapper) if ngp else NerfstudioRenderer(mapping_model=mapper)
    renderer = EvaluationRenderer(dataset=ds, nerf=nerf, keyframes=kf, dir_prediction=args.dir_prediction)
    renderer.render_frames(mode="evaluation_frames")
    exported = renderer.export_keyframe_poses()
    mesh_info = None
    if mesh:  # the protocol's last render step (run.py:71): mesh/mesh_from_evaluation_frames.ply
        t_mesh = time.perf_counter()
        file_mesh = renderer.render_mesh(source="frames", mode="evaluation_frames", volume=mesh_volume)
        mesh_info = {"volume": mesh_volume, "file": file_mesh if not own_dir else os.path.basename(file_mesh),
                     "bytes": os.path.getsize(file_mesh),
                     "seconds": time.perf_counter() - t_mesh}
    mesh_nerf_info = None
    if mesh_nerf:  # run.py:72: mesh/mesh_from_nerf_raw.ply and its crop mesh/mesh_from_nerf.ply
        t_mesh = time.perf_counter()
        if ngp:
            file_mesh = renderer.render_mesh(source="nerf", **({"vertex_attributes": True} if mesh_nerf_attributes else {}))
        else:
            mesh_nerf_points, poisson_depth = _mesh_nerf_defaults(mesh_nerf_points, poisson_depth, keyframes * height * width)
            file_mesh = renderer.render_mesh(source="nerf", num_points=mesh_nerf_points, depth=poisson_depth)
        mesh_nerf_info = {"file": file_mesh if not own_dir else os.path.basename(file_mesh), "bytes": os.path.getsize(file_mesh),
                          "seconds": time.perf_counter() - t_mesh}
        if not ngp:
            mesh_nerf_info.update(points_requested=mesh_nerf_points, poisson_depth=poisson_depth)
    cloud_info = None
    if pointcloud:  # the first half of the reference's nerfstudio render_mesh: pointcloud/pointcloud_from_nerf.ply, and its score
        import pandas as pd

        t_cloud = time.perf_counter()
        file_cloud = renderer.render_point_cloud(num_points=int(pointcloud_points))
        seconds_cloud = time.perf_counter() - t_cloud
        t_cloud = time.perf_counter()
        Evaluator3D(ds, args.dir_prediction, out_dir + "/results").calculate_metrics_3d_clouds()
        row = pd.read_csv(out_dir + "/results/metrics_3d_pointcloud.csv").set_index("mesh").loc["pointcloud_from_nerf"]
        cloud_info = {"file": file_cloud if not own_dir else os.path.basename(file_cloud), "bytes": os.path.getsize(file_cloud),
                      "points_requested": int(pointcloud_points), "seconds": seconds_cloud,
                      "metrics_3d": {k: float(v) for k, v in row.items()},
                      "metrics_seconds_incl_ground_truth_mesh": time.perf_counter() - t_cloud}
    m_3d = None
    if metrics_3d:  # run.py:79: ground-truth mesh fused from all ground-truth frames, results/metrics_3d.csv
        import pandas as pd

        t_3d = time.perf_counter()
        Evaluator3D(ds, args.dir_prediction, out_dir + "/results").calculate_metrics_3d()
        seconds_3d = time.perf_counter() - t_3d
        table = pd.read_csv(out_dir + "/results/metrics_3d.csv").set_index("mesh")
        m_3d = {**{k: float(v) for k, v in table.loc["mesh_from_evaluation_frames"].items()},
                "seconds_incl_ground_truth_mesh": seconds_3d}
        if "mesh_from_nerf" in table.index:
            m_3d["mesh_from_nerf"] = {k: float(v) for k, v in table.loc["mesh_from_nerf"].items()}
    # run.py:78: results/metrics_trajectory.csv.  The mapping file is there (export_keyframe_poses); the tracking file holds
    # the poses as ingested, translations scaled like the exported ones (the alignment's own scale absorbs the factor)
    tracked = poses.double().numpy().copy()
    tracked[:, :3, 3] *= renderer.pred2gt_transformation["scale_pred2gt"]
    with open(f"{args.dir_prediction}/matrices/matrices_origin2frame_keyframes_tracking.json", "w") as file:
        json.dump(tracked.tolist(), file)
    EvaluatorTrajectory(ds, kf, args.dir_prediction, out_dir + "/results").calculate_metrics_trajectory()
    import pandas as pd

    m_traj = {row["trajectory"]: {k: float(v) for k, v in row.items() if k != "trajectory"}
              for row in pd.read_csv(out_dir + "/results/metrics_trajectory.csv").to_dict("records")}
    lpips_loss = None
    if lpips_weights:
        from nerf_vo_amd.lpips import LPIPS

        lpips_loss = LPIPS.from_files(*lpips_weights, device=dev)
    ev = Evaluator2D(ds, kf, args.dir_prediction, out_dir + "/results", lpips_loss=lpips_loss,
                     device=None if metrics_device == "cpu" else dev)
    m_eval = ev.calculate_metrics_2d(mode="evaluation_frames")
    m_kf = {}
    if keyframe_views:  # (every keyframe through JPEG / PNG files and the CPU metrics: seconds per hundred frames)
        renderer.render_frames(mode="keyframes")
        m_kf = ev.calculate_metrics_2d(mode="keyframes")
    # conventional (float-MSE) PSNR of the same JPEG files, beside the reference's definition
    cdir = args.dir_prediction + "/evaluation_frames/color"
    files = sorted(f for f in os.listdir(cdir) if f.endswith(".jpg"))
    gts = ds.frames_color(mode="evaluation_frames", keyframes=kf)
    psnr_float = float(np.mean([calculate_psnr_float(read_color(os.path.join(cdir, f)), g) for f, g in zip(files, gts)]))
    # keyframe trajectory in the ground truth's world through the protocol's frame-0 alignment
    t = renderer.pred2gt_transformation
    gt_kf = np.asarray(ds.camera_extrinsics[kf], dtype=np.float64)
    traj = transform_matrices_pred2gt(np.stack([nerf.get_camera_extrinsics(i) for i in range(keyframes)]), t)
    pose_err = _pose_errors(traj, gt_kf)
    # the same for the poses as INGESTED (no camera-optimiser correction): what the optimiser had to improve on
    ing = poses.double().numpy()
    ing = np.asarray(gt_kf[0])[None] @ np.linalg.inv(ing[0])[None] @ ing  # frame-0 anchored, as the protocol does
    eng = mapper.ngp._engine if ngp else mapper.trainer.pipeline.model.engine
    res = {"method": method, "scene_scale": ds.scene_scale, "keyframes": keyframes, "resolution": [width, height], "iterations": iterations, "train_seconds": train_s,
           "camera_optimizer_mode": camera_optimizer_mode or "SE3", "pose_noise": list(pose_noise) if pose_noise else None,
           "scale_pred2gt": float(t["scale_pred2gt"]),
           "evaluation_frames": {**{k: float(v) for k, v in m_eval.items()}, "psnr_float_mse": psnr_float, "frames": len(files)},
           "keyframe_views": {k: float(v) for k, v in m_kf.items()},
           "pose_error_after_frame0_alignment": pose_err, "pose_error_of_ingested_poses": _pose_errors(ing, gt_kf),
           # the same error split into the cameras' common rigid motion (gauge) and the residual
           "pose_error_gauge_split": _gauge_split(traj, gt_kf),
           # results/metrics_trajectory.csv: Kabsch-Umeyama alignment with scale, the reference's six ATE statistics
           "metrics_trajectory": m_traj, "metrics_device": metrics_device,
           "pose_adjustment_rms": float((eng.pose_adjustment if ngp else eng.view("camera_opt.pose_adjustment")).pow(2).mean().sqrt()),
           "deterministic": bool(deterministic), "seed": seed, "exported_poses": int(exported.shape[0])}
    if mesh_info is not None:
        res["mesh"] = mesh_info
    if mesh_nerf_info is not None:
        res["mesh_nerf"] = mesh_nerf_info
    if m_3d is not None:
        res["metrics_3d"] = m_3d
    if cloud_info is not None:
        res["pointcloud"] = cloud_info
    if ngp:
        res.update({"camera_optimizer_mode": "instant-ngp extrinsics", "ms_per_step_incl_ingest": 1e3 * train_s / iterations,
                    "rays_per_batch": eng.rays_per_batch, "applied_steps": eng.applied_steps})
    else:
        res.update({"dynamic_loss_scale": bool(eng.cfg.dynamic_loss_scale), "loss_scale_end": eng.current_loss_scale()})
    if not quiet:
        print(json.dumps(res))
    if own_dir:
        import shutil
        shutil.rmtree(out_dir, ignore_errors=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=48)
    ap.add_argument("--height", type=int, default=120)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--iterations", type=int, default=1500)
    ap.add_argument("--eval-frames", type=int, default=8)
    ap.add_argument("--camera-optimizer-mode", default=None, help="SE3 (default) | SO3xR3 | off")
    ap.add_argument("--pose-noise", type=float, nargs=2, default=None, metavar=("SIGMA_ROT", "SIGMA_TRANS"))
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--static-loss-scale", action="store_true", help="tcnn's static 128 instead of GradScaler's dynamics")
    ap.add_argument("--no-keyframe-views", action="store_true")
    ap.add_argument("--method", default="nerfstudio", choices=["nerfstudio", "instant-ngp"])
    ap.add_argument("--scene-scale", type=float, default=None)
    ap.add_argument("--mesh", action="store_true", help="also fuse the rendered evaluation frames into mesh/mesh_from_evaluation_frames.ply")
    ap.add_argument("--mesh-volume", default="dense", choices=["dense", "blocks"], help="--mesh: fuse into the dense volume or "
                    "into the block-sparse one (the reference's VoxelBlockGrid shape)")
    ap.add_argument("--metrics-3d", action="store_true", help="also score the mesh against the fused ground-truth mesh "
                    "(results/metrics_3d.csv); implies --mesh")
    ap.add_argument("--mesh-nerf", action="store_true", help="also the mesh of the field itself, cropped to the ground-truth mesh's "
                    "box (mesh/mesh_from_nerf.ply): the density iso-surface (instant-ngp) or the Poisson reconstruction of the "
                    "oriented point cloud (nerfstudio); with --metrics-3d the table gains its row")
    ap.add_argument("--poisson-depth", type=int, default=None, help="nerfstudio --mesh-nerf: depth of the Poisson lattice (2..10); "
                    "default: the reference's 9, lowered until a surface cell holds about four points")
    ap.add_argument("--mesh-nerf-points", type=int, default=None, help="nerfstudio --mesh-nerf: points of the cloud before "
                    "outlier removal; default: the reference's 33554432, at most a quarter of the training pixels")
    ap.add_argument("--mesh-nerf-attributes", action="store_true", help="instant-ngp --mesh-nerf: the density mesh carries "
                    "vertex normals (negated density gradient) and colours")
    ap.add_argument("--pointcloud", action="store_true", help="also export the field's oriented point cloud, "
                    "cropped to the ground-truth mesh's box (pointcloud/pointcloud_from_nerf.ply), and score it "
                    "(results/metrics_3d_pointcloud.csv)")
    ap.add_argument("--pointcloud-points", type=int, default=33554432, help="points of the cloud before outlier removal and crop")
    ap.add_argument("--metrics-device", default="cpu", choices=["cpu", "cuda"], help="where metrics_2d_*.csv is computed: the host "
                    "functions, or the HIP kernels of nerf_vo_amd/metrics2d.py on batches of uploaded frames")
    ap.add_argument("--lpips-weights", nargs="+", default=None, metavar="FILE", help="AlexNet's and the LPIPS linear layers' weight "
                    "files (one or two .pth state dicts; never fetched): adds the lpips column to metrics_2d_*.csv")
    a = ap.parse_args()
    run(a.keyframes, a.height, a.width, a.iterations, eval_frames=a.eval_frames, camera_optimizer_mode=a.camera_optimizer_mode,
        pose_noise=a.pose_noise, deterministic=a.deterministic, seed=a.seed, quiet=False,
        dynamic_loss_scale=False if a.static_loss_scale else None, keyframe_views=not a.no_keyframe_views,
        method=a.method, scene_scale=a.scene_scale, mesh=a.mesh, metrics_3d=a.metrics_3d, mesh_nerf=a.mesh_nerf,
        pointcloud=a.pointcloud, pointcloud_points=a.pointcloud_points, poisson_depth=a.poisson_depth,
        mesh_nerf_points=a.mesh_nerf_points, mesh_nerf_attributes=a.mesh_nerf_attributes, mesh_volume=a.mesh_volume,
        metrics_device=a.metrics_device, lpips_weights=a.lpips_weights)
