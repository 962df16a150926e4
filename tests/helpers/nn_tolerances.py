"""What the float32 distance rule alone changes, measured on the CPU: the helper run with the kernel's float32 rule
against the helper in float64, for the ICP scene (largest difference of a transform entry) and for the metrics of the
room meshes.  tests/test_metrics3d_gpu.py takes its bounds from these figures.   python tests/helpers/nn_tolerances.py"""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [TESTS, os.path.dirname(TESTS)]

from helpers import nn_oracle  # noqa: E402
from helpers.nn_cases import icp_scene, room_meshes  # noqa: E402


def main():
    from nerf_vo_amd.evaluation import sample_metric_clouds

    source, target = icp_scene()
    t64 = nn_oracle.icp(source, target)
    t32 = nn_oracle.icp(source, target, fp32_distance_rule=True)
    print("icp: iterations", t64[3], t32[3], "max |T_fp32rule - T_f64|", np.abs(t64[0] - t32[0]).max())
    mesh_gt, mesh_pred = room_meshes()
    gt, pred = (c.numpy() for c in sample_metric_clouds(mesh_gt, mesh_pred, seed=0, device="cpu"))
    m64 = nn_oracle.metrics_from_clouds(gt, pred)
    m32 = nn_oracle.metrics_from_clouds(gt, pred, fp32_distance_rule=True)
    print("clouds", gt.shape, pred.shape, "float64", m64)
    print("metrics |fp32rule - f64|", {k: abs(m64[k] - m32[k]) for k in m64})


if __name__ == "__main__":
    main()
