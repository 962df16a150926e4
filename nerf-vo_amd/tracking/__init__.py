"""Tracking: the dense bundle adjustment of the DROID front-end.  The update network, the
correlation volumes and keyframe management are not built."""
from .dense_ba import DenseWindow, depth_covariance, reduced_camera_matrix, reproject, solve, solve_depth  # noqa: F401
