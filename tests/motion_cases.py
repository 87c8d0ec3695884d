"""Scenes, cameras and moves shared by the CPU and GPU tests of option svgf_motion (tests/test_motion_cpu.py computes on the CPU
oracle's G-buffers, for the same cases, what tests/test_motion_gpu.py asks of the device).  TEST INFRASTRUCTURE, NOT PRODUCT CODE."""
import numpy as np

from test_reproject_cpu import moved as moved_camera

W, H = 256, 192
BOXES = [1, 2]  # cornell_parts: the short and the tall box


def small_transform(kind):
    """test_refit_gpu.world_transform scaled down to a few pixels at 256 x 192: translate and scale go 15 % of the way from the
    identity (about 2 px / 3 % .. 5 % in size), rotate is the helper's own smallest step (k = -3: 2 degrees)."""
    from test_refit_gpu import world_transform
    if kind == "rotate":
        return world_transform("rotate", -3)
    return np.eye(4) + 0.15 * (world_transform(kind) - np.eye(4))


# (kind of move, camera move between the two frames or None for a static camera)
CORNELL_CASES = [(kind, cam) for kind in ("translate", "rotate", "scale") for cam in (None, dict(pan=(0.04, 0.0, 0.0), yaw_deg=-0.4))]


def cameras(cam_move):
    from test_refit_gpu import cornell_camera
    prev = cornell_camera()
    return prev, (prev if cam_move is None else moved_camera(prev, **cam_move))
