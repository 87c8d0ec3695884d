"""Scenes, cameras and deformations shared by the CPU and GPU tests of option svgf_vertex_motion (tests/test_vertex_motion_cpu.py checks
on reference-made G-buffers, for the same cases, the conditions tests/test_vertex_motion_gpu.py relies on).
TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Two scenes.  The Cornell parts at 256 x 192 with the short box twisted 2 degrees about its vertical axis and sheared 6 mm over its
height per frame (test_deform_gpu.twist_and_shear): about 1.5 px at its top edge.  The beamed room of views_ref at the 64 x 48 of
test_update_views_gpu with views_ref.RUG_SINE on its floor patch along the normal, from one phase to the opposite one: 2.4 cm at the
crests, all the patch's two centimetres of clearance above the floor allow -- about a pixel at this size from room_camera().
"""
import math

import numpy as np

import views_ref as V
from motion_cases import H, W
from test_deform_gpu import sine_along_normal, twist_and_shear, with_arrays
from test_refit_gpu import cornell_camera, cornell_parts
from test_reproject_cpu import moved as moved_camera

SHORT_BOX = 1
CAMERA_MOVE = dict(pan=(0.04, 0.0, 0.0), yaw_deg=-0.4)  # motion_cases' moving camera
TWIST = dict(angle_deg=2.0, shear=0.01)


def twisted(sc, k=1):
    """the short box of `sc` after k steps of the twist, from the pose it has in `sc` -> the arrays of update_vertices"""
    return twist_and_shear(sc, SHORT_BOX, angle_deg=TWIST["angle_deg"] * k, shear=TWIST["shear"] * k)


def cornell_case(textured=True):
    """-> (scene at the previous frame, {geometry: arrays} of the deformation, the scene then, W, H)"""
    sc0 = cornell_parts(textured=textured)
    deform = {SHORT_BOX: twisted(sc0)}
    return sc0, deform, with_arrays(sc0, deform), W, H


# The phase of the patch's sine.  Where the two poses cross, a pixel's point does not move, and with a static camera its tap position
# is an integer to within rounding: of six phases tried on the reference alone (0.3 .. 2.8 in steps of 0.5) this one leaves one such
# pixel in either camera case; RUG_SINE's own 0.3 leaves three of the 3 072, which is all the 0.1 % cap allows.
ROOM_PHASE = 1.3


def room_case():
    """the beamed room with the sine already on its patch at the previous frame, and the opposite phase at this one"""
    rest = V.beamed_room()
    sc0 = with_arrays(rest, {V.RUG: sine_along_normal(rest, V.RUG, **dict(V.RUG_SINE, phase=ROOM_PHASE))})
    deform = {V.RUG: sine_along_normal(rest, V.RUG, **dict(V.RUG_SINE, phase=ROOM_PHASE + math.pi))}
    return sc0, deform, with_arrays(sc0, deform), V.VW, V.VH


SCENES = {"cornell": cornell_case, "room": room_case}
# (scene, camera move between the two frames or None)
CASES = [(name, cam) for name in SCENES for cam in (None, CAMERA_MOVE)]
CASE_IDS = [f"{name}-{'pan' if cam else 'static'}" for name, cam in CASES]


def room_camera():
    """Looks down on the patch from the room's open front, rolled: the patch moves along the vertical, and under an upright camera a
    vertical step leaves the column of every pixel near the middle of the image unchanged -- tap positions within 1e-4 of an integer
    by construction, which is the one thing the comparison has to leave out."""
    return V.look((-0.25, 0.35, -0.15), (0.1, -0.98, -1.2), up=(0.35, 1.0, 0.1))


def cameras(name, cam_move):
    prev = room_camera() if name == "room" else cornell_camera()
    return prev, (prev if cam_move is None else moved_camera(prev, **cam_move))


def matrices(sc):
    return np.stack([g["M"] for g in sc.geometries])
