"""CPU check of a sun table KEPT across scene updates: lit::box_may_shadow of nebulae_amd/csrc/lit_predicate.h, plain C++ a kernel can
compile unchanged, here compiled by g++ through tools/lit_keep_proto.cpp.  Flags are made for pose A (tools/lit_proto.cpp), five submeshes
move, the predicate clears what their new world boxes can have invalidated and the moved submeshes' own bits; the criterion is
test_sun_table_cpu's: no shadow ray the ORACLE traces in the moved scene from a side still called lit is occluded.
(The predicate only: the library still drops the table on every update)"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from nebulae_amd import scene as S
from oracle_lib import OracleTracer
from test_sun_table_cpu import _world_triangles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def proto(tmp_path_factory):
    so = tmp_path_factory.mktemp("litkeep") / "liblit_keep_proto.so"
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if os.environ.get("NEB_ORACLE_SAN") else []  # tools/run_sanitized.sh
    subprocess.check_call(["g++", "-O2", "-fopenmp", "-shared", "-fPIC"] + san + ["-I", os.path.join(ROOT, "nebulae_amd", "csrc"),
                           os.path.join(ROOT, "tools", "lit_proto.cpp"), os.path.join(ROOT, "tools", "lit_keep_proto.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.lit_keep_apply.restype = C.c_int
    return lib


# The 60-submesh atrium: 0 floor, 1-4 gallery floors, 5-8 their undersides, 9-12 roofs, 13-16 walls, 17-40 ground-storey columns round the
# open court (0 .. 4.3 units high), 41-59 upper-storey columns.  Two updates, world-space translations:
#   first: column 21 up under the gallery roof, column 24 across the floor into the sunlit court, column 30 straight up OUT of the scene box
#          (top at 16.8 units: still within the +-17.4 where the certificate's slack is its floor, so the margin does not grow), upper column 43
#          along its gallery, the gallery underside 7 lowered;
#   second: column 30 back INTO the box, to another place in the court.
UPDATES = [{21: (0.0, 6.5, -2.0), 24: (0.0, 0.0, -4.5), 30: (0.0, 12.5, 0.0), 43: (0.8, 0.0, 0.0), 7: (0.0, -0.6, 0.0)},
           {30: (1.0, 0.0, 3.0)}]


# the first three (sun, diameter, shift) rows of test_sun_table_cpu
@pytest.mark.parametrize("sun,diameter,shift", [((0.5, -1.0, -0.2), 0.58, (0.0, 0.0, 0.0)), ((-0.3, -1.0, 0.4), 3.0, (0.0, 0.0, 0.0)),
                                                ((0.5, -1.0, -0.2), 0.58, (150.0, 40.0, -90.0))])
def test_no_ray_from_a_side_kept_lit_through_two_updates_is_occluded_in_the_oracle(proto, sun, diameter, shift):
    sc = S.moved_scene(S.atrium_standin(target_triangles=30000, n_submeshes=60, tex_size=16), 1.0, shift)  # (a copy: its matrices are its own)
    cam = S.moved_camera(S.sponza_camera(), 1.0, shift)
    W, H = 240, 136
    V, N, first = _world_triangles(sc)
    n = len(V)
    counts = np.diff(np.append(first, n))
    consts = S.default_constants(frame_index=3)
    consts.cameraWorldPos[:] = tuple(cam.eye)
    consts.sunLightDirection[:] = sun
    consts.sunTanHalfAngle = math.tan(math.radians(diameter * 0.5))
    sd = np.array(sun, np.float32)
    flags = np.zeros(n, np.uint8)
    proto.lit_proto_flags(n, V.ctypes.data_as(C.c_void_p), N.ctypes.data_as(C.c_void_p), sd.ctypes.data_as(C.c_void_p), C.c_float(consts.sunTanHalfAngle),
                          flags.ctypes.data_as(C.c_void_p), None)
    built_abs_max = float(np.abs(V).max())
    lit_a = int((flags & 1).sum() + (flags >> 1).sum())
    cleared_own = cleared_box = 0
    for moves in UPDATES:
        moved = np.zeros(n, np.uint8)
        boxes = []
        for gi, d in moves.items():
            sc.geometries[gi]["M"][3, :3] += np.asarray(d, np.float32)
        V, N, _ = _world_triangles(sc)
        for gi in moves:
            tri = slice(first[gi], first[gi] + counts[gi])
            moved[tri] = 1
            boxes.append(np.concatenate([V[tri].reshape(-1, 3).min(axis=0), V[tri].reshape(-1, 3).max(axis=0)]))
        boxes = np.ascontiguousarray(np.array(boxes, np.float32))
        stats = np.zeros(4, np.float64)
        grew = proto.lit_keep_apply(n, V.ctypes.data_as(C.c_void_p), N.ctypes.data_as(C.c_void_p), sd.ctypes.data_as(C.c_void_p), C.c_float(consts.sunTanHalfAngle),
                                    C.c_double(built_abs_max), flags.ctypes.data_as(C.c_void_p), len(boxes), boxes.ctypes.data_as(C.c_void_p),
                                    moved.ctypes.data_as(C.c_void_p), stats.ctypes.data_as(C.c_void_p))
        assert grew == 0, "the moves were chosen not to enlarge the certificate's margin"
        cleared_own += int(stats[1])
        cleared_box += int(stats[2])
    lit_b = int((flags & 1).sum() + (flags >> 1).sum())
    # the reference alone: the moves clear bits of sides that did not move, and leave others standing
    assert cleared_box > 0 and lit_b > 0 and lit_a - lit_b == cleared_own + cleared_box, (lit_a, lit_b, cleared_own, cleared_box)
    o = OracleTracer(sc)
    gb = o.gbuffer(W, H, cam)
    _, hits, _ = o.gi(gb, consts)
    hit = hits["t"] > 0
    tri = np.where(hit, first[np.minimum(hits["geometry"], len(first) - 1)] + hits["primitive"], 0)
    L = -sd.astype(np.float64) / np.linalg.norm(sd)
    nl = N[tri].astype(np.float64) @ L
    margin = consts.sunTanHalfAngle + 0.01
    plus, minus = (nl > margin).all(axis=2), (nl < -margin).all(axis=2)
    lit = (np.where(plus, flags[tri] & 1, (flags[tri] >> 1) & 1).astype(bool) & (plus | minus) | (flags[tri] == 3)) & hit
    visible = (hits["flags"] & 1).astype(bool) & hit
    assert not (lit & ~visible).any(), f"{int((lit & ~visible).sum())} rays from a (triangle, side) kept lit through the updates are occluded in the oracle's trace"
    print(f"[+ {shift}, disk {diameter}] sides lit {lit_a} -> {lit_b} after two updates ({cleared_own} on moved submeshes, {cleared_box} under their boxes): "
          f"{lit_b / max(lit_a, 1):.3f} survive; kept-lit rays {int((lit & visible).sum())} of {int(visible.sum())} unoccluded")
    o.close()
