"""neb_gi_set_skin, neb_gi_skin_vertices, neb_gi_download_vertices: what holds without a GPU -- the reference of the written order
(tests/skin_ref.py) against float64 linear-blend skinning, the exports, the ctypes mirrors of the two structs, the null-context answers."""
import ctypes as C
import os
import subprocess

import numpy as np

import skin_ref
from nebulae_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("neb_gi_set_skin", "neb_gi_skin_vertices", "neb_gi_download_vertices")
F = np.float32
EPS = float(np.finfo(np.float32).eps)


def _random_case(n=100_000, n_joints=6, seed=5):
    rng = np.random.default_rng(seed)
    P = rng.uniform(-40.0, 40.0, (n, 3)).astype(F)
    N = rng.normal(size=(n, 3))
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(F)
    T = np.concatenate([np.roll(N, 1, axis=1), np.where(rng.random((n, 1)) < 0.5, -1.0, 1.0)], axis=1).astype(F)
    joints = rng.integers(0, n_joints, (n, 4)).astype(np.uint16)
    w = rng.random((n, 4))
    w[:, 3] = 0.0  # (three influences and a fourth of weight zero, as the hat skins have)
    w = (w / w.sum(1, keepdims=True)).astype(F)
    J = np.zeros((n_joints, 4, 4))
    for j in range(n_joints):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        J[j, :3, :3] = q
        J[j, 3, :3] = rng.uniform(-300.0, 300.0, 3)
        J[j, 3, 3] = 1.0
    return P, N, T, joints, w, J.astype(F)


def test_the_written_order_stays_float32_and_is_within_eight_roundings_of_float64_skinning():
    """Bound per component: 4 FLT_EPSILON sum|terms| = 8 unit roundoffs -- any path through the expression crosses eight roundings (the
    product w J, three sums of S, the product p S, three sums of the bake; the normals' paths are shorter).
    sum|terms| = sum_i |w_i| (|p| |J_i| column + |t_i|)."""
    P, N, T, joints, w, J = _random_case()
    got = skin_ref.skin(P, N, T, joints, w, J)
    for key, width in (("positions", 3), ("normals", 3), ("tangents", 4)):
        assert got[key].dtype == np.float32 and got[key].shape == (P.shape[0], width), key
    assert skin_ref.blended(joints, w, J).dtype == np.float32
    j64, w64 = J.astype(np.float64), w.astype(np.float64)
    jn = joints.astype(np.int64)
    worst = {}
    for key, V, translate in (("positions", P, True), ("normals", N, False), ("tangents", T[:, :3], False)):
        V64 = V.astype(np.float64)
        want, mag = np.zeros((P.shape[0], 3)), np.zeros((P.shape[0], 3))
        for i in range(4):
            Ji = j64[jn[:, i]]
            term = np.einsum("nr,nrc->nc", V64, Ji[:, :3, :3]) + (Ji[:, 3, :3] if translate else 0.0)
            want += w64[:, i, None] * term
            mag += np.abs(w64[:, i, None]) * (np.einsum("nr,nrc->nc", np.abs(V64), np.abs(Ji[:, :3, :3])) + (np.abs(Ji[:, 3, :3]) if translate else 0.0))
        err = np.abs(got[key][:, :3].astype(np.float64) - want)
        worst[key] = float((err / mag).max() / EPS)
        assert (err <= 4.0 * EPS * mag).all(), (key, worst[key])
    print(f"[skin_ref] worst error in units of FLT_EPSILON sum|terms|: {worst}")
    assert np.array_equal(got["tangents"][:, 3], T[:, 3])  # (.w copied)


def test_identity_matrices_and_unit_weights_return_the_input_bits():
    P, N, T, _, _, _ = _random_case(n=1000)
    joints, w = skin_ref.identity_skin(P.shape[0])
    got = skin_ref.skin(P, N, T, joints, w, skin_ref.identity_pose(3))
    for key, a in (("positions", P), ("normals", N), ("tangents", T)):
        assert np.array_equal(got[key].view(np.uint32), a.view(np.uint32)), key


def test_hat_skins_and_poses_are_what_the_gpu_tests_assume():
    rng = np.random.default_rng(2)
    P = rng.uniform(-1.0, 1.0, (500, 3)) * (0.04, 1.9, 0.04)
    for nj, fourth in ((2, "split"), (3, "zero"), (3, "split"), (4, "zero"), (6, "zero")):
        joints, w = skin_ref.hat_skin(P, nj, fourth=fourth, spare=nj - 1)
        assert joints.dtype == np.uint16 and joints.max() < nj and w.dtype == np.float32
        assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() < 4 * EPS and w.min() >= 0.0
        nonzero = (w > 1e-3).sum(1)
        if nj >= 4:  # four distinct joints, four weights that matter, on every vertex
            assert (nonzero == 4).all() and all(len(set(row)) == 4 for row in joints[:50].tolist())
        elif fourth == "zero":  # three influences at most, the fourth zero on an arbitrary valid joint
            assert (w[:, 3] == 0).all() and (joints[:, 3] == nj - 1).all() and (nonzero == 3).all()
            assert all(len(set(row[:3])) == 3 for row in joints[:50].tolist())
        else:  # every slot non-zero somewhere, the fourth on two vertices of three
            assert (w[:, :3] > 1e-3).all() and 0.6 < (w[:, 3] > 1e-3).mean() < 0.7 and (w[::3, 3] == 0).all()
        assert ((w > 0.05) & (w < 0.95)).any()  # (fractional weights: the blend is exercised)
        M = skin_ref.pose(P, nj, k=1)
        assert M.shape == (nj, 4, 4) and M.dtype == np.float32
        for m in M.astype(np.float64):
            ang = float(np.degrees(np.arccos(np.clip((np.trace(m[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))))
            assert 10.0 - 1e-3 <= ang <= 25.0 + 1e-3, ang
            assert np.abs(m[:3, :3] @ m[:3, :3].T - np.eye(3)).max() < 1e-6


def test_the_library_exports_the_three_calls_and_the_binding_declares_them():
    build.build()
    raw = C.CDLL(build.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.exported_symbols(), name
    sigs = _lib._gi_sigs()
    assert sigs["neb_gi_set_skin"] == (C.c_int, [C.c_void_p, C.POINTER(_lib.SkinDesc), C.c_uint32, C.c_void_p])
    assert sigs["neb_gi_skin_vertices"] == (C.c_int, [C.c_void_p, C.POINTER(_lib.SkinUpdate), C.c_uint32, C.c_void_p])
    assert sigs["neb_gi_download_vertices"][1][1:4] == [C.c_uint32] * 3 and len(sigs["neb_gi_download_vertices"][1]) == 8
    mirror = open(os.path.join(ROOT, "include", "nebulae_hip.hpp")).read()
    for name in NAMES:
        assert name in mirror, name


def test_the_ctypes_structs_have_the_sizes_and_offsets_of_the_header(tmp_path):
    fields = {"neb_skin_desc": ("geometry", "numJoints", "joints", "jointStride", "weights", "weightStride"),
              "neb_skin_update": ("geometry", "jointMatrices")}
    lines = "".join(f'  printf("{s} %zu", sizeof({s}));' + "".join(f' printf(" %zu", offsetof({s}, {f}));' for f in fs) + ' printf("\\n");\n'
                    for s, fs in fields.items())
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nebulae_hip.h"\nint main(void) {\n' + lines + "  return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    for line, (s, fs), T in zip(out, fields.items(), (_lib.SkinDesc, _lib.SkinUpdate)):
        words = line.split()
        assert words[0] == s
        assert int(words[1]) == C.sizeof(T), (s, words[1], C.sizeof(T))
        assert [int(x) for x in words[2:]] == [getattr(T, f).offset for f in fs], s
        assert [n for n, _ in T._fields_] == list(fs), s


def test_a_null_context_is_refused_before_anything_else_is_looked_at():
    lib = _lib.load()
    d = _lib.SkinDesc(geometry=0, numJoints=1, joints=16, jointStride=8, weights=16, weightStride=16)  # (never dereferenced)
    u = _lib.SkinUpdate(geometry=0)
    p = (C.c_float * 3)()
    assert lib.neb_gi_set_skin(None, C.byref(d), 1, None) == -1
    assert lib.neb_gi_set_skin(None, None, 0, None) == -1
    assert lib.neb_gi_skin_vertices(None, C.byref(u), 1, None) == -1
    assert lib.neb_gi_skin_vertices(None, None, 0, None) == -1
    assert lib.neb_gi_download_vertices(None, 0, 0, 1, p, None, None, None) == -1
