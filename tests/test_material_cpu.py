"""Materials and texels updated in place: what holds without a GPU.

The device keeps no images, only footprint tables and material bundles, so a texel update is a PATCH of those tables.  The arithmetic of
the patch lives in nebulae_amd/csrc/texture_patch.h, which texture_patch_kernel compiles unchanged; here g++ compiles it through
tools/texture_patch_proto.cpp and it is held to the one property that matters: the tables of the old image, patched, equal the tables built
from the edited image (texture_tables_ref.py), byte for byte -- standalone, each role of a bundle, two roles of one bundle, two bundles."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import texture_tables_ref as T
from nebulae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("neb_gi_update_materials", "neb_gi_set_geometry_materials", "neb_gi_update_textures", "neb_gi_update_textures_device",
         "neb_gi_debug_texture_tables")
SIZES = [(1, 1), (1, 8), (8, 1), (2, 2), (16, 16), (8, 4), (67, 5)]  # (w, h)


def rectangles(w, h):
    """lists of (x, y, rw, rh) applied in order; the last list holds two overlapping rectangles"""
    return {"whole": [(0, 0, w, h)],
            "first texel (wraps to the last column and row of entries)": [(0, 0, 1, 1)],
            "last texel": [(w - 1, h - 1, 1, 1)],
            "full-width band": [(0, h // 2, w, max(1, h // 3))],
            "full-height band": [(w // 2, 0, max(1, w // 3), h)],
            "interior": [(min(1, w - 1), min(1, h - 1), max(1, w - 2), max(1, h - 2))],
            "touching right and bottom": [(w // 2, h // 2, w - w // 2, h - h // 2)],
            "two overlapping, in order": [(0, 0, max(1, (2 * w) // 3), max(1, (2 * h) // 3)), (w // 3, h // 3, w - w // 3, h - h // 3)]}


@pytest.fixture(scope="module")
def proto(tmp_path_factory):
    so = tmp_path_factory.mktemp("texpatch") / "libtexture_patch_proto.so"
    subprocess.check_call(["g++", "-O2", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "nebulae_amd", "csrc"),
                           os.path.join(ROOT, "tools", "texture_patch_proto.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    u32 = C.c_uint32
    lib.tp_patch_table.restype = lib.tp_patch_bundle.restype = C.c_long
    lib.tp_patch_table.argtypes = [u32] * 6 + [C.c_void_p, u32, C.c_void_p]
    lib.tp_patch_bundle.argtypes = [u32] * 6 + [C.c_void_p, u32, u32, C.c_void_p]
    return lib


def _image(rng, w, h):
    return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


def _source(rng, rw, rh, pad):
    """rh rows of rw texels inside rows of rw + pad: a pitch that is not tight"""
    full = rng.integers(0, 256, (rh, rw + pad, 4), dtype=np.uint8)
    return full, full[:, :rw]


@pytest.mark.parametrize("w,h", SIZES)
def test_patched_tables_equal_the_tables_of_the_edited_image(proto, w, h):
    rng = np.random.default_rng(1000 * w + h)
    checked = 0
    for what, rects in rectangles(w, h).items():
        imgs = [_image(rng, w, h) for _ in range(4)]  # albedo, normal, rm of one material; a second material's albedo
        # the uses of the texture being edited: (which of imgs it is, [(bundle maps, role mask)])
        #   standalone + one role of one bundle, each of the three; two roles of one bundle; two bundles
        for edited, bundles in ((0, [((0, 1, 2), T.ROLE_ALBEDO)]), (1, [((0, 1, 2), T.ROLE_NORMAL)]), (2, [((0, 1, 2), T.ROLE_RM)]),
                                (0, [((0, 0, 2), T.ROLE_ALBEDO | T.ROLE_NORMAL)]), (2, [((0, 1, 2), T.ROLE_RM), ((3, 1, 2), T.ROLE_RM)])):
            cur = [im.copy() for im in imgs]
            table = T.footprints(cur[edited]).copy()
            packed = [T.bundle(*(cur[k] for k in maps)).copy() for maps, _ in bundles]
            for (x, y, rw, rh) in rects:
                full, view = _source(rng, rw, rh, pad=3)
                args = (w, h, x, y, rw, rh, full.ctypes.data, full.strides[0])
                n_aff = min(rw + 1, w) * min(rh + 1, h)
                assert proto.tp_patch_table(*args, table.ctypes.data) == n_aff, what
                for (maps, roles), b in zip(bundles, packed):
                    assert proto.tp_patch_bundle(*args, roles, b.ctypes.data) == n_aff, what
                cur[edited][y:y + rh, x:x + rw] = view
            assert np.array_equal(table, T.footprints(cur[edited])), (what, "standalone")
            for (maps, roles), b in zip(bundles, packed):
                assert np.array_equal(b, T.bundle(*(cur[k] for k in maps))), (what, maps, roles)
            checked += 1
    assert checked == 8 * 5


def test_the_prototype_refuses_what_the_library_refuses(proto):
    table = np.zeros((16, 4), np.uint32)
    src = np.zeros((4, 4, 4), np.uint8)
    for x, y, rw, rh, pitch in ((0, 0, 0, 1, 16), (0, 0, 1, 0, 16), (4, 0, 1, 1, 16), (3, 0, 2, 1, 16), (0, 3, 1, 2, 16), (0, 0, 2, 2, 4), (0, 0, 2, 2, 10)):
        assert proto.tp_patch_table(4, 4, x, y, rw, rh, src.ctypes.data, pitch, table.ctypes.data) == -1
    assert not table.any()


def test_the_reference_layout_follows_the_bundling_rule():
    tex = [np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((2, 8, 4), np.uint8)]
    mats = [(0, 1, 2), (0, -1, -1), (3, 1, 2), (0, 1, 9), (2, 2, 2)]
    bundled, standalone = T.layout(mats, tex)
    assert bundled == {0: 0, 4: 16}             # all three maps, one size; the same map three times still bundles
    assert standalone == {0: 0, 1: 16, 2: 32, 3: 48}  # material 1's albedo, material 2's three (sizes differ), material 3's two (index 9 is no map)
    u = T.uses(mats, tex)
    assert u[2] == (True, [(0, T.ROLE_RM), (4, T.ROLE_ALBEDO | T.ROLE_NORMAL | T.ROLE_RM)])


def test_the_header_declares_the_calls_and_the_mirror_has_them():
    text = open(os.path.join(ROOT, "include", "nebulae_hip.h")).read()
    mirror = open(os.path.join(ROOT, "include", "nebulae_hip.hpp")).read()
    for name in NAMES:
        assert f"int {name}(neb_ctx* ctx" in text, name
        assert name in mirror, name
    assert "typedef struct neb_texture_update" in text


def test_the_library_exports_the_entry_points_and_they_refuse_a_null_context():
    exported = _lib.exported_symbols()
    lib = _lib.load()
    for name in NAMES:
        assert name in exported and hasattr(lib, name), name
    idx = (C.c_uint32 * 1)(0)
    mat = (C.c_int32 * 1)(0)
    from nebulae_amd import scene as S
    md = (S.MaterialDesc * 1)()
    px = (C.c_uint8 * 4)()
    tu = _lib.TextureUpdate(texture=0, x=0, y=0, width=1, height=1, pitchBytes=4, rgba8=C.addressof(px))
    n = C.c_size_t(0)
    assert lib.neb_gi_update_materials(None, idx, md, 1, None) == -1
    assert lib.neb_gi_update_materials(None, None, None, 0, None) == -1
    assert lib.neb_gi_set_geometry_materials(None, idx, mat, 1, None) == -1
    assert lib.neb_gi_update_textures(None, C.byref(tu), 1, None) == -1
    assert lib.neb_gi_update_textures_device(None, C.byref(tu), 1, None) == -1
    assert lib.neb_gi_debug_texture_tables(None, None, 0, C.byref(n), None) == -1
