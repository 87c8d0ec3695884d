"""CPU tests of albedo demodulation (option svgf_demodulate): what the headers declare, and the numpy helper (tests/demod_ref.py) the GPU
tests compare against -- its decode, the floor's exact round trip, and the filter seeing a constant under a checker albedo."""
import os
import re

import numpy as np

import demod_ref as D
from oracle import gi_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_plane_and_option_are_declared_and_mirrored():
    text = open(os.path.join(ROOT, "include", "nebulae_hip.h")).read()
    assert "#define NEB_PLANE_DEMOD 14" in text and "NEB_PLANE_COUNT = 12" in text
    assert '"svgf_demodulate"' in text and "neb_svgf_reset_history" in text
    assert "SetAlbedoDemodulation" in open(os.path.join(ROOT, "include", "nebulae_hip.hpp")).read()
    from nebulae_amd import _lib
    from nebulae_amd.renderer import DeferredRenderer
    from nebulae_amd.svgf import PLANE_DEMOD, PLANE_LAYOUT
    assert _lib.PLANE_DEMOD == 14 and PLANE_DEMOD == 14 and PLANE_LAYOUT[PLANE_DEMOD] == (np.float32, 4)
    assert DeferredRenderer().albedo_demodulation is False


def test_the_floor_comes_from_the_one_header():
    assert D.FLOOR == F(1.0 / 32.0)
    hits = []
    for folder in ("nebulae_amd", "include", "tests"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, folder)):
            for f in files:
                if f.endswith((".h", ".hpp", ".hip", ".py")) and re.search(r"kDemodFloor\s*=", open(os.path.join(dirpath, f), errors="ignore").read()):
                    hits.append(f)
    assert hits == ["svgf_demod.h"], hits


def test_decode_equals_the_oracles_on_every_field_value():
    r = np.arange(1 << 11, dtype=np.uint32)
    b = np.arange(1 << 10, dtype=np.uint32)
    for words in (r, r << np.uint32(11), b << np.uint32(22)):
        got, want = D.decode_r11g11b10(words), gi_np.unpack_r11g11b10(words)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) or np.array_equal(np.nan_to_num(got, nan=-1.0), np.nan_to_num(want, nan=-1.0))
    # ... and the device's shortcut -- the field as the top bits of a positive half -- is the same decode
    assert np.array_equal(np.nan_to_num((r << np.uint32(4)).astype(np.uint16).view(np.float16).astype(F), nan=-1.0),
                          np.nan_to_num(D.decode_r11g11b10(r)[..., 0], nan=-1.0))
    assert np.array_equal(np.nan_to_num((b << np.uint32(5)).astype(np.uint16).view(np.float16).astype(F), nan=-1.0),
                          np.nan_to_num(D.decode_r11g11b10(b << np.uint32(22))[..., 2], nan=-1.0))
    d = D.divisor(np.array([0, 0xFFFFFFFF], np.uint32))
    assert (d == D.FLOOR).all()  # zero and NaN fields take the floor


def test_floor_round_trips_bit_for_bit():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(0.0, 64.0, 100000), np.exp(rng.uniform(-60.0, 60.0, 100000)), [0.0, 1e-38, 3e38 / 32]]).astype(F)
    black = D.divisor(np.zeros(x.shape, np.uint32))[..., 0]
    back = ((x / black).astype(F) * black).astype(F)
    assert np.array_equal(back.view(np.uint32), x.view(np.uint32))
    assert np.array_equal(((x * F(32.0)) * F(1.0 / 32.0)).view(np.uint32), x.view(np.uint32))


def test_the_filter_sees_a_constant_under_a_checker_albedo():
    """albedo (.) E with E constant, a checker albedo, flat geometry, no noise: demodulated, the image is a constant; four frames of
    temporal + a-trous return it, and the product gives the input back to 1e-6 relative."""
    W, H, L = 64, 48, 5
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    checker = ((xs // 4 + ys // 4) & 1).astype(bool)
    # 0.8 / 0.4 / 0.2 against 0.0625 / 0.125 / 0.5, as R11G11B10 words (exponent 14: [0.5, 1))
    light = np.uint32((14 << 6) | 38) | (np.uint32((13 << 6) | 38) << np.uint32(11)) | (np.uint32((12 << 5) | 19) << np.uint32(22))
    dark = np.uint32(11 << 6) | (np.uint32(12 << 6) << np.uint32(11)) | (np.uint32(14 << 5) << np.uint32(22))
    albedo = np.where(checker, light, dark).astype(np.uint32)
    d = D.divisor(albedo)
    E = np.array([1.7, 0.9, 2.3], F)
    rad = np.ones((H, W, 4), F)
    rad[..., :3] = d * E
    depth = np.full((H, W), 0x800000, np.uint32)
    normal = np.zeros((H, W, 4), np.float16)  # oct (0, 0): +z
    s = D.DemodSVGF(W, H, L)
    for f in range(1, 5):
        # frame 1 starts as after a reset_history on a G-buffer that was already there: the history is the seed, the frame over its albedo
        s.begin_frame(f, depth, normal, rad, albedo, history=D.demodulate(rad, d) if f == 1 else None)
        if f == 1:
            s.o.depth[s.o.hist][...] = depth
            s.o.normal[s.o.hist][...] = normal
        s.temporal()
        out = s.atrous()
        rel = np.abs(out["radiance"][..., :3] - rad[..., :3]) / rad[..., :3]
        assert rel.max() <= 1e-6, (f, rel.max())
        assert np.abs(out["demod"][..., :3] / E - 1.0).max() <= 1e-6
        assert np.array_equal(out["radiance"][..., 3], rad[..., 3])
    s.close()
