"""neb_gi_set_morph_targets, neb_gi_morph_vertices: what holds without a GPU -- the reference of the written order (tests/morph_ref.py)
against float64 blending, the zero-weight rule, the cases the GPU tests assume, the exports, the ctypes mirrors of the two structs, the
null-context answers."""
import ctypes as C
import os
import subprocess

import numpy as np

import morph_ref
from nebulae_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("neb_gi_set_morph_targets", "neb_gi_morph_vertices")
F = np.float32
U = float(np.finfo(np.float32).eps) / 2.0  # the unit roundoff


def _random_case(n=100_000, T=6, seed=7):
    rng = np.random.default_rng(seed)
    P = rng.uniform(-40.0, 40.0, (n, 3)).astype(F)
    N = rng.normal(size=(n, 3))
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(F)
    Tn = np.concatenate([np.roll(N, 1, axis=1), np.where(rng.random((n, 1)) < 0.5, -1.0, 1.0)], axis=1).astype(F)
    targets = dict(positions=rng.uniform(-5.0, 5.0, (T, n, 3)).astype(F), normals=rng.uniform(-0.5, 0.5, (T, n, 3)).astype(F),
                   tangents=rng.uniform(-0.5, 0.5, (T, n, 3)).astype(F))
    return P, N, Tn, targets


def test_the_written_order_stays_float32_and_is_within_its_roundings_of_float64_blending():
    """Bound per component, for A active targets: gamma(A + 1) * sum|terms|, gamma(r) = r u / (1 - r u), u = 2^-24 -- to first order
    (A + 1) unit roundoffs.  The longest path through the expression is the first active product's: its own rounding and then the A
    sums, A + 1 roundings; the rest value crosses the A sums, the k-th active product A - k + 2 roundings.  Each rounding multiplies
    what passes it by (1 + d), |d| <= u, so every term's relative error is at most (1 + u)^(A + 1) - 1 <= gamma(A + 1), and the sum of
    the absolute terms carries it.  sum|terms| = |rest| + sum_k |w_k d_k| over the active targets, formed in float64 from the same
    float32 inputs.  Weight sets: all six active, a zero in the middle, a negative weight."""
    P, N, Tn, targets = _random_case()
    worst = {}
    for kind in ("all", "zero_mid", "negative"):
        w = morph_ref.weight_set(6, kind)
        A = int((w != 0).sum())
        assert A == (5 if kind == "zero_mid" else 6)
        got = morph_ref.morph(P, N, Tn, targets, w)
        gamma = (A + 1) * U / (1.0 - (A + 1) * U)
        for key, rest, width in (("positions", P, 3), ("normals", N, 3), ("tangents", Tn[:, :3], 4)):
            assert got[key].dtype == np.float32 and got[key].shape == (P.shape[0], width), key
            terms = w.astype(np.float64)[:, None, None] * targets[key].astype(np.float64)
            want = rest.astype(np.float64) + terms.sum(0)
            mag = np.abs(rest.astype(np.float64)) + np.abs(terms).sum(0)
            err = np.abs(got[key][:, :3].astype(np.float64) - want)
            worst[kind, key] = float((err / mag).max() / U)
            assert (err <= gamma * mag).all(), (kind, key, worst[kind, key])
        assert np.array_equal(got["tangents"][:, 3], Tn[:, 3])  # (.w copied)
    print(f"[morph_ref] worst error in unit roundoffs of sum|terms| (bound: A + 1 = 7, 6 with a zero weight): "
          + ", ".join(f"{k[0]}/{k[1]} {v:.2f}" for k, v in worst.items()))


def test_all_zero_weights_return_the_rest_bits_and_a_zero_weight_is_skipped():
    P, N, Tn, targets = _random_case(n=1000)
    P[3, 1] = N[5, 0] = Tn[7, 2] = -0.0  # (x + 0 * d would turn these into +0.0)
    w = morph_ref.weight_set(6, "none")
    assert not w.any() and np.signbit(w[-1])
    got = morph_ref.morph(P, N, Tn, targets, w)
    for key, a in (("positions", P), ("normals", N), ("tangents", Tn)):
        assert np.array_equal(got[key].view(np.uint32), a.view(np.uint32)), key
    # a zero in the list: the same bits as the list without that target
    w = morph_ref.weight_set(6, "zero_mid")
    keep = np.flatnonzero(w != 0)
    assert len(keep) == 5
    short = {k: v[keep] for k, v in targets.items()}
    a, b = morph_ref.morph(P, N, Tn, targets, w), morph_ref.morph(P, N, Tn, short, w[keep])
    assert all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in morph_ref.KEYS)
    # targets without normal and tangent deltas: the rest bits
    got = morph_ref.morph(P, N, Tn, dict(positions=targets["positions"], normals=None, tangents=None), morph_ref.weight_set(6, "all"))
    assert np.array_equal(got["normals"].view(np.uint32), N.view(np.uint32)) and np.array_equal(got["tangents"].view(np.uint32), Tn.view(np.uint32))
    assert not np.array_equal(got["positions"], P)


def test_the_cases_are_what_the_gpu_tests_assume():
    for name, make in morph_ref.CASES.items():
        c = make()
        for k in (0, 1):
            morph_ref.guard(c, k)
        w2 = c.weights(2)
        assert all(not w.any() for w in w2.values()), name
        for gi in c.indices:
            t = c.targets[gi]
            nv = len(c.sc0.geometries[gi]["positions"])
            assert t["positions"].shape == (c.T(gi), nv, 3) and t["positions"].dtype == np.float32, (name, gi)
            assert (t["normals"] is None) == (name == "room") and (t["tangents"] is None) == (name == "room"), (name, gi)
    # the shapes the issue names
    c = morph_ref.cornell_case()
    w = c.weights(0)[morph_ref.SHORT_BOX]
    assert c.T(morph_ref.SHORT_BOX) == 3 and w[1] == 0 and w[0] != 0 and w[2] != 0
    assert (c.weights(1)[morph_ref.SHORT_BOX] < 0).any()
    c = morph_ref.boxes_case()
    assert (c.T(morph_ref.SHORT_BOX), c.T(morph_ref.TALL_BOX)) == (1, 4)
    c = morph_ref.room_case()
    assert [c.T(gi) for gi in c.indices] == [2]
    # the atrium call: different T and active sets, ranges that cross 256-lane blocks, and at least one 64-lane wave of the one launch
    # (lanes in geometry order, one per vertex) spans two geometries whose active lists differ in length
    c = morph_ref.atrium_case()
    counts = [len(c.sc0.geometries[gi]["positions"]) for gi in c.indices]
    active = [int((c.weights(0)[gi] != 0).sum()) for gi in c.indices]
    assert len(c.indices) == 4 and len({c.T(gi) for gi in c.indices}) == 4 and len(set(active)) >= 3, (counts, active)
    assert all(n > 256 for n in counts) and max(active) > 4 > min(active)  # (a full group of four and a remainder; fewer than a group)
    ends = np.cumsum(counts)[:-1]
    spanning = [int(e) for e, a, b in zip(ends, active[:-1], active[1:]) if e % 64 != 0 and a != b]
    print(f"[morph cases] atrium grids: vertices {counts}, active targets {active}, range ends inside a wave with another list length: {spanning}")
    assert spanning
    # with skins: the same targets
    for make in (morph_ref.cornell_case, morph_ref.atrium_case):
        c = make(skinned=True)
        assert sorted(c.skins) == c.indices
        for arrays in c.morphed_and_skinned(0, 0).values():
            assert all(np.isfinite(arrays[k]).all() for k in morph_ref.KEYS)


def test_the_library_exports_the_two_calls_and_the_binding_declares_them():
    build.build()
    raw = C.CDLL(build.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.exported_symbols(), name
    sigs = _lib._gi_sigs()
    assert sigs["neb_gi_set_morph_targets"] == (C.c_int, [C.c_void_p, C.POINTER(_lib.MorphDesc), C.c_uint32, C.c_void_p])
    assert sigs["neb_gi_morph_vertices"] == (C.c_int, [C.c_void_p, C.POINTER(_lib.MorphUpdate), C.c_uint32, C.c_void_p])
    header = open(os.path.join(ROOT, "include", "nebulae_hip.h")).read()
    assert "int neb_gi_set_morph_targets(neb_ctx* ctx, const neb_morph_desc* descs, uint32_t n, neb_stream stream);" in header
    assert "int neb_gi_morph_vertices(neb_ctx* ctx, const neb_morph_update* updates, uint32_t n, neb_stream stream);" in header
    mirror = open(os.path.join(ROOT, "include", "nebulae_hip.hpp")).read()
    for name in NAMES:
        assert name in mirror, name


def test_the_ctypes_structs_have_the_sizes_and_offsets_of_the_header(tmp_path):
    fields = {"neb_morph_desc": ("geometry", "numTargets", "positionDeltas", "positionStride", "normalDeltas", "normalStride", "tangentDeltas",
                                 "tangentStride"),
              "neb_morph_update": ("geometry", "weights", "jointMatrices")}
    lines = "".join(f'  printf("{s} %zu", sizeof({s}));' + "".join(f' printf(" %zu", offsetof({s}, {f}));' for f in fs) + ' printf("\\n");\n'
                    for s, fs in fields.items())
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nebulae_hip.h"\nint main(void) {\n' + lines + "  return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    for line, (s, fs), T in zip(out, fields.items(), (_lib.MorphDesc, _lib.MorphUpdate)):
        words = line.split()
        assert words[0] == s
        assert int(words[1]) == C.sizeof(T), (s, words[1], C.sizeof(T))
        assert [int(x) for x in words[2:]] == [getattr(T, f).offset for f in fs], s
        assert [n for n, _ in T._fields_] == list(fs), s


def test_a_null_context_is_refused_before_anything_else_is_looked_at():
    lib = _lib.load()
    d = _lib.MorphDesc(geometry=0, numTargets=1, positionStride=12)  # (never dereferenced)
    u = _lib.MorphUpdate(geometry=0)
    assert lib.neb_gi_set_morph_targets(None, C.byref(d), 1, None) == -1
    assert lib.neb_gi_set_morph_targets(None, None, 0, None) == -1
    assert lib.neb_gi_morph_vertices(None, C.byref(u), 1, None) == -1
    assert lib.neb_gi_morph_vertices(None, None, 0, None) == -1
