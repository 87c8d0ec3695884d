"""tests/probe_frame_ref.py on the CPU: the decode against the oracle's and against hand-made words, the calibration of
the frame-weight tolerance, the judge against the corruptions it must catch, the new symbols of the ABI, and the Python mirror's
argument errors, which need no device."""
import ctypes as C

import numpy as np
import pytest

import probe_frame_ref as PF
import probe_volume_ref as PV
from nebulae_amd import _lib
from nebulae_amd.renderer import DeferredRenderer
from nebulae_amd.svgf import NebError
from oracle import gi_np

F, F64, U32 = np.float32, np.float64, np.uint32


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def cpu_case(dims, kind, w=70, h=45):
    g = PV.gpu_grid(dims)
    rec = PV.random_records(g)
    planes = PF.synthetic_gbuffer(g, kind, w, h)
    return g, rec, planes, PF.random_radiance(w, h)


def test_the_written_out_oct_unpack_is_the_oracles_on_every_fp16_pair_of_a_lattice():
    v = np.arange(0, 1 << 16, 37, dtype=np.uint16).view(np.float16)
    v = v[np.abs(v.astype(F)) <= 1.0]
    pairs = np.stack(np.meshgrid(v, v[::3]), -1).reshape(-1, 2).astype(F)
    with np.errstate(all="ignore"):
        assert same_bits(PF.oct_unpack32(pairs), gi_np.oct16_fast_unpack(pairs)) and len(pairs) > 100000
    assert same_bits(PF.oct_unpack32(np.zeros((1, 2), F)), np.array([[0, 0, 1]], F))  # a zero pair is +z, not a zero normal
    assert same_bits(PF.oct_unpack32(np.array([[1.0, 1.0]], F)), (np.array([[0, 0, -1]], F64)).astype(F))


def test_points_follow_the_planes():
    g, _, planes, _ = cpu_case((5, 4, 3), "special")
    pts = PF.points32(planes).reshape(45, 70, 8)
    sky = PF.sky(planes)
    assert sky.any() and not pts[sky][:, [0, 1, 2, 4, 5, 6]].any() and (pts[..., 3] == F(0.01)).all() and np.isinf(pts[..., 7]).all()
    assert same_bits(pts[~sky][:, 0:3], planes["world_pos"][~sky][:, 0:3].astype(F))
    use = PV.usable(pts.reshape(-1, 8)).reshape(45, 70)
    turn = (np.mgrid[0:45, 0:70][1] + 3 * np.mgrid[0:45, 0:70][0]) % 16
    assert not use[turn <= 2].any() and use[turn >= 3].all()  # sky, infinity, NaN: not usable; the zero oct pair is +z and is
    n = pts[use][:, 4:7].astype(F64)
    assert np.abs(np.sqrt((n * n).sum(-1)) - 1.0).max() < 1e-6
    gn = PF.points32(planes, geometric_normal=True).reshape(45, 70, 8)
    assert not same_bits(gn[use][:, 4:7], pts[use][:, 4:7]) and same_bits(gn[..., 0:4], pts[..., 0:4])
    got = PV.gather32(g, PV.random_records(g), pts.reshape(-1, 8))
    flags = got["flags"].reshape(45, 70)
    assert (flags[turn <= 2] == _lib.GATHER_NOT_GATHERED).all() and (flags[turn == 6] & _lib.GATHER_NO_PROBE).all()
    assert (flags[(turn == 4) | (turn == 5)] & _lib.GATHER_CLAMPED).all() and PF.stored(got).sum() > 1500


@pytest.mark.parametrize("kind", PF.KINDS)
def test_every_synthetic_gbuffer_has_the_wave_shape_it_is_named_for(kind):
    g = PV.gpu_grid((5, 4, 3))
    planes = PF.synthetic_gbuffer(g, kind, 70, 45)
    got = PV.gather32(g, PV.random_records(g), PF.points32(planes))
    cell, ok = got["cell"].reshape(45, 70), (got["flags"] & _lib.GATHER_NOT_GATHERED).reshape(45, 70) == 0
    shared = [len(set(cell[y:y + 8, x:x + 8][ok[y:y + 8, x:x + 8]])) for y in range(0, 45, 8) for x in range(0, 70, 8)]
    if kind == "uniform":
        assert max(shared) == 1 and ok.all()
    elif kind == "stray":
        assert max(shared) == 2 and shared.count(2) > len(shared) // 2
    else:
        assert min(shared[:40]) > 4


def test_a_constant_field_gives_lambert_and_metal_pixels_gain_nothing():
    g, rec, planes, rad = cpu_case((5, 4, 3), "uniform")
    n = 45 * 70
    gathered = dict(irradiance=np.full((n, 3), np.pi, F), flags=np.zeros(n, U32))
    out = PF.indirect32(rad, planes, gathered)
    want = rad[..., 0:3].astype(F64) + PF.diffuse_k(planes, F64)
    assert np.abs(out[..., 0:3] - want).max() < 1e-5 and same_bits(out[..., 3], rad[..., 3])
    metal = planes["rough_metal"][..., 1] == 1.0
    assert metal.any() and np.array_equal(out[metal], rad[metal])  # (adds 0: the values, since -0 + 0 is +0)
    w32, w64 = (PF.frame_weighted(rad, planes, gathered, PF.CAMERA, T) for T in (F, F64))
    assert np.array_equal(w32[metal], rad[metal]) and np.array_equal(w64[metal], rad[metal].astype(F64))
    factor = PF.frame_factor(planes, PF.CAMERA, F64)
    assert factor.min() >= 1.1 - 1e-12 and factor.max() <= 1.9 + 1e-12 and factor.std() > 0.01  # pd is clamped to 0.1 .. 0.9


def test_calibration():
    """MEASURED is the measurement: the float32 statement's largest error under the judge over the GPU test's own planes, within 10 %
    above it (the rule of probe_volume_ref.MEASURED)"""
    worst = 0.0
    for dims in PF.GRIDS:
        for kind in PF.KINDS:
            g, rec, planes, rad = cpu_case(dims, kind)
            gathered = PV.gather32(g, rec, PF.points32(planes))
            got = PF.frame_weighted(rad, planes, gathered, PF.CAMERA, F)
            worst = max(worst, PF.judge_weighted(got, rad, planes, gathered, PF.CAMERA, f"{dims} / {kind}", tol=np.inf))
    print(f"[calibration] frame_weight: {worst:.3e}, MEASURED {PF.MEASURED['frame_weight']:.1e}")
    assert worst <= PF.MEASURED["frame_weight"] <= 1.1 * worst


@pytest.mark.parametrize("dims", PF.GRIDS)
def test_the_identity_judge_fails_what_it_should(dims):
    kind = "special" if dims == (5, 4, 3) else "permuted"
    g, rec, planes, rad = cpu_case(dims, kind)
    gathered = PV.gather32(g, rec, PF.points32(planes))
    good = PF.indirect32(rad, planes, gathered)
    assert PF.judge_identity(good, rad, planes, gathered, "the statement itself") > 100
    for corrupt in PF.CORRUPTIONS:
        if corrupt == "geometric normal used":
            bad = PF.indirect32(rad, planes, PV.gather32(g, rec, PF.points32(planes, geometric_normal=True)))
        else:
            bad = PF.indirect32(rad, planes, gathered, corrupt)
        if same_bits(bad, good):  # the corruption has nothing to act on in this case: say why
            assert (corrupt, dims) in (("sky pixels lit", (1, 1, 1)), ("a NO_PROBE pixel stored to", (1, 1, 1))), (corrupt, dims)
            continue
        with pytest.raises(AssertionError):
            PF.judge_identity(bad, rad, planes, gathered, corrupt)
        with pytest.raises(AssertionError):  # and the float64 judge of the weighted term is no blinder
            PF.judge_weighted(bad, rad, planes, gathered, PF.CAMERA, corrupt, tol=1.0 if corrupt in ("alpha written", "a NO_PROBE pixel stored to") else None)


def test_the_weighted_judge_fails_a_missing_factor():
    g, rec, planes, rad = cpu_case((5, 4, 3), "permuted")
    gathered = PV.gather32(g, rec, PF.points32(planes))
    PF.judge_weighted(PF.frame_weighted(rad, planes, gathered, PF.CAMERA, F), rad, planes, gathered, PF.CAMERA, "the statement itself")
    with pytest.raises(AssertionError):
        PF.judge_weighted(PF.indirect32(rad, planes, gathered), rad, planes, gathered, PF.CAMERA, "plain Lambert")
    with pytest.raises(AssertionError):
        PF.judge_weighted(PF.frame_weighted(rad, planes, gathered, (0.0, 0.0, -3.0), F), rad, planes, gathered, PF.CAMERA, "another camera")


def test_the_library_exports_the_calls_and_refuses_a_null_context_without_a_device():
    lib = _lib.load()
    assert lib.neb_gbuffer_points(None, 0, 1, None, None) == -1
    assert lib.neb_gi_probe_indirect(None, None, None, None, 0, None) == -1
    assert lib.neb_gi_probe_indirect_rows(None, None, None, None, 0, 0, 1, None) == -1
    assert _lib.INDIRECT_FRAME_WEIGHT == 1


class _NoDevice(DeferredRenderer):
    """a renderer whose context was never created: the mirror's own checks run first"""

    def __init__(self, w, h, row_begin=0, row_end=0):
        super().__init__()
        self.width, self.height = w, h
        self.svgf.row_begin, self.svgf.row_end = row_begin, row_end or h


def test_the_mirror_raises_its_argument_errors_without_a_device():
    torch = pytest.importorskip("torch")
    r = _NoDevice(70, 45, 8, 24)
    g = PV.gpu_grid((5, 4, 3))
    grid = PV.grid_struct(g)
    rec = torch.zeros((60, 32))
    for rows in ((0, 8), (8, 8), (20, 10), (8, 25), (8,), "ab", (1, 2, 3)):
        with pytest.raises(NebError, match="rows"):
            r.gbuffer_points(rows=rows)
    for out in (torch.zeros((16 * 70, 8)), torch.zeros((3, 8), dtype=torch.float64), np.zeros((16 * 70, 8), F)):
        with pytest.raises(NebError, match="out must be"):
            r.gbuffer_points(out=out)
    with pytest.raises(NebError, match="grid must be"):
        r.submit_commands_gi_probes(g, rec)
    with pytest.raises(NebError, match="records must be"):
        r.submit_commands_gi_probes(grid, rec)  # (not on a device)
    bad = PV.grid_struct(g)
    bad.spacing[1] = 0.0
    with pytest.raises(NebError, match="spacing"):
        r.submit_commands_gi_probes(bad, rec)
