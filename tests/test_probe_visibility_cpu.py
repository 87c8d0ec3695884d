"""tests/probe_visibility_ref.py on the CPU: the float32 restatement against the float64 one gives the constants the
GPU test judges by; every corruption the reference can name is caught by the judge that guards it; the octahedral lookup is continuous
across the map's edges and corners; maps that see everything give probe_volume_ref's plain gather bit for bit; the accumulation's special
cases; and the leak fixture shows its reduction in float64, from maps built with the brute-force float64 caster."""
import numpy as np
import pytest

import probe_visibility_ref as R
import probe_volume_ref as PV
import views_ref as V

F, F64, U32 = np.float32, np.float64, np.uint32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def inputs():
    """the GPU test's synthetic gather inputs with both restatements, computed once and left unchanged"""
    out = []
    for dims in PV.DIMS:
        g = PV.gpu_grid(dims)
        rec, maps = PV.random_records(g), R.random_maps(g)
        for n in PV.COUNTS:
            for kind in R.KINDS:
                pts = PV.points(g, kind, n)
                parts = {}
                want = R.gather64(g, rec, maps, R.NORMAL_BIAS, pts, parts=parts)
                out.append(dict(name=f"{dims} / {n} / {kind}", grid=g, records=rec, maps=maps, points=pts, want=want, branch=parts["branch"],
                                got=R.gather32(g, rec, maps, R.NORMAL_BIAS, pts)))
    return out


def test_calibration(inputs):
    """MEASURED is the measurement rounded up (TOL = 4 x), on inputs in which both branches of the Chebyshev test and its floor each
    decide at least a tenth of the corners looked up."""
    worst = max(R.judge_gather(c["got"], c["want"], c["name"], tol=np.inf) for c in inputs)
    print(f"[calibration] measured gather error {worst:.4e}; constant {R.MEASURED['gather']:.3e}")
    assert worst <= R.MEASURED["gather"] <= 1.25 * worst, f"the constant is not the measurement {worst:.4e} rounded up"
    shares = R.branch_shares(dict(branch=np.concatenate([c["branch"] for c in inputs], 1)))
    print(f"[calibration] corners with r <= m1 {shares[0]:.3f}, Chebyshev above the floor {shares[1]:.3f}, at the floor {shares[2]:.3f}")
    assert min(shares) >= 0.1, shares
    d, t, hit, D = R.synthetic_samples()
    bake = R.judge_bake(R.bake_reduce(d, t, hit, D, F), R.bake_reduce(d, t, hit, D), "bake32", tol=np.inf)
    print(f"[calibration] measured bake error {bake:.4e}; constant {R.MEASURED['bake']:.3e}")
    assert bake <= R.MEASURED["bake"] <= 1.25 * bake, f"the constant is not the measurement {bake:.4e} rounded up"
    assert all(R.TOL[k] == 4.0 * R.MEASURED[k] for k in R.MEASURED)


@pytest.mark.parametrize("corrupt", R.GATHER_CORRUPTIONS)
def test_every_corruption_of_the_gather_is_caught(inputs, corrupt):
    """the corrupted float32 gather, judged as the device is, fails on the GPU test's own inputs"""
    caught = 0
    for c in inputs:
        if len(c["points"]) < 4097:
            continue
        bad = R.gather32(c["grid"], c["records"], c["maps"], R.NORMAL_BIAS, c["points"], corrupt=corrupt)
        try:
            R.judge_gather(bad, c["want"], c["name"])
        except AssertionError:
            caught += 1
    assert caught > 0, f"'{corrupt}' passes the judge on every input"


def test_a_reversed_sample_order_is_caught_by_the_bit_comparison():
    """The bake is held to bake_reduce in float32 BIT FOR BIT, which is the judge that guards the order of its sums: in float64 the two
    orders differ by 1e-16, far below any tolerance on float32 data, so no tolerance can see this corruption and tolerance 0 must."""
    d, t, hit, D = R.synthetic_samples()
    a, b = R.bake_reduce(d, t, hit, D, F), R.bake_reduce(d, t, hit, D, F, corrupt="sample order reversed")
    assert not same_bits(a["moments"], b["moments"]) and not same_bits(a["weight"], b["weight"])
    R.judge_bake(b, R.bake_reduce(d, t, hit, D), "reversed", tol=R.TOL["bake"])  # (inside the tolerance: only the bits tell)
    assert R.CORRUPTIONS[-1] == "sample order reversed" and set(R.GATHER_CORRUPTIONS) | {R.CORRUPTIONS[-1]} == set(R.CORRUPTIONS)


def test_the_bake_reduction_on_inputs_with_known_answers():
    nk = R.texel_directions()
    assert np.allclose(np.linalg.norm(nk, axis=-1), 1.0, atol=1e-15) and (nk[[27, 28, 35, 36], 2] > 0.9).all()  # (the map's middle looks along +z)
    # one sample along texel 27's direction, a hit at 0.5: the texels within 75.5 degrees of it hold exactly (0.5, 0.25), the others nothing
    d = np.tile(nk[27].astype(F), (1, 64, 1))
    t, hit = np.full((1, 64), 0.5, F), np.ones((1, 64), bool)
    out = R.bake_reduce(d, t, hit, 2.0)
    c = nk @ d[0, 0].astype(F64)
    near = c >= 0.25
    assert near.sum() > 8 and (~near).sum() > 8
    assert np.allclose(out["moments"][0, near], (0.5, 0.25), rtol=1e-12) and np.allclose(out["weight"][0, near], 64 * c[near] ** 32, rtol=1e-12)
    assert (out["moments"][0, ~near] == (2.0, 4.0)).all() and (out["weight"][0, ~near] == 0).all()
    # misses and hits beyond max_distance count as max_distance; a probe that is not baked holds max_distance everywhere
    far = R.bake_reduce(d, np.full((1, 64), 7.0, F), hit, 2.0)
    miss = R.bake_reduce(d, np.full((1, 64), np.inf, F), ~hit, 2.0)
    assert np.allclose(far["moments"][0, near], (2.0, 4.0)) and same_bits(far["moments"], miss["moments"])
    none = R.bake_reduce(d, t, hit, 2.0, is_baked=[False])
    assert (none["moments"] == (2.0, 4.0)).all() and not none["weight"].any()
    pr = PV.grid_probes(PV.gpu_grid((2, 2, 2)), tmin=0.0, tmax=1.0)
    pr[1, 0], pr[2, 7], pr[3, 3] = np.nan, 0.0, -1.0
    assert R.baked(pr).tolist() == [True, False, False, False, True, True, True, True]


def test_the_lookup_is_continuous_across_the_edges_and_corners_of_the_map():
    """The four edges of the map are the four half planes ux = 0 and uy = 0 of the lower hemisphere (each edge glued to itself, mirrored
    about its middle), and its four corners are the pole -z.  Directions a hair (1e-7) apart on either side of an edge, around the pole,
    and across the fold at uz = 0 read moments that differ by less than a bilinear step of that size: the wrapped taps are the
    neighbours on the sphere.  With the wrap replaced by a clamp they are not."""
    rng = np.random.default_rng(5)
    maps = np.zeros((1, 64, 2))
    maps[0, :, 0] = rng.uniform(0.2, 2.0, 64)
    maps[0, :, 1] = maps[0, :, 0] ** 2 * 1.3
    step = 1e-6 * np.ptp(maps[0, :, 0]) * 4.0  # (a bilinear step of 1e-6 texels moves m1 by at most that share of the map's range, per axis, twice)

    def m1_at(u, corrupt=None):
        parts = {}
        R.visibility_factor(np.repeat(maps, len(u), 0), np.asarray(u, F64), F64, corrupt, parts)
        return parts["m1"]

    # across uz = 0 everywhere along the fold, the axes +-x and +-y included
    phi = np.concatenate([np.linspace(0.0, 2.0 * np.pi, 257)[:-1], [0.0, 0.5 * np.pi, np.pi, 1.5 * np.pi]])
    ring = np.stack([np.cos(phi), np.sin(phi), np.zeros_like(phi)], -1)
    up, down = ring + (0, 0, 1e-7), ring - (0, 0, 1e-7)
    assert np.abs(m1_at(up) - m1_at(down)).max() < step
    # across each of the four edges, all along it
    along = np.linspace(0.02, 0.98, 97)
    for axis in (0, 1):
        for sign in (-1.0, 1.0):
            u = np.zeros((len(along), 3))
            u[:, 1 - axis], u[:, 2] = sign * along, -(1.0 - along)
            left, right = u.copy(), u.copy()
            left[:, axis], right[:, axis] = -1e-7, 1e-7
            assert np.abs(m1_at(left) - m1_at(right)).max() < step, (axis, sign)
            assert np.abs(m1_at(left, "wrap replaced by clamp") - m1_at(right, "wrap replaced by clamp")).max() > 1000 * step, (axis, sign)
    # around the pole -z, where the four corners of the map meet, and around +z, its middle
    for pole in (-1.0, 1.0):
        small = 1e-7 * ring + (0, 0, pole)
        values = m1_at(small)
        assert np.ptp(values) < step, (pole, np.ptp(values))
    # taps on the rows and columns -1 and 7 do occur, on both sides of the fold
    taps, fx, fy = R.lookup(np.concatenate([up, down, ring * 0.3 + (0, 0, -1.0), ring * 0.3 + (0, 0, 1.0)]), F64)
    assert R.wrap(-1, -1) == 63 and R.wrap(8, 3) == 7 + 8 * 4 and R.wrap(3, 8) == 4 + 8 * 7 and R.wrap(-1, 3) == 8 * 4 and R.wrap(8, 8) == 0
    edge = set(range(8)) | set(range(56, 64)) | set(range(0, 64, 8)) | set(range(7, 64, 8))
    assert edge <= set(np.unique(taps).tolist())  # (every texel of the map's rim is tapped)


def test_maps_that_see_everything_give_the_plain_gather_bit_for_bit(inputs):
    for c in inputs:
        g = c["grid"]
        clear = R.all_visible(PV.count(g), 64.0)  # (64 is above every distance of these grids)
        a, b = R.gather32(g, c["records"], clear, R.NORMAL_BIAS, c["points"]), PV.gather32(g, c["records"], c["points"])
        assert all(same_bits(a[k], b[k]) for k in b), c["name"]
        a, b = R.gather64(g, c["records"], clear, R.NORMAL_BIAS, c["points"]), PV.gather64(g, c["records"], c["points"])
        assert all(same_bits(a[k], b[k]) for k in b), c["name"]


def test_a_point_on_a_probe_and_the_floor():
    """rr == 0 gives 1 whatever the map holds; a probe far in front of what it sees keeps the floor 0.05 of its weight"""
    maps = np.zeros((2, 64, 2))
    maps[..., 0], maps[..., 1] = 0.1, 0.0101
    vis = R.visibility_factor(maps, np.array([[0.0, 0.0, 0.0], [0.3, -0.2, 5.0]]))
    assert vis[0] == 1.0 and vis[1] == 0.05
    assert R.visibility_factor(maps, np.array([[0.3, -0.2, 5.0]] * 2), corrupt="floor 0.05 dropped")[0] < 1e-6
    near = R.visibility_factor(maps, np.array([[0.01, 0.02, -0.05]] * 2))
    assert (near == 1.0).all()  # (r <= m1)


def test_accumulation():
    rng = np.random.default_rng(2)
    maps = []
    for q in range(4):
        m = R.random_maps(PV.gpu_grid((2, 2, 2)), seed=20 + q)
        m["weight"][rng.uniform(size=m["weight"].shape) < 0.2] = 0.0
        maps.append(m)
    acc = R.Accumulator64(8)
    acc.add(maps[0])
    taken = maps[0]["weight"] != 0
    assert same_bits(acc.records["moments"][taken], maps[0]["moments"][taken]) and not acc.records["weight"][~taken].any()  # (a zeroed start takes `add`)
    before = acc.records.copy()
    empty = maps[1].copy()
    empty["weight"][...] = 0.0
    acc.add(empty)
    assert same_bits(acc.records, before)  # (a zero-weight add keeps every bit)
    for m in maps[1:]:
        acc.add(m)
    # the float64 mean of all four, straight: sum(w m) / sum(w)
    w = np.stack([m["weight"].astype(F64) for m in maps])
    mom = np.stack([m["moments"].astype(F64) for m in maps])
    some = w.sum(0) > 0
    mean = (w[..., None] * mom).sum(0)[some] / w.sum(0)[some][:, None]
    assert np.allclose(acc.value[some], mean, rtol=1e-13) and (acc.bound[some] < 1e-5).all() and acc.folds.max() == 3


def test_the_leak_fixture_shows_its_reduction_in_float64():
    """The scene of the GPU test's leak case, its maps built from the float64 brute-force caster along the float64 directions of the
    bake: the probes of the lit half, whose SH hold radiance 1, lose most of their weight at points behind the dividing wall."""
    sc, g = R.leak_scene(), R.leak_grid()
    pr = PV.grid_probes(g, tmin=0.0, tmax=1e4)
    n, S = len(pr), R.LEAK_SAMPLES
    # no probe lies inside a slab of the scene
    for lo, hi in R.leak_parts():
        assert not ((pr[:, 0:3] > np.array(lo)) & (pr[:, 0:3] < np.array(hi))).all(-1).any()
    dirs = R.probe_directions64(pr, S, 1)
    hits = V.cast(V.triangles(sc), np.repeat(pr[:, 0:3].astype(F64), S, 0), dirs.reshape(-1, 3), 0.0, 1e4)
    t = hits["t"].reshape(n, S)
    dark = pr[:, 0] > 0
    assert np.isfinite(t[dark]).all() and (~np.isfinite(t[~dark])).any()  # (the dark half is closed, the lit one open above)
    maps = R.bake_reduce(dirs, t, np.isfinite(t), R.LEAK_MAX_DISTANCE)
    vis = R.as_array({k: v.astype(F) for k, v in maps.items()})
    rec, pts = R.leak_records(g), R.leak_points()
    assert len(pts) == 200 and (pts[:, 0] - 0.025 > R.LEAK_BIAS).all() and (pts[:, 0] < 0.025 + R.LEAK_SPACING).all()
    plain = PV.gather64(g, rec, pts)["irradiance"][:, 0]
    visible = R.gather64(g, rec, vis, R.LEAK_BIAS, pts)["irradiance"][:, 0]
    ratio = float(visible.sum() / plain.sum())
    print(f"[leak] float64: sum(E_visible) / sum(E_plain) = {ratio:.4f} over {len(pts)} points; plain E from {plain.min():.3f} to {plain.max():.3f}")
    assert (plain > 0).all() and (visible < plain).all()
    assert ratio < 0.5
