"""GPU test of the one-call strip frame (neb_strip_frame_begin / _finish with neb_strip_peers, strips.hip) with every strip on a stream
of its OWN: N strip contexts on N streams of one GPU, the closest this suite can come to N devices.  It is the one part of the library whose
result rests on ordering BETWEEN streams, and on one stream the stream order hides every missing dependency -- so here single streams are
made late by bounded device work (never a host sleep, never a kernel that waits for a flag) at each place where an event has to carry the
order: in front of a strip's inputs (the neighbours' pushes into its halo must wait for them: `inputs`; its own pushes are late: `pushed`),
between the two sweeps, and behind its finish (`frame_done`).  Every run must equal the full image (one context, fused chain) bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from nebulae_amd import scene as S
from nebulae_amd import strips
from nebulae_amd.renderer import RenderInfo
from nebulae_amd.svgf import PLANE_RADIANCE

pytestmark = pytest.mark.gpu

# (W, H, N, L), the smallest at which each mechanism exists: three 32-row strips with a 14-row halo (the middle one has both neighbours);
# two 96-row strips whose 62-row halo is most of a strip
SHAPES = [(128, 96, 3, 3), (256, 192, 2, 5)]
FRAMES = range(1, 7)  # frame 1 moves (SVGF skipped), frame 2 resets the history, then steady frames
RESET_FRAME, STEADY_FRAME = 2, 4
MARGIN = 10.0         # a delay must measure at least this many undelayed frames: the delayed stream is then certainly the last one
DELAY_ELEMS = 1 << 26  # one delay step = one in-place elementwise pass over 256 MiB: long against the host's cost of launching it


def _shape_id(shape):
    return "%dx%d_N%d_L%d" % shape


class _Delays:
    """Bounded device work on one stream: a chain of elementwise passes over a large tensor, its length taken from a measurement."""

    def __init__(self):
        self.buf = torch.zeros(DELAY_ELEMS, dtype=torch.float32, device="cuda")
        for _ in range(3):
            self.buf.add_(1.0)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(10):
            self.buf.add_(1.0)
        t1.record()
        torch.cuda.synchronize()
        self.step_ms = t0.elapsed_time(t1) / 10

    def enqueue(self, stream, ms):
        """at least `ms` of work on `stream` -> the two events that bracket it"""
        steps = max(1, math.ceil(ms / self.step_ms))
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            t0.record(stream)
            for _ in range(steps):
                self.buf.add_(1.0)
            t1.record(stream)
        return t0, t1


def _neighbours(rs, k):
    return (rs[k - 1] if k > 0 else None, rs[k + 1] if k + 1 < len(rs) else None)


def _run_strips(shape, sc, cam, want_frames, order="up", delays=None, delay_ms=None, time_frames=False, violate=False, share_first_two=False):
    """Six frames of N strips, strip r on stream s[r] from its first call to its last.  delays: {(frame, where, strip): multiple of delay_ms},
    where = "inputs" (in front of the strip's inputs of that frame), "sweeps" (between the begin sweep and the finish sweep) or "after"
    (behind its finish).  time_frames: a host synchronisation in front of every frame and its time on the device, all strips (ms).
    violate: in the steady frame, the calls the contract forbids are made first and must be refused.
    -> (owned rows of every strip stacked = the image, [ms per SVGF frame], [(units of delay, ms measured)])"""
    W, H, N, L = shape
    part = strips.StripPartition(W, H, N, L, scheme="once")
    rs = [strips.StripRenderer(part, k) for k in range(N)]
    s = [torch.cuda.Stream() for _ in range(N)]
    if share_first_two:  # strips 0 and 1 on one stream, the others on their own: stream order on one edge, events on the next
        s[1] = s[0]
    sweep = list(range(N)) if order == "up" else list(reversed(range(N)))
    delays = delays or {}
    times, measured = [], []

    def delay(f, where, k):
        if (f, where, k) in delays:
            units = delays[(f, where, k)]
            measured.append((units, _delayer().enqueue(s[k], units * delay_ms)))

    for f in FRAMES:
        if time_frames:
            torch.cuda.synchronize()
            start = torch.cuda.Event(enable_timing=True)
            start.record()
            for st in s:
                st.wait_event(start)
        for k, r in enumerate(rs):
            delay(f, "inputs", k)
            r.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f, stream=s[k].cuda_stream))
            r.submit_commands_gbuffer()
            with torch.cuda.stream(s[k]):
                r.svgf.plane_tensor(PLANE_RADIANCE, r.svgf.get_current_resource_index()).fill_(0.125)  # the direct term's stand-in
        refusals = violate and f == STEADY_FRAME
        if refusals:
            _refused(rs, sweep[0], "finish", b"without the neb_strip_frame_begin of this frame")
        ran = []
        for k in sweep:
            ran.append(rs[k].submit_strip_frame_local("begin", *_neighbours(rs, k)))
            if refusals and k == sweep[0]:
                _refused(rs, k, "finish", b"before the neb_strip_frame_begin of a neighbouring strip")
                _refused(rs, k, "begin", b"has begun a frame")
        for k in range(N):
            delay(f, "sweeps", k)
        ran2 = []
        for k in sweep:
            ran2.append(rs[k].submit_strip_frame_local("finish", *_neighbours(rs, k)))
            if refusals and k == sweep[0]:  # (this strip's next frame, while its neighbour is still in this one)
                _refused(rs, k, "begin", b"a neighbouring strip has not finished its previous frame")
            delay(f, "after", k)
        assert ran == ran2 == [want_frames[f]] * N
        for r in rs:
            r.end_frame()
        if time_frames:
            ends = [torch.cuda.Event(enable_timing=True) for _ in s]
            for e, st in zip(ends, s):
                e.record(st)
            torch.cuda.synchronize()
            if want_frames[f]:
                times.append(max(start.elapsed_time(e) for e in ends))
    torch.cuda.synchronize()
    got = np.concatenate([r.svgf.download(PLANE_RADIANCE, row0=part.owned(k)[0], nrows=part.owned(k)[1] - part.owned(k)[0]) for k, r in enumerate(rs)], axis=0)
    for r in rs:
        r.destroy()
    return got, times, [(units, t0.elapsed_time(t1)) for units, (t0, t1) in measured]


def _refused(rs, k, call, fragment):
    """the raw library call of strip k returns NEB_ERR_STATE and says why"""
    from nebulae_amd import _lib
    r = rs[k]
    peers = _lib.StripPeers(*[p._ctx if p is not None else None for p in _neighbours(rs, k)])
    plan, st = r.strip_plan(False), C.c_void_p(r.info.stream)
    if call == "begin":
        c = r.global_constants()
        rc = r._lib.neb_strip_frame_begin(r._ctx, C.byref(c), C.byref(plan), C.byref(peers), st)
    else:
        rc = r._lib.neb_strip_frame_finish(r._ctx, None, C.byref(plan), C.byref(peers), st)
    message = r._lib.neb_last_error(r._ctx) or b""
    assert rc == -4 and fragment in message, (call, rc, message)  # NEB_ERR_STATE


_DELAYER = None


def _delayer():
    global _DELAYER
    if _DELAYER is None:
        _DELAYER = _Delays()
    return _DELAYER


@pytest.fixture(scope="module")
def scene_and_camera():
    return S.atrium_standin(target_triangles=20000, n_submeshes=40, tex_size=32), S.sponza_camera()


@pytest.fixture(scope="module")
def references(scene_and_camera):
    """Per shape, computed once: the full image of one context (one strip = the whole frame, fused chain, through the same entry point), which
    frames ran SVGF, and t_frame = the device time of one undelayed steady frame of all N strips on their N streams."""
    sc, cam = scene_and_camera
    out = {}
    for shape in SHAPES:
        W, H, N, L = shape
        full = strips.StripRenderer(strips.StripPartition(W, H, 1, L), 0)
        ran = {}
        for f in FRAMES:
            full.begin_frame(RenderInfo(scene=sc, camera=cam, frame_index=f))
            full.submit_commands_gbuffer()
            full.svgf.plane_tensor(PLANE_RADIANCE, full.svgf.get_current_resource_index()).fill_(0.125)
            ran[f] = full.submit_strip_frame()
            full.end_frame()
        torch.cuda.synchronize()
        want = full.svgf.download(PLANE_RADIANCE)
        full.destroy()
        assert [ran[f] for f in FRAMES] == [False] + [True] * 5
        assert np.isfinite(want).all() and float(np.abs(want[..., :3]).max()) > 0.2  # (a halo left at the direct term's 0.125 cannot be right)
        want.setflags(write=False)
        got, times, _ = _run_strips(shape, sc, cam, ran, time_frames=True)
        assert len(times) == 5
        t_frame = max(times[1:])  # the steady frames (the reset frame also pays what a first call pays)
        print(f"{_shape_id(shape)}: undelayed strip frames {['%.3f' % t for t in times]} ms, t_frame {t_frame:.3f} ms; delay step {_delayer().step_ms:.3f} ms")
        out[shape] = (want, ran, t_frame, got)
    return out


def _compare(shape, got, want):
    W, H, N, L = shape
    h = H // N
    bad = [(k, np.flatnonzero((got[k * h:(k + 1) * h] != want[k * h:(k + 1) * h]).any(axis=(1, 2))) + k * h) for k in range(N)]
    bad = [(k, rows) for k, rows in bad if rows.size]
    if bad:
        worst = float(np.abs(got.astype(np.float64) - want).max())
        msg = "; ".join(f"strip {k}: {rows.size} rows differ, image rows {rows.min()}..{rows.max()}" for k, rows in bad)
        pytest.fail(f"{_shape_id(shape)}: strips != full image -- {msg}; max |difference| {worst:.6g}", pytrace=False)
    assert np.array_equal(got, want)


def _delayed_case(shape, references, scene_and_camera, delays, order="up", share_first_two=False):
    want, ran, t_frame, _ = references[shape]
    # one unit of delay is asked for with room above the MARGIN frames that its measurement must reach
    got, _, measured = _run_strips(shape, *scene_and_camera, ran, order=order, delays=delays, delay_ms=1.5 * MARGIN * t_frame,
                                   share_first_two=share_first_two)
    assert len(measured) == len(delays)
    for units, took in measured:
        print(f"{_shape_id(shape)}: delay of {units} unit(s) measured {took:.3f} ms = {took / t_frame:.1f} x t_frame ({t_frame:.3f} ms)")
        assert took >= units * MARGIN * t_frame, (f"a delay of {units} unit(s) measured {took:.3f} ms, under {units} x {MARGIN:.0f} x t_frame "
                                                  f"({t_frame:.3f} ms): the delayed stream is not certainly the last one")
    _compare(shape, got, want)


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_undelayed_timing_run_equals_full_image(shape, references):
    """the run t_frame was taken from (a host synchronisation in front of every frame, strips on their own streams inside it)"""
    want, _, _, got = references[shape]
    _compare(shape, got, want)


@pytest.mark.parametrize("order", ["up", "down"])
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_d0_strips_on_their_own_streams_equal_full_image(shape, order, references, scene_and_camera):
    """no delay, no host synchronisation inside the run: streams only, the begin and the finish sweep in host order 0 .. N-1 and N-1 .. 0
    (the header prescribes no order inside a sweep)"""
    want, ran, _, _ = references[shape]
    got, _, _ = _run_strips(shape, *scene_and_camera, ran, order=order)
    _compare(shape, got, want)


@pytest.mark.parametrize("frame", [RESET_FRAME, STEADY_FRAME], ids=["reset_frame", "steady_frame"])
@pytest.mark.parametrize("shape,k", [(sh, k) for sh in SHAPES for k in range(sh[2])], ids=lambda v: _shape_id(v) if isinstance(v, tuple) else f"k{v}")
def test_d1_a_stream_late_before_its_strips_inputs(shape, k, frame, references, scene_and_camera):
    """stream k is late when strip k's inputs of the frame are enqueued: the neighbours' pushes into strip k's halo rows must still land behind
    strip k's own write of those rows (the direct term covers all resident rows), and strip k's late pushes in front of the neighbours' border rows"""
    _delayed_case(shape, references, scene_and_camera, {(frame, "inputs", k): 1})


@pytest.mark.parametrize("shape,k", [(sh, k) for sh in SHAPES for k in range(sh[2])], ids=lambda v: _shape_id(v) if isinstance(v, tuple) else f"k{v}")
def test_d2_a_stream_late_between_the_sweeps(shape, k, references, scene_and_camera):
    """stream k is late between the begin sweep and the finish sweep: its levels, and with them the end of its frame, come late"""
    _delayed_case(shape, references, scene_and_camera, {(STEADY_FRAME - 1, "sweeps", k): 1})


@pytest.mark.parametrize("shape,k", [(sh, k) for sh in SHAPES for k in range(sh[2])], ids=lambda v: _shape_id(v) if isinstance(v, tuple) else f"k{v}")
def test_d3_a_stream_late_behind_its_finish(shape, k, references, scene_and_camera):
    """stream k is late behind strip k's finish, before the next frame's inputs: the neighbours' next pushes wait for strip k's frame_done"""
    _delayed_case(shape, references, scene_and_camera, {(STEADY_FRAME - 1, "after", k): 1})


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_all_streams_late_by_different_amounts_every_frame(shape, references, scene_and_camera):
    """every strip delayed in every frame, by 1, 2 .. N units that rotate through the strips and at a place that rotates too; sweeps N-1 .. 0"""
    N = shape[2]
    places = ("inputs", "sweeps", "after")
    delays = {(f, places[(k + f) % 3], k): 1 + (k + 2 * f) % N for f in FRAMES for k in range(N)}
    _delayed_case(shape, references, scene_and_camera, delays, order="down")


@pytest.mark.parametrize("order", ["up", "down"])
@pytest.mark.parametrize("k", [0, 2])
def test_two_strips_on_one_stream_beside_a_third_on_its_own(k, order, references, scene_and_camera):
    """strips 0 and 1 share a stream, strip 2 has its own: the edge 0|1 is ordered by the stream, the edge 1|2 by events, whichever of the two
    streams is late in front of its inputs"""
    _delayed_case(SHAPES[0], references, scene_and_camera, {(RESET_FRAME, "inputs", k): 1, (STEADY_FRAME, "inputs", k): 1}, order=order, share_first_two=True)


def test_calls_out_of_order_are_refused_before_anything_is_enqueued(references, scene_and_camera):
    """every strip begins, then every strip finishes: a finish without its begin, a finish before a neighbour's begin and a second begin return
    NEB_ERR_STATE with a message, and the run they were made in still equals the full image"""
    shape = SHAPES[0]
    want, ran, _, _ = references[shape]
    got, _, _ = _run_strips(shape, *scene_and_camera, ran, violate=True)
    _compare(shape, got, want)
