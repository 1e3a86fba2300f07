"""The pipelined present loop's two contracts (include/dogeray_amd.h, dr_pipeline_submit / dr_pipeline_wait), on frames that are still HELD --
submitted, their group not launched yet -- when something else happens on the context:

  1. a frame is rendered with the state it was submitted under: a scene upload, a stripe, a traversal, the counters switch or an option that
     arrives later applies to the frames submitted after it, and every other call is ordered behind the frames submitted before it;
  2. a ticket handed out by dr_pipeline_submit can be waited for, and dr_pipeline_wait(ticket) returns exactly
     clamp(sum of the frames <= ticket / present_divide_by, 0, 255), however many groups have been launched since.

Expected values never come from the pipeline: a frame is `ref.render_frame` of a second Context that never submits (holding the scene and the
stripe the frame was SUBMITTED under), frames are summed in int64 and a ticket's image is clip(trunc(sum / div), 0, 255) transposed to row-major,
as test_pipelined_present_loop computes it.  Scenario 1 takes its frames from the oracle instead, so one scenario rests on nothing in the product.
Every comparison is integer equality; nothing sleeps or is timed.

96 x 64 frames (not square: a transposition shows), 1 spp, depth as the scene says, pipe_group = 8, pipe_streams = 2.  Every scenario asserts its
preconditions first and proves from the launches / frames of stats() at its end that frames really were held: a group of 3 counted as ONE launch
was not launched frame by frame.  The counters switch has no getter: this file switches it only through _counters(), which remembers it, and a
group counted as one launch is itself the proof that it was off (a counting launch holds one frame)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import CUBE_SETTINGS, SCENEGEN, SCENES, with_settings

pytestmark = pytest.mark.gpu

W, H = 96, 64
STRIDE = 1000003
SEED = 41
TILES = (W // 8) * (H // 8)
ERR_INVALID = -1
THREADED, WIDE = 0, 2
RESTORE = (("schedule", 0), ("occupancy", 6), ("kernel", 1), ("pipe_lean", 0), ("pipe_group", 8), ("moments", 0))


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    return dogeray_amd


@pytest.fixture(scope="module")
def world(dr, tmp_path_factory):
    """the Context under test and `ref`, a second one that never submits a frame; two scenes without textures ("A" the cube, "B" a height field),
    each with its view and background; frames rendered by `ref` are kept (frame())"""
    from oracle import orc
    d = tmp_path_factory.mktemp("contracts")
    paths = {"A": with_settings(os.path.join(SCENES, "cube.rts"), str(d / "cube.rts"), CUBE_SETTINGS), "B": str(d / "hf_small.rts")}
    subprocess.check_call([SCENEGEN, "heightfield", paths["B"], "71", "320", "192"])
    w = {"dr": dr, "orc": orc, "paths": paths, "scene": {}, "st": {}, "bg": {}, "frames": {}, "counting": False}
    for key, path in paths.items():
        sc = dr.Scene.load(path, "")
        sc.build_bvh()
        s = sc.settings()
        assert s.backtex == -1 and not sc.textures(), "scene %s has textures" % key
        w["scene"][key], w["st"][key], w["bg"][key] = sc, dr.pack_settings13(s, 1, spp=1), s.background
    w["ctx"], w["ref"] = dr.Context(0), dr.Context(0)
    for c in (w["ctx"], w["ref"]):
        c.upload(w["scene"]["A"])
        c.set_option("pipe_streams", 2)
    w["ctx_scene"], w["ref_scene"], w["ref_stripe"] = "A", "A", (1, 0)
    yield w
    w["ctx"].close()
    w["ref"].close()


def _counters(world, on):
    world["ctx"].enable_counters(on)
    world["counting"] = bool(on)


@pytest.fixture()
def ctx(world):
    """the Context under test with an empty accumulator of W x H and statistics at 0; afterwards every option, the stripe, the traversal, the
    counters switch and the scene are put back, and the pipeline's ticket numbering starts again (option pipe_streams: a test that failed half way
    leaves no ticket behind)"""
    c = world["ctx"]
    try:
        c.accum_reset(W, H)
        c.stats_reset()
        yield c
    finally:
        for name, value in RESTORE:
            c.set_option(name, value)
        c.set_stripe(1, 0)
        c.set_traversal(WIDE)
        _counters(world, False)
        if world["ctx_scene"] != "A":
            c.upload(world["scene"]["A"])
            world["ctx_scene"] = "A"
        c.set_option("pipe_streams", 3)
        c.set_option("pipe_streams", 2)


def _preconditions(world, c):
    assert c.get_option("traversal") == WIDE
    assert c.get_option("pipe_group") == 8 and c.get_option("pipe_streams") == 2 and c.get_option("pipe_lean") == 0
    assert c.get_option("schedule") == 0 and c.get_option("occupancy") == 6 and c.get_option("kernel") == 1
    assert world["counting"] is False
    s = c.stats()
    assert s["frames"] == 0 and s["launches"] == 0


def frame(world, scene, st, seed, stripe=(1, 0)):
    """the frame `ref` renders of this scene, view, seed and stripe, as int64[W, H, 3]; rendered once"""
    key = (scene, stripe, np.asarray(st, dtype=np.float32).tobytes(), seed)
    if key not in world["frames"]:
        ref = world["ref"]
        if world["ref_scene"] != scene:
            ref.upload(world["scene"][scene])
            world["ref_scene"] = scene
        if world["ref_stripe"] != stripe:
            ref.set_stripe(*stripe)
            world["ref_stripe"] = stripe
        f = ref.render_frame(st, W, H, world["bg"][scene], seed).astype(np.int64)
        f.flags.writeable = False
        world["frames"][key] = f
    return world["frames"][key]


def image(total, div):
    """what dr_pipeline_wait hands out for these sums: C's integer division truncates toward zero; row-major"""
    quot = (np.abs(total) // div) * np.sign(total)
    return np.clip(quot, 0, 255).astype(np.uint8).transpose(1, 0, 2)


def _seeds(n, first=SEED):
    return [first + k * STRIDE for k in range(n)]


def _submit(world, c, scene, seeds, st=None, presents=True, first_div=1):
    """submits one frame per seed (frame k presented with divisor first_div + k); the tickets"""
    st = world["st"][scene] if st is None else st
    return [c.pipeline_submit(st, W, H, world["bg"][scene], seed, present_divide_by=(first_div + k if presents else 0)) for k, seed in enumerate(seeds)]


def _wait_all(c, tickets, frames, total=None, first_div=1):
    """waits for every ticket in order with its image; each is exactly the image of the frames so far.  Returns the sums."""
    total = np.zeros((W, H, 3), dtype=np.int64) if total is None else total.copy()
    for k, (t, f) in enumerate(zip(tickets, frames)):
        total = total + f
        got = c.pipeline_wait(t, want_image=True)
        want = image(total, first_div + k)
        assert np.array_equal(got, want), "image of ticket %d (frame %d): %d pixels differ" % (t, k, int((got != want).any(axis=2).sum()))
    return total


def _assert_sums(c, total, what):
    got = c.accum_read().astype(np.int64)
    assert np.array_equal(got, total), "%s: the accumulator differs from the sum of the frames at %d pixels" % (what, int((got != total).any(axis=2).sum()))


def _assert_counts(c, frames, launches):
    s = c.stats()
    assert (s["frames"], s["launches"]) == (frames, launches), "%d frames in %d launches, not %d in %d" % (s["frames"], s["launches"], frames, launches)


def test_scene_upload_applies_to_frames_submitted_after_it(world, ctx):
    """1.  Three held frames of scene A, an upload of scene B, two frames of B: the sum of the ORACLE's three A frames and two B frames."""
    _preconditions(world, ctx)
    want = np.zeros((W, H, 3), dtype=np.int64)
    for key, n in (("A", 3), ("B", 2)):
        os_ = world["orc"].Scene(world["paths"][key], None)
        os_.build_bvh()
        for seed in _seeds(n):
            f, _ = os_.render(world["st"][key], W, H, world["bg"][key], seed, nthreads=4)
            assert np.array_equal(f, frame(world, key, world["st"][key], seed)), "scene %s seed %d: the frame of `ref` is not the oracle's" % (key, seed)
            want += f
        os_.close()
    _submit(world, ctx, "A", _seeds(3), presents=False)
    ctx.upload(world["scene"]["B"])
    world["ctx_scene"] = "B"
    _submit(world, ctx, "B", _seeds(2), presents=False)
    _assert_sums(ctx, want, "3 frames of A, upload of B, 2 frames of B")
    _assert_counts(ctx, 5, 2)


def test_stripe_applies_to_frames_submitted_after_it(world, ctx):
    """2.  Three held frames under stripe (1, 0), set_stripe(2, 1), three more: three whole frames and three striped ones, every ticket's image."""
    _preconditions(world, ctx)
    st = world["st"]["A"]
    frames = [frame(world, "A", st, seed) for seed in _seeds(3)] + [frame(world, "A", st, seed, (2, 1)) for seed in _seeds(6)[3:]]
    assert frames[3].any() and not np.array_equal(frames[3], frame(world, "A", st, _seeds(6)[3])), "the stripe hides nothing"
    tickets = _submit(world, ctx, "A", _seeds(3))
    ctx.set_stripe(2, 1)
    tickets += _submit(world, ctx, "A", _seeds(6)[3:], first_div=4)
    total = _wait_all(ctx, tickets, frames)
    _assert_sums(ctx, total, "3 whole frames, 3 striped ones")
    _assert_counts(ctx, 6, 2)


CHANGES = [
    ("schedule=1", lambda w, c: c.set_option("schedule", 1)),
    ("occupancy=5", lambda w, c: c.set_option("occupancy", 5)),
    ("kernel=tile", lambda w, c: c.set_option("kernel", 0)),
    ("pipe_lean=1", lambda w, c: c.set_option("pipe_lean", 1)),
    ("pipe_group=1", lambda w, c: c.set_option("pipe_group", 1)),
    ("pipe_group=3", lambda w, c: c.set_option("pipe_group", 3)),
    ("traversal=threaded", lambda w, c: c.set_traversal(THREADED)),
    ("counters=on", lambda w, c: _counters(w, True)),
]


@pytest.mark.parametrize("change", [c[1] for c in CHANGES], ids=[c[0] for c in CHANGES])
def test_group_size_options_keep_every_ticket(world, ctx, change):
    """3.  Seven held frames with presents, then a change that takes the grouped launch away: the seven are ONE launch under the configuration
    they were submitted with, and tickets 0 .. 6 are waited for in order, each with its exact image."""
    _preconditions(world, ctx)
    st = world["st"]["A"]
    frames = [frame(world, "A", st, seed) for seed in _seeds(7)]
    tickets = _submit(world, ctx, "A", _seeds(7))
    change(world, ctx)
    total = _wait_all(ctx, tickets, frames)
    _assert_sums(ctx, total, "7 frames")
    _assert_counts(ctx, 7, 1)


def test_statistics_see_held_and_running_frames(world, ctx):
    """4.  stats() counts frames that were still held, and the device counters of launches running on the pipeline's other streams."""
    _preconditions(world, ctx)
    st, bg = world["st"]["A"], world["bg"]["A"]
    _submit(world, ctx, "A", _seeds(3), presents=False)
    s = ctx.stats()
    assert (s["frames"], s["launches"], s["samples"]) == (3, 1, 3 * TILES * 64), s
    _assert_sums(ctx, sum(frame(world, "A", st, seed) for seed in _seeds(3)), "3 frames")
    # with counters: four frames are four launches on alternating streams; the counts are those of the same frames rendered on `ref`
    ref = world["ref"]
    assert world["ref_scene"] == "A" and world["ref_stripe"] == (1, 0)
    try:
        ref.enable_counters(True)
        ref.set_traversal(THREADED)
        ref.accum_reset(W, H)
        ref.stats_reset()
        ref.render_accumulate(st, W, H, bg, SEED, STRIDE, 4)
        want = ref.stats()
    finally:
        ref.enable_counters(False)
        ref.set_traversal(WIDE)
    assert want["rays"] >= 4 * TILES * 64 and want["node_visits"] > 0 and want["prim_tests"] > 0 and want["shades"] > 0, want
    _counters(world, True)
    ctx.set_traversal(THREADED)
    ctx.stats_reset()
    _submit(world, ctx, "A", _seeds(4), presents=False)
    got = ctx.stats()
    for name in ("rays", "shades", "node_visits", "prim_tests"):
        assert got[name] == want[name], "%s: %d counted, %d on the reference context" % (name, got[name], want[name])
    assert got["frames"] == 4 and got["launches"] == 4, got


def test_moving_camera_keeps_every_ticket(world, ctx):
    """5.  Sixteen frames in flight, each of another view and each with a present -- sixteen groups of one for three slots: every ticket is waited
    for in order and every image is exact.  A ticket that was never handed out is still refused."""
    dr = world["dr"]
    _preconditions(world, ctx)
    views = []
    for k in range(16):
        st = world["st"]["A"].copy()
        st[0] += 0.05 * k
        views.append(st)
    seeds = _seeds(16)
    frames = [frame(world, "A", st, seed) for st, seed in zip(views, seeds)]
    tickets = [ctx.pipeline_submit(st, W, H, world["bg"]["A"], seed, present_divide_by=k + 1) for k, (st, seed) in enumerate(zip(views, seeds))]
    assert tickets == list(range(tickets[0], tickets[0] + 16))
    total = _wait_all(ctx, tickets, frames)
    _assert_sums(ctx, total, "16 views")
    _assert_counts(ctx, 16, 16)
    with pytest.raises(dr.DogerayError) as e:
        ctx.pipeline_wait(tickets[-1] + 1)
    assert e.value.code == ERR_INVALID


def _read_on_context_stream(world, c, ptr, nbytes):
    """the int32 words at a device pointer, read by torch on the context's own stream"""
    import torch
    from dogeray_amd import multigpu
    with torch.cuda.stream(world["torch_stream"]):
        return torch.as_tensor(multigpu._DevArray(ptr, nbytes // 4), device=torch.device("cuda", c.device)).cpu().numpy()


def test_device_pointers_are_ordered_behind_held_frames(world, ctx):
    """6.  dr_accum_device_ptr / dr_accum_moments_device_ptr with three frames held: work the caller orders on dr_context_stream() reads the planes
    with the three frames in them.  No library call between the pointer and the read."""
    import torch
    dr = world["dr"]
    _preconditions(world, ctx)
    st, bg = world["st"]["A"], world["bg"]["A"]
    world["torch_stream"] = torch.cuda.ExternalStream(ctx.stream_ptr(), device=torch.device("cuda", ctx.device))
    total = sum(frame(world, "A", st, seed) for seed in _seeds(3))
    _submit(world, ctx, "A", _seeds(3), presents=False)
    ptr, nbytes = ctx.accum_device_ptr()
    got = _read_on_context_stream(world, ctx, ptr, nbytes)
    assert nbytes == W * H * 3 * 4
    got = got.reshape(W, H, 3).astype(np.int64)
    assert np.array_equal(got, total), "the sums read through the pointer differ from the 3 frames at %d pixels" % int((got != total).any(axis=2).sum())
    _assert_counts(ctx, 3, 1)
    # the second-moment plane: what the same three frames, added one call at a time, leave on `ref`
    ref = world["ref"]
    assert world["ref_scene"] == "A" and world["ref_stripe"] == (1, 0)
    try:
        ref.set_option("moments", 1)
        ref.accum_reset(W, H)
        ref.accum_reset(W, H)
        for seed in _seeds(3):
            ref.render_accumulate(st, W, H, bg, seed, STRIDE, 1)
        want = ref.accum_moments()
        assert np.array_equal(ref.accum_read().astype(np.int64), total)
    finally:
        ref.set_option("moments", 0)
        ref.accum_reset(W, H)
    assert want.any()
    ctx.set_option("moments", 1)
    ctx.accum_reset(W, H)
    ctx.stats_reset()
    _submit(world, ctx, "A", _seeds(3), presents=False)
    p, n = C.c_void_p(), C.c_uint64()
    assert dr.lib().dr_accum_moments_device_ptr(ctx._h, C.byref(p), C.byref(n)) == 0
    got = _read_on_context_stream(world, ctx, p.value, int(n.value))
    assert p.value and n.value == W * H * 8
    got = got.view(np.uint64).reshape(W, H)
    assert np.array_equal(got, want), "the second moments read through the pointer differ at %d pixels" % int((got != want).sum())
    _assert_counts(ctx, 3, 1)


def test_tickets_without_presents_retire_cleanly(world, ctx):
    """7.  Twelve frames without presents across five view changes -- six groups for three slots: waiting for each ticket in order succeeds (a frame
    whose slot was reused has finished, which is no error); asking for the image of one is refused as before."""
    dr = world["dr"]
    _preconditions(world, ctx)
    plan = []
    for v in range(6):
        st = world["st"]["A"].copy()
        st[0] += 0.05 * v
        plan += [(st, seed) for seed in _seeds(2, SEED + 7 * v)]
    total = sum(frame(world, "A", st, seed) for st, seed in plan)
    tickets = [ctx.pipeline_submit(st, W, H, world["bg"]["A"], seed) for st, seed in plan]
    for t in tickets:
        assert ctx.pipeline_wait(t) is None
    for t in (tickets[0], tickets[-1]):
        with pytest.raises(dr.DogerayError) as e:
            ctx.pipeline_wait(t, want_image=True)
        assert e.value.code == ERR_INVALID and "submitted without a present" in str(e.value), str(e.value)
    _assert_sums(ctx, total, "12 frames of 6 views")
    _assert_counts(ctx, 12, 6)


def test_submit_refuses_rather_than_drop_an_image(world, ctx):
    """8.  Presented frames of alternating views that nobody waits for: the library keeps the images of at most 32 frames whose buffers it has reused
    (2 x PIPE_GROUP_MAX), so with the three groups in flight and the one frame held -- one ticket each here -- between 32 and 36 tickets can be
    outstanding.  The submit after that is refused with DR_ERR_INVALID and takes no ticket; every ticket handed out is still waited for with its
    exact image, and after the waits frames are accepted again."""
    dr = world["dr"]
    _preconditions(world, ctx)
    views = [world["st"]["A"].copy(), world["st"]["A"].copy()]
    views[1][0] += 0.05
    bg = world["bg"]["A"]
    tickets, refused = [], None
    for k, seed in enumerate(_seeds(40)):
        try:
            tickets.append(ctx.pipeline_submit(views[k % 2], W, H, bg, seed, present_divide_by=k + 1))
        except dr.DogerayError as e:
            refused = e
            break
    assert refused is not None, "40 presented frames, none waited for, and no submit refused"
    assert refused.code == ERR_INVALID and "dr_pipeline_wait" in str(refused), str(refused)
    n = len(tickets)
    assert 32 <= n <= 36, n
    frames = [frame(world, "A", views[k % 2], seed) for k, seed in enumerate(_seeds(n))]
    total = _wait_all(ctx, tickets, frames)
    t = ctx.pipeline_submit(views[n % 2], W, H, bg, _seeds(n + 1)[n], present_divide_by=n + 1)
    total = total + frame(world, "A", views[n % 2], _seeds(n + 1)[n])
    assert np.array_equal(ctx.pipeline_wait(t, want_image=True), image(total, n + 1))
    _assert_sums(ctx, total, "%d frames" % (n + 1))
    _assert_counts(ctx, n + 1, n + 1)


def _image_call(dr, c, ticket):
    """dr_pipeline_image(ticket): (return code, error text, pointer)"""
    ptr = C.c_void_p()
    rc = dr.lib().dr_pipeline_image(c._h, ticket, C.byref(ptr))
    return rc, (dr.lib().dr_last_error().decode() if rc != 0 else ""), ptr.value


def test_a_ticket_whose_slot_was_reused_keeps_its_image_and_its_order_of_calls(world, ctx):
    """9.  Five presented frames of five views -- five groups of one for three slots: the launches of tickets 3 and 4 reuse the slots of tickets 0
    and 1, whose images are kept aside.  dr_pipeline_image of such a ticket is refused before its wait, as it is for a ticket still in its slot;
    the wait then returns exactly that ticket's image, and dr_pipeline_image the same bytes."""
    dr = world["dr"]
    _preconditions(world, ctx)
    views = []
    for k in range(5):
        st = world["st"]["A"].copy()
        st[0] += 0.05 * k
        views.append(st)
    frames = [frame(world, "A", st, seed) for st, seed in zip(views, _seeds(5))]
    tickets = [ctx.pipeline_submit(st, W, H, world["bg"]["A"], seed, present_divide_by=k + 1) for k, (st, seed) in enumerate(zip(views, _seeds(5)))]
    assert tickets == [0, 1, 2, 3, 4]
    ctx.synchronize()                        # ticket 4, held, is launched: five launches
    _assert_counts(ctx, 5, 5)
    for t in (0, 1, 4):                      # two whose slot has been reused, one in its slot
        rc, text, _ = _image_call(dr, ctx, t)
        assert rc == ERR_INVALID and "dr_pipeline_wait(ticket) comes first" in text, (t, rc, text)
    totals = np.cumsum(np.stack(frames), axis=0)
    for t in (1, 0, 4):                      # in no particular order
        want = image(totals[t], t + 1)
        got = ctx.pipeline_wait(t, want_image=True)
        assert np.array_equal(got, want), "image of ticket %d: %d pixels differ" % (t, int((got != want).any(axis=2).sum()))
        rc, text, ptr = _image_call(dr, ctx, t)
        assert rc == 0 and ptr, (t, rc, text)
        again = np.frombuffer((C.c_uint8 * (W * H * 3)).from_address(ptr), dtype=np.uint8).reshape(H, W, 3)
        assert np.array_equal(again, want), "dr_pipeline_image of ticket %d" % t
    _assert_sums(ctx, totals[4], "5 views")


def test_tickets_start_again_from_0_after_pipe_streams_with_exact_images(world, ctx):
    """10.  Two held frames, then pipe_streams 2 -> 3 -> 4 -> 2 with three presented frames after each change: the change launches what is held, the
    tickets after it count from 0 again, and every image is still the exact image of all the frames so far."""
    _preconditions(world, ctx)
    st = world["st"]["A"]
    seeds = _seeds(11)
    frames = [frame(world, "A", st, seed) for seed in seeds]
    tickets = _submit(world, ctx, "A", seeds[:2])
    assert tickets == [0, 1]
    total, done = None, 0
    try:
        for streams in (3, 4, 2):
            ctx.set_option("pipe_streams", streams)
            if done == 0:
                _assert_counts(ctx, 2, 1)    # the two held frames: ONE launch, under the numbering they were submitted in
                total = frames[0] + frames[1]
                done = 2
            tickets = _submit(world, ctx, "A", seeds[done:done + 3], first_div=done + 1)
            assert tickets == [0, 1, 2], (streams, tickets)
            total = _wait_all(ctx, tickets, frames[done:done + 3], total, first_div=done + 1)
            done += 3
    finally:
        ctx.set_option("pipe_streams", 2)
    _assert_sums(ctx, total, "11 frames across three changes of pipe_streams")
    _assert_counts(ctx, 11, 4)
