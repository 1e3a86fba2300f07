"""Rates of dr_trace_radiance on the GPU (profiles/radiance_rate.txt):   python tools/radiance_rate.py
The bench scene at 1920x1080, spp 1, the scene's depth, device pointers, HIP events (torch.cuda.Event on the library's stream); per figure one warm-up
and seven timed runs, the two kernels alternating run by run: the median and [min .. max].
  (a) the frame's own camera rays (dr_context_probe_rays' first W * H rays) through both kernels: paths/s, and rays/s from the summed `bounces`
  (b) the same for lists of 2^16, 2^20, 2^22 and 2^24 rays (the camera rays repeated; ray i draws from seed + i, so no two paths are the same):
      the cross-over is launch_plan.hpp RADIANCE_PERSISTENT_MIN_RAYS
  (c) the yardstick: dr_render_accumulate of one frame of the same view in the same process, its rays from the probe's count
  (d) as (b) for rays that start on the scene's surfaces (the probe's rays behind the camera rays): a lightmap's or an irradiance probe's rays"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
import dogeray_amd as dr

W, H = 1920, 1080
REPS = 7
path = bench.ensure_scene(os.environ.get("DOGERAY_BENCH_CACHE", "/tmp/dogeray_bench"), 709, W, H)
sc = dr.Scene.load(path, "")
sc.build_bvh()
s = sc.settings()
ctx = dr.Context(0).upload(sc)
st = dr.pack_settings13(s, 1, spp=1)
depth, backtex = int(st[9]), int(st[12])
dev = torch.device("cuda", 0)
lib_stream = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev)


def once(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(lib_stream)
    f()
    e1.record(lib_stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(fs):
    """ms per function of fs, alternating: a list of REPS times each, after one warm-up each"""
    for f in fs:
        once(f)
    out = [[] for _ in fs]
    for _ in range(REPS):
        for k, f in enumerate(fs):
            out[k].append(once(f))
    return out


def show(ms):
    return "%.3f ms [%.3f .. %.3f]" % (statistics.median(ms), min(ms), max(ms))


def both(o, d):
    def run(force):
        ctx.set_option("radiance_kernel", force)
        ctx.radiance(o, d, 1, depth, s.background, backtex, seed=1)
    return timed([lambda: run(1), lambda: run(2)])


o_all, d_all = ctx.probe_rays(st, W, H, s.background, 1)
n_frame_rays, npix = len(o_all), W * H
o1, d1 = np.ascontiguousarray(o_all[:npix]), np.ascontiguousarray(d_all[:npix])
print("bench scene %dx%d, depth %d: %d camera rays, %d rays in the frame of seed 1" % (W, H, depth, npix, n_frame_rays))
o, d = torch.from_numpy(o1).to(dev), torch.from_numpy(d1).to(dev)
ctx.set_option("radiance_kernel", 1)
out = ctx.radiance(o, d, 1, depth, s.background, backtex, seed=1, channels=("radiance", "bounces"))
rays = int(out["bounces"].sum().item())
ctx.set_option("radiance_kernel", 2)
out2 = ctx.radiance(o, d, 1, depth, s.background, backtex, seed=1, channels=("radiance", "bounces"))
same = bool(torch.equal(out["radiance"].view(torch.int32), out2["radiance"].view(torch.int32)) and torch.equal(out["bounces"], out2["bounces"]))
print("(a) %d paths make %d rays (%.2f per path); the two kernels' results are %s" % (npix, rays, rays / npix, "identical" if same else "DIFFERENT"))
plain, pers = both(o, d)
for name, ms in (("one ray per lane", plain), ("persistent", pers)):
    m = statistics.median(ms)
    print("(a) %-16s %s: %.1f Mpaths/s, %.3f Grays/s" % (name, show(ms), npix / m / 1e3, rays / m / 1e6))
print("(a) persistent against one ray per lane: x %.2f" % (statistics.median(plain) / statistics.median(pers)))



def lengths(part, what, o_np, d_np):
    cross = None
    for k in (16, 20, 22, 24):
        m = 1 << k
        reps = (m + len(o_np) - 1) // len(o_np)
        om, dm = torch.from_numpy(np.tile(o_np, (reps, 1))[:m]).to(dev), torch.from_numpy(np.tile(d_np, (reps, 1))[:m]).to(dev)
        plain, pers = both(om, dm)
        ratio = statistics.median(plain) / statistics.median(pers)
        print("(%s) %s, n = 2^%d = %8d: one ray per lane %s, persistent %s (x %.2f)" % (part, what, k, m, show(plain), show(pers), ratio))
        if ratio >= 1.0 and cross is None:
            cross = m
        if ratio < 1.0:
            cross = None
        del om, dm
    print("(%s) %s: the persistent kernel is no slower from n = %s on" % (part, what, cross))


lengths("b", "camera rays", o1, d1)
# (d) beyond what the yardstick can render: rays that START ON THE SURFACES -- the frame's scattered rays, the probe's rays behind the camera rays --,
# what a lightmap or an irradiance probe sends
o2, d2 = np.ascontiguousarray(o_all[npix:]), np.ascontiguousarray(d_all[npix:])
lengths("d", "rays from the surfaces", o2, d2)
ctx.set_option("radiance_kernel", 0)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_kernel
print("launch_plan.hpp at the time of this run: RADIANCE_PERSISTENT_MIN_RAYS = %d, refill at %d lanes, leaf steps for %d, chunks of %d rays, %d waves per SIMD" % (
    host_kernel.radiance_persistent_min_rays(), host_kernel.radiance_refill_min(), host_kernel.radiance_park(), host_kernel.radiance_chunk(), host_kernel.radiance_occ()))

ctx.accum_reset(W, H)
frame = timed([lambda: ctx.render_accumulate(st, W, H, s.background, 1, 1000003, 1)])[0]
m = statistics.median(frame)
print("(c) dr_render_accumulate, one frame of the same view: %s: %.1f Mpaths/s, %.3f Grays/s" % (show(frame), npix / m / 1e3, n_frame_rays / m / 1e6))
ctx.close()
