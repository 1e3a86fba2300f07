"""Rates of dr_trace_rays on the GPU (profiles/trace_rays_rate.txt):   python tools/trace_rate.py [copies=20]
The rays of one real frame of the bench scene in wavefront order (dr_context_probe_rays: what the trace-only probe walks), device pointers, HIP events
(torch.cuda.Event on the library's stream), one warm-up and the best of five per figure.
  (a) closest hit, tmax NULL, t and object written, `copies` copies of the frame's rays, against dr_context_probe_trace's own rate on the same rays
      (variant 2, the persistent kernel's parameters; variant 0, one ray per lane)
  (b) occlusion against closest on the same rays: tmax NULL, then tmax = the ray's own closest t times 0.5, 1 and 2 (misses: NULL's 10000)
  (c) the one-ray-per-lane kernel against the persistent kernel over prefixes of the list: the cross-over is launch_plan.hpp TRACE_PERSISTENT_MIN_RAYS"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
import dogeray_amd as dr

W, H = 1920, 1080
copies = int(sys.argv[1]) if len(sys.argv) > 1 else 20
path = bench.ensure_scene(os.environ.get("DOGERAY_BENCH_CACHE", "/tmp/dogeray_bench"), 709, W, H)
sc = dr.Scene.load(path, "")
sc.build_bvh()
s = sc.settings()
ctx = dr.Context(0).upload(sc)
st = dr.pack_settings13(s, 1, spp=1)
dev = torch.device("cuda", 0)
lib_stream = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev)


def timed(f, reps=5):
    """best of reps, in ms, on the library's stream; one warm-up"""
    best = 1e30
    for k in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(lib_stream)
        f()
        e1.record(lib_stream)
        e1.synchronize()
        if k > 0:
            best = min(best, e0.elapsed_time(e1))
    return best


o1, d1 = ctx.probe_rays(st, W, H, s.background, 1)
n1 = len(o1)
print("bench scene %dx%d, one frame: %d rays in wavefront order; %d copies = %d rays per timed launch" % (W, H, n1, copies, n1 * copies))
for v in (2, 0):
    r, n, bad = ctx.probe_trace(st, W, H, s.background, 1, copies, v)
    print("(a) dr_context_probe_trace variant %d (%s): %.3f Grays/s, %d results differ from one ray per lane" % (v, "persistent 6/8/20" if v == 2 else "one ray per lane", r / 1e9, bad))
    if v == 2:
        probe_rate = r
o, d = torch.from_numpy(np.tile(o1, (copies, 1))).to(dev), torch.from_numpy(np.tile(d1, (copies, 1))).to(dev)
n = o.shape[0]
for force, name in ((2, "persistent"), (1, "one ray per lane")):
    ctx.set_option("trace_kernel", force)
    ms = timed(lambda: ctx.trace(o, d))
    print("(a) dr_trace_rays closest, tmax NULL, t + object, %s kernel: %.3f Grays/s (%.3f ms)%s" % (name, n / ms / 1e6, ms, " = %.3f of the probe's variant 2" % (n / ms * 1e3 / probe_rate) if force == 2 else ""))
ctx.set_option("trace_kernel", 2)
ms = timed(lambda: ctx.trace(o, d, channels=("t",)))
print("(a) ... t only: %.3f Grays/s; bytes per ray: the probe reads 32 and writes 8, dr_trace_rays reads 24 and writes 8 (t + object) or 4 (t)" % (n / ms / 1e6))
ms = timed(lambda: ctx.trace(o, d, channels=("t", "object", "material", "distance", "normal", "uv", "albedo")))
print("(a) ... every channel (trace + surface pass): %.3f Grays/s" % (n / ms / 1e6))

t = ctx.trace(o, d, channels=("t",))["t"]
torch.cuda.synchronize()
hit = t > 0
print("(b) %.3f of the rays hit" % float(hit.float().mean()))
for label, tmax in (("NULL", None), ("0.5 t", torch.where(hit, t * 0.5, torch.full_like(t, 10000.0))), ("1 t", torch.where(hit, t, torch.full_like(t, 10000.0))),
                    ("2 t", torch.where(hit, t * 2.0, torch.full_like(t, 10000.0)))):
    if tmax is not None:
        tmax = tmax.contiguous()
    torch.cuda.synchronize()
    for force, name in ((2, "persistent"), (1, "one ray per lane")):
        ctx.set_option("trace_kernel", force)
        mc = timed(lambda: ctx.trace(o, d, tmax, channels=("t",)))
        ma = timed(lambda: ctx.trace(o, d, tmax, any_hit=True))
        occ = float(ctx.trace(o, d, tmax, any_hit=True)["occluded"].float().mean())
        print("(b) tmax %-5s %-16s closest %.3f Grays/s, any-hit %.3f Grays/s (x %.2f), %.3f occluded" % (label, name, n / mc / 1e6, n / ma / 1e6, mc / ma, occ))

print("(c) tmax NULL, prefixes of the list, closest (t + object) and any-hit:")
sizes = [1 << k for k in range(10, 31, 2) if (1 << k) < n] + [n // 4 * 3, n]
cross = None
for m in sorted(set(sizes)):
    om, dm = o[:m].contiguous(), d[:m].contiguous()
    row = []
    for any_hit in (False, True):
        ctx.set_option("trace_kernel", 1)
        plain = timed(lambda: ctx.trace(om, dm, any_hit=any_hit), reps=7)
        ctx.set_option("trace_kernel", 2)
        pers = timed(lambda: ctx.trace(om, dm, any_hit=any_hit), reps=7)
        row += [plain, pers, plain / pers]
    print("(c) n = %9d: closest one ray per lane %.4f ms, persistent %.4f ms (x %.2f); any-hit %.4f ms, %.4f ms (x %.2f)" % ((m,) + tuple(row)))
    if row[1] <= row[0] and cross is None:
        cross = m
    if row[1] > row[0]:
        cross = None
ctx.set_option("trace_kernel", 0)
print("(c) the persistent kernel is no slower from n = %s on" % cross)
ctx.close()
