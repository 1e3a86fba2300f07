"""Rates of dr_trace_all_hits on the GPU (profiles/allhits_rate.txt):   python tools/allhits_rate.py [--out profiles/allhits_rate.txt] [--sample 20000]
The 1M-triangle bench scene, the rays of one real frame in wavefront order (dr_context_probe_rays), device pointers, HIP events (torch.cuda.Event on
the library's stream), one warm-up and the best of five per figure, everything in one run:
  (a) the count only (max_hits 0) and K = 4 (count + t + object), one ray per lane against the persistent kernel, on one frame's rays
  (b) on the same rays: Context.trace closest hit (t + object), and the peeling loop that dr_trace_all_hits replaces -- four rounds of closest hit
      with the origin advanced to the hit
  (c) one ray per lane against persistent over prefixes and copies of the list: where launch_plan.hpp ALLHITS_PERSISTENT_MIN_RAYS comes from
  (d) records visited per ray by the un-pruned walk beside the closest-hit walk's, from the host build of both on a sample of the rays, and whether
      the GPU's answers on that sample are the host build's"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import bench
import dogeray_amd as dr
import host_kernel as hk

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "allhits_rate.txt"))
ap.add_argument("--sample", type=int, default=20000, help="rays walked on the host for the records per ray")
ap.add_argument("--copies", type=int, default=16, help="largest multiple of the frame's rays in part (c)")
args = ap.parse_args()

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


W, H = 1920, 1080
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
n = len(o1)
o, d = torch.from_numpy(o1).to(dev), torch.from_numpy(d1).to(dev)
say("bench scene %dx%d, one frame: %d rays in wavefront order" % (W, H, n))

KERNELS = ((1, "one ray per lane"), (2, "persistent"))
for K, chan, what in ((0, ("count",), "count only (K = 0)"), (4, ("count", "t", "object"), "K = 4, count + t + object")):
    for force, name in KERNELS:
        ctx.set_option("allhits_kernel", force)
        ms = timed(lambda: ctx.trace_all(o, d, None, K, channels=chan))
        say("(a) all hits, %-26s %-16s %.3f ms = %.3f Grays/s" % (what + ",", name, ms, n / ms / 1e6))
ctx.set_option("allhits_kernel", 1)
ms = timed(lambda: ctx.trace_all(o, d, None, 4, channels=tuple(dr.ALLHITS_CHANNELS)))
say("(a) all hits, K = 4, every channel (walk + surface pass), one ray per lane: %.3f ms = %.3f Grays/s" % (ms, n / ms / 1e6))
cnt = ctx.trace_all(o, d, None, 0, channels=("count",))["count"]
torch.cuda.synchronize()
hist = torch.bincount(cnt.clamp(max=9).long(), minlength=10).cpu().numpy()
say("(a) crossings per ray: mean %.3f, max %d; rays with 0, 1, .. 8, 9+ crossings: %s" % (float(cnt.float().mean()), int(cnt.max()), hist.tolist()))

ctx.set_option("trace_kernel", 0)
ms_closest = timed(lambda: ctx.trace(o, d))
say("(b) closest hit (Context.trace, t + object): %.3f ms = %.3f Grays/s" % (ms_closest, n / ms_closest / 1e6))


def peel(rounds=4):
    oo = o
    for _ in range(rounds):
        with torch.cuda.stream(lib_stream):
            t = ctx.trace(oo, d, channels=("t",))["t"]
            oo = torch.where((t > 0)[:, None], oo + t[:, None] * d, oo)
    return oo


ms_peel = timed(peel)
say("(b) peeling, 4 rounds of closest hit with the origin advanced to the hit: %.3f ms = %.3f Grays/s per original ray" % (ms_peel, n / ms_peel / 1e6))

say("(c) K = 4 (count + t + object) and the count only, one ray per lane against persistent:")
cross = None
sizes = [1 << k for k in range(14, 31, 2) if (1 << k) < n] + [n] + [n * c for c in (4, args.copies) if c > 1]
for m in sizes:
    reps = (m + n - 1) // n
    om = (o.repeat(reps, 1) if reps > 1 else o)[:m].contiguous()
    dm = (d.repeat(reps, 1) if reps > 1 else d)[:m].contiguous()
    row = []
    for K, chan in ((4, ("count", "t", "object")), (0, ("count",))):
        for force, _ in KERNELS:
            ctx.set_option("allhits_kernel", force)
            row.append(timed(lambda: ctx.trace_all(om, dm, None, K, channels=chan)))
    say("(c) n = %9d: K = 4 one ray per lane %.4f ms, persistent %.4f ms (x %.2f); count only %.4f ms, %.4f ms (x %.2f)" %
        (m, row[0], row[1], row[0] / row[1], row[2], row[3], row[2] / row[3]))
    if row[1] <= row[0] and cross is None:
        cross = m
    if row[1] > row[0]:
        cross = None
    del om, dm
ctx.set_option("allhits_kernel", 0)
say("(c) K = 4: the persistent kernel is no slower from n = %s on" % cross)

rng = np.random.default_rng(5)
pick = np.sort(rng.permutation(n)[:args.sample])
hs = hk.Scene(path)
os_, ds_ = np.ascontiguousarray(o1[pick]), np.ascontiguousarray(d1[pick])
host = hs.allhits(os_, ds_, None, 4, 3, 2, 2, want_visits=True, nthreads=16)
closest = hs.trace(os_, ds_, None, 2, 2, want_visits=True)
got = ctx.trace_all(os_, ds_, None, 4)
same = all(np.array_equal(got[k].view(np.uint32), host[k].view(np.uint32)) for k in ("count", "t", "object"))
say("(d) host build, %d of the rays: the un-pruned walk visits %.1f records per ray (max %d), the closest-hit walk %.1f (max %d): x %.2f; "
    "GPU answers on the sample %s" % (len(pick), host["visits"].mean(), host["visits"].max(), closest["visits"].mean(), closest["visits"].max(),
                                      host["visits"].mean() / closest["visits"].mean(), "identical" if same else "DIFFER"))
ctx.close()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
