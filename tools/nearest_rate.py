"""Rates of dr_query_nearest on the GPU (profiles/nearest_rate.txt):   python tools/nearest_rate.py [--queries 4194304] [--grid 160] [--udf out.npy]
The bench scene, device pointers, HIP events (torch.cuda.Event on the library's stream), one warm-up and the best of five per figure, for two
distributions of query points:
  near   points within a few triangle sizes of the surface (a random surface point pushed off by up to three times its triangle's extent)
  grid   a regular voxel grid over the scene's bounds, x fastest
For each: queries/s with distance + object and with every channel (walk + finishing pass), and -- on the host build of the same walk, a sample of the
points -- the records visited per query.  The baseline beside them: hk_nearest_brute, the minimum over every primitive, on 16 CPU threads.
--udf writes the grid's unsigned distances as a float32 .npy of shape [grid, grid, grid] (z, y, x)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import bench
import dogeray_amd as dr
import host_kernel as hk

ap = argparse.ArgumentParser()
ap.add_argument("--queries", type=int, default=1 << 22)
ap.add_argument("--grid", type=int, default=160)
ap.add_argument("--sample", type=int, default=20000, help="points per distribution walked on the host for the records per query")
ap.add_argument("--brute", type=int, default=512, help="points of the brute-force baseline")
ap.add_argument("--udf", default=None)
args = ap.parse_args()

W, H = 1920, 1080
path = bench.ensure_scene(os.environ.get("DOGERAY_BENCH_CACHE", "/tmp/dogeray_bench"), 709, W, H)
sc = dr.Scene.load(path, "")
sc.build_bvh()
ctx = dr.Context(0).upload(sc)
hs = hk.Scene(path)
rec = hs.nearest_prims()
tri = np.nonzero(rec["kind"] == 1)[0]
a, b, c = rec["a"][tri].astype(np.float64), rec["b"][tri].astype(np.float64), rec["c"][tri].astype(np.float64)
lo, hi = np.minimum(a, np.minimum(a + b, a + c)).min(axis=0), np.maximum(a, np.maximum(a + b, a + c)).max(axis=0)
print("bench scene: %d primitives (%d triangles), bounds %s .. %s, Lmax %.4f, %d records in the wide tree" %
      (len(rec["kind"]), len(tri), np.round(lo, 3).tolist(), np.round(hi, 3).tolist(), rec["lmax"], hs.nearest_records(2, 2)))

rng = np.random.default_rng(7)
n = args.queries
idx = rng.integers(0, len(tri), n)
u, v = rng.random((n, 1)), rng.random((n, 1))
flip = u + v > 1
u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
ext = np.linalg.norm(b[idx], axis=1, keepdims=True) + np.linalg.norm(c[idx], axis=1, keepdims=True)
dirn = rng.normal(size=(n, 3)); dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
near = (a[idx] + u * b[idx] + v * c[idx] + dirn * ext * rng.uniform(0, 3, (n, 1))).astype(np.float32)
g = args.grid
ax = [np.linspace(lo[k], hi[k], g) for k in range(3)]
zz, yy, xx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
grid = np.ascontiguousarray(np.stack([xx, yy, zz], axis=-1).reshape(-1, 3).astype(np.float32))

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


for name, pts in (("near", near), ("grid", grid)):
    tp = torch.from_numpy(pts).to(dev)
    m = len(pts)
    ms2 = timed(lambda: ctx.nearest(tp))
    ms6 = timed(lambda: ctx.nearest(tp, channels=tuple(dr.NEAREST_CHANNELS)))
    pick = rng.permutation(m)[:args.sample]
    t0 = time.time()
    host = hs.nearest(pts[pick], walk=2, tree=2, channels=("distance", "object"), want_visits=True, nthreads=16)
    host_s = time.time() - t0
    got = ctx.nearest(pts[pick])
    same = np.array_equal(got["distance"].view(np.uint32), host["distance"].view(np.uint32)) and np.array_equal(got["object"], host["object"])
    print("%-4s %9d queries: distance + object %.3f ms = %.1f Mqueries/s; every channel %.3f ms = %.1f Mqueries/s; host build, %d of them on 16 threads: "
          "%.1f records per query (max %d), %.3f Mqueries/s, GPU answers %s" %
          (name, m, ms2, m / ms2 / 1e3, ms6, m / ms6 / 1e3, len(pick), host["visits"].mean(), host["visits"].max(), len(pick) / host_s / 1e6,
           "identical" if same else "DIFFER"))
    if name == "grid" and args.udf:
        np.save(args.udf, ctx.nearest(tp, channels=("distance",))["distance"].cpu().numpy().reshape(g, g, g))
        print("wrote %s" % args.udf)

pb = near[:args.brute]
t0 = time.time()
ref = hs.nearest_brute(pb, channels=("distance", "object"), nthreads=16)
bs = time.time() - t0
got = ctx.nearest(pb)
print("baseline: hk_nearest_brute, %d near points x %d primitives on 16 CPU threads: %.2f s = %.1f queries/s; GPU answers %s" %
      (len(pb), len(rec["kind"]), bs, len(pb) / bs,
       "identical" if np.array_equal(got["distance"].view(np.uint32), ref["distance"].view(np.uint32)) and np.array_equal(got["object"], ref["object"]) else "DIFFER"))
ctx.close()
