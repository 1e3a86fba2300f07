"""The camera rays' entry table priced on the host (no GPU; DESIGN.md 4.10, option camera_entry): records per ray of the bench view with and without
the table, over the library's own device code compiled for the CPU (tools/host_kernel.cpp), on sampled block columns of the C4 stand-in at 1920x1080.
   python tools/exp_camera_entry.py [col_mod [frames]]        (default: every 8th block column, 2 frames)
Prints the tiles' depth histogram (records between the root and the entry) and V per ray; the lines go into profiles/camera_entry_ab.txt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

import bench
import host_kernel as hk
import dogeray_amd as dr

W, H = 1920, 1080
col_mod = int(sys.argv[1]) if len(sys.argv) > 1 else 8
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 2
path = bench.ensure_scene(os.environ.get("DOGERAY_BENCH_CACHE", "/tmp/dogeray_bench"), 709, W, H)
sc = dr.Scene.load(path, "")
s = sc.settings()
st = dr.pack_settings13(s, 1, spp=1)
hs = hk.Scene(path, "")
ncpu = len(os.sched_getaffinity(0))
table = hs.camera_entry(st, W, H, col_mod, 0)
assert table is not None, "the bench view gives no table"
codes, c = table
geo = c["tiles"] - c["none"]
print("C4 stand-in %dx%d, every %d-th block column: %d tiles, %d see no leaf (ENTRY_NONE), %d at the root, %d at a leaf record; every-tile flag %d; %d leaves" %
      (W, H, col_mod, c["tiles"], c["none"], c["root"], c["leaf"], c["every"], c["leaves"]))
print("tiles per depth of the entry below the root (0 = root): %s" % c["depth"])
print("mean depth over the tiles that see geometry: %.2f" % (sum(d * n for d, n in enumerate(c["depth"])) / max(1, geo)))
tot = {"off": [0, 0], "on": [0, 0]}
for f in range(frames):
    seed = 1 + (4 + f) * 1000003          # the timed region's first frames (bench.py: seed_base + (warmup + f) * seed_stride)
    a, ca = hs.render(st, W, H, s.background, seed, traversal=2, nthreads=ncpu, col_mod=col_mod, col_rem=0, entry_plane=np.zeros_like(codes))
    b, cb = hs.render(st, W, H, s.background, seed, traversal=2, nthreads=ncpu, col_mod=col_mod, col_rem=0, entry_plane=codes)
    assert np.array_equal(a, b), "frames differ with the entry table"
    assert ca["rays"] == cb["rays"]
    tot["off"][0] += ca["rays"]; tot["off"][1] += ca["V"]
    tot["on"][0] += cb["rays"]; tot["on"][1] += cb["V"]
voff, von = tot["off"][1] / tot["off"][0], tot["on"][1] / tot["on"][0]
print("%d frames, %d rays, frames identical: V per ray %.4f from the root, %.4f from the entries: %.4f fewer (%.2f %%)" %
      (frames, tot["on"][0], voff, von, voff - von, 100 * (voff - von) / voff))
print("(the scene's margin on every ray: no certificate in these host frames; the difference is the table's)")
