"""Time of one first-hit AOV pass (dr_render_aov, every channel, device buffers) over the full 1920x1080 grid of the C4 stand-in (the 1M-triangle
heightfield bench.py renders): median of --launches launches, each timed with HIP events on the library's stream, after two warm-up launches.

    python tools/aov_rate.py [--launches 10] [--traversal 2] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--traversal", type=int, default=2)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import dogeray_amd as dr
    W, H = 1920, 1080
    path = bench.ensure_scene(os.environ.get("DOGERAY_BENCH_CACHE", "/tmp/dogeray_bench"), 709, W, H)
    sc = dr.Scene.load(path, "")
    sc.build_bvh()
    ctx = dr.Context(0).upload(sc)
    ctx.set_traversal(a.traversal)
    st = dr.pack_settings13(sc.settings(), 1)
    gw, gh = dr.pixel_grid(st, W, H)
    dev = torch.device("cuda", 0)
    tdt = {np.float32: torch.float32, np.int32: torch.int32}
    bufs = dr.DrAovBuffers()
    keep = {}
    for k, (dt, n) in dr.AOV_CHANNELS.items():
        keep[k] = torch.empty((gh, gw, n), dtype=tdt[dt], device=dev)
        setattr(bufs, k, keep[k].data_ptr())
    torch.cuda.synchronize(dev)
    stream = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev)
    L = dr.lib()
    times = []
    for i in range(a.launches + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = L.dr_render_aov(ctx._h, st.ctypes.data_as(C.c_void_p), W, H, 0, 0, gw, gh, C.byref(bufs), 1)
        if rc != 0:
            raise RuntimeError(L.dr_last_error().decode())
        e1.record(stream)
        e1.synchronize()
        if i >= 2:
            times.append(e0.elapsed_time(e1))
    hits = float((keep["object"] >= 0).float().mean().item())
    res = {"what": "first-hit AOV pass, all channels", "scene": os.path.basename(path), "pixels": gw * gh, "traversal": ctx.get_option("traversal"),
           "launches": a.launches, "median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times)),
           "mrays_per_s": gw * gh / (float(np.median(times)) * 1e3), "hit_fraction": hits}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
