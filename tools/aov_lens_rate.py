"""Time of one lens-averaged AOV pass (dr_render_aov_lens, every channel, device buffers) over the full 1920x1080 grid of the C4 stand-in (the
1M-triangle heightfield bench.py renders) with N = --frames x spp samples per pixel, for both loop shapes of the kernel (option aov_lens_loop: 0 the
nested loop, 1 the refilling walk loop), beside N x the pinhole pass (dr_render_aov, the same channels) from the same run -- what the nested loop
should cost.  Median of --launches launches each, timed with HIP events on the library's stream, after two warm-up
launches.

    python tools/aov_lens_rate.py [--launches 10] [--frames 16] [--traversal 2] [--aperture A] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOOPS = ((0, "nested"), (1, "refill"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--traversal", type=int, default=2)
    ap.add_argument("--aperture", type=float, default=None, help="settings13[6] (default: the scene's own)")
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
    if a.aperture is not None:
        st[6] = a.aperture
    gw, gh = dr.pixel_grid(st, W, H)
    dev = torch.device("cuda", 0)
    tdt = {np.float32: torch.float32, np.int32: torch.int32}
    keep = {}

    def buffers(struct, channels, only=None):
        bufs = struct()
        for k, (dt, n) in channels.items():
            if only is None or k in only:
                keep[(struct, k)] = torch.empty((gh, gw, n), dtype=tdt[dt], device=dev)
                setattr(bufs, k, keep[(struct, k)].data_ptr())
        return bufs
    lens = buffers(dr.DrAovLensBuffers, dr.AOV_LENS_CHANNELS)
    pin = buffers(dr.DrAovBuffers, dr.AOV_CHANNELS, only=("depth", "distance", "material", "normal", "albedo"))
    torch.cuda.synchronize(dev)
    stream = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev)
    L = dr.lib()
    stp = st.ctypes.data_as(C.c_void_p)

    def timed(call):
        times = []
        for i in range(a.launches + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            if call() != 0:
                raise RuntimeError(L.dr_last_error().decode())
            e1.record(stream)
            e1.synchronize()
            if i >= 2:
                times.append(e0.elapsed_time(e1))
        return {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times))}
    spp = int(st[10])
    N = a.frames * spp
    res = {"what": "lens-averaged AOV pass, all channels", "scene": os.path.basename(path), "pixels": gw * gh, "traversal": ctx.get_option("traversal"),
           "launches": a.launches, "frames": a.frames, "spp": spp, "samples": N, "aperture": float(st[6])}
    res["pinhole"] = timed(lambda: L.dr_render_aov(ctx._h, stp, W, H, 0, 0, gw, gh, C.byref(pin), 1))
    res["pinhole_x_samples_ms"] = N * res["pinhole"]["median_ms"]
    cov = {}
    for loop, name in LOOPS:
        ctx.set_option("aov_lens_loop", loop)
        res[name] = timed(lambda: L.dr_render_aov_lens(ctx._h, stp, W, H, 0, 0, gw, gh, dr.GUIDE_SEED, 1, a.frames, C.byref(lens), 1))
        res[name]["mrays_per_s"] = gw * gh * N / (res[name]["median_ms"] * 1e3)
        res[name]["over_pinhole_x_samples"] = res[name]["median_ms"] / res["pinhole_x_samples_ms"]
        cov[name] = keep[(dr.DrAovLensBuffers, "coverage")].clone()
    ctx.set_option("aov_lens_loop", 0)
    res["same_bits"] = bool(torch.equal(cov["refill"], cov["nested"]))
    res["mean_coverage"] = float(cov["nested"].mean().item())
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
