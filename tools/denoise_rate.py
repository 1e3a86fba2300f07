"""Time of the a-trous denoiser (dr_accum_denoise, RGB8 into a device buffer) over the full 1920x1080 grid of the C4 stand-in (the 1M-triangle
heightfield bench.py renders), with 4 frames in the accumulator: median of --launches calls, each timed with HIP events on the library's stream,
after two warm-up calls, for both shapes of the a-trous pass (option denoise_tiles):
  filter      default parameters (5 iterations), guides cached
  with_guides default parameters, the guides recomputed on every call (the settings' spp alternates, which is part of the cache key)
  iterations  1 .. 5, guides cached

    python tools/denoise_rate.py [--launches 10] [--json out.json]
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
    st = dr.pack_settings13(sc.settings(), 1)
    st_other = st.copy()
    st_other[10] += 1                   # another spp: the same guides, another cache key
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, sc.settings().background, 1, 1000003, 4)
    dev = torch.device("cuda", 0)
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev)
    L = dr.lib()

    def timed(settings_list, **params):
        p = dr.denoise_params(**params)
        times = []
        for i in range(a.launches + 2):
            s = settings_list[i % len(settings_list)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = L.dr_accum_denoise(ctx._h, s.ctypes.data_as(C.c_void_p), W, H, 4, C.byref(p), None, C.c_void_p(rgb.data_ptr()), 1)
            if rc != 0:
                raise RuntimeError(L.dr_last_error().decode())
            e1.record(stream)
            e1.synchronize()
            if i >= 2:
                times.append(e0.elapsed_time(e1))
        return {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times))}

    res = {"what": "a-trous denoiser, RGB8 out, device buffer", "scene": os.path.basename(path), "pixels": W * H, "launches": a.launches}
    for tiles in (1, 0):
        ctx.set_option("denoise_tiles", tiles)
        r = {"filter": timed([st]), "with_guides": timed([st, st_other])}
        for it in range(1, 6):
            r["iterations_%d" % it] = timed([st], iterations=it)
        res["denoise_tiles_%d" % tiles] = r
    ctx.set_option("denoise_tiles", 1)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
