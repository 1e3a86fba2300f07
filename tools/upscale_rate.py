"""Time of the AOV-guided upsampler (dr_accum_upscale, RGB8 into a device buffer) on the C4 stand-in (the 1M-triangle heightfield bench.py renders)
at 1920x1080, with 4 frames at the divisor in the accumulator: median of --launches calls, each timed with HIP events on the library's stream, after
two warm-up calls.  Per divisor 8, 4, 2:
  guided_warm      default parameters, both guide caches warm
  guided_one_pass  the low guides traced on every call (an untimed dr_accum_denoise of another divisor takes the cache between two calls)
  guided_two_pass  low and full guides traced on every call (the settings' spp alternates, which is part of both cache keys)
  block            the reference's block fill
  prefiltered      guided behind the default a-trous prefilter, guides warm
and, in the same run, the yardsticks: dr_accum_present (with its download) and dr_accum_denoise (defaults, device buffer) at full resolution, and one
frame of a batch of 32 at div 1 and at div 2 (what "a div-2 frame plus the upscale" costs beside a full frame).

    python tools/upscale_rate.py [--launches 10] [--json out.json]
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
    s = sc.settings()
    ctx = dr.Context(0).upload(sc)
    dev = torch.device("cuda", 0)
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    host = np.empty((H, W, 3), np.uint8)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev)
    L = dr.lib()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)

    def check(rc):
        if rc != 0:
            raise RuntimeError(L.dr_last_error().decode())

    def timed(call, between=None):
        times = []
        for i in range(a.launches + 2):
            if between:
                between(i)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call(i)
            e1.record(stream)
            e1.synchronize()
            if i >= 2:
                times.append(e0.elapsed_time(e1))
        return {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times))}

    def passes():
        return ctx.get_option("upscale_aov_passes")

    res = {"what": "AOV-guided upsampler, RGB8 out, device buffer", "scene": os.path.basename(path), "pixels": W * H, "launches": a.launches}
    one = dr.denoise_params(iterations=1)
    pre = dr.denoise_params()
    for div in (8, 4, 2):
        st = dr.pack_settings13(s, div)
        st_spp = st.copy()
        st_spp[10] += 1                  # another spp: the same guides, another cache key
        st_div = dr.pack_settings13(s, 16 if div == 8 else 8)
        ctx.accum_reset(W, H)
        ctx.render_accumulate(st, W, H, s.background, 1, 1000003, 4)
        guided, block = dr.upscale_params(), dr.upscale_params(mode=dr.UPSCALE_BLOCK)
        up = lambda st13, p, f=None: check(L.dr_accum_upscale(ctx._h, vp(st13), W, H, 4, C.byref(p), C.byref(f) if f is not None else None, None,
                                                              C.c_void_p(rgb.data_ptr()), 1))
        seen = []
        r = {}
        r["guided_warm"] = timed(lambda i: (up(st, guided), seen.append(passes())))
        assert seen[2:] == [0] * a.launches, seen
        del seen[:]
        r["guided_one_pass"] = timed(lambda i: (up(st, guided), seen.append(passes())),
                                     between=lambda i: check(L.dr_accum_denoise(ctx._h, vp(st_div), W, H, 4, C.byref(one), None, C.c_void_p(rgb.data_ptr()), 1)))
        assert seen[2:] == [1] * a.launches, seen
        del seen[:]
        r["guided_two_pass"] = timed(lambda i: (up((st, st_spp)[i % 2], guided), seen.append(passes())))
        assert seen[2:] == [2] * a.launches, seen
        r["block"] = timed(lambda i: up(st, block))
        r["prefiltered"] = timed(lambda i: up(st, guided, pre))
        res["div_%d" % div] = r
    # the yardsticks, at full resolution
    st1, st2 = dr.pack_settings13(s, 1), dr.pack_settings13(s, 2)
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st1, W, H, s.background, 1, 1000003, 4)
    res["present_full_with_download"] = timed(lambda i: check(L.dr_accum_present(ctx._h, 4, vp(host))))
    res["denoise_full"] = timed(lambda i: check(L.dr_accum_denoise(ctx._h, vp(st1), W, H, 4, C.byref(pre), None, C.c_void_p(rgb.data_ptr()), 1)))
    for name, st in (("frame_div_1", st1), ("frame_div_2", st2)):
        ctx.accum_reset(W, H)
        t = timed(lambda i: ctx.render_accumulate(st, W, H, s.background, 1 + 32 * i, 1000003, 32))
        res[name] = {k: v / 32 for k, v in t.items()}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
