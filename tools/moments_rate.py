"""What the second-moment plane (option "moments") costs, on the C4 stand-in (the 1M-triangle heightfield bench.py renders) at 1920x1080, in one
process, every figure the median of --launches measurements after two warm-up ones:
  pipelined   wall-clock ms per frame of dr_render_accumulate_pipelined over --frames frames, with moments = 0, then 1, then 0 again: the two
              moments = 0 runs are the parent's code path and give the run-to-run spread
  add         the plain add (acc += frame) and the fused add (acc += frame, M2 += yc^2), each launch timed alone with HIP events
              (dr_context_probe_frame_add), and the bytes per pixel each moves (36 / 52)
  error       dr_accum_error: the counts only, the counts and the sigma plane into a device buffer, and into host memory

    python tools/moments_rate.py [--launches 10] [--frames 32] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--frames", type=int, default=32)
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
    bg = sc.settings().background

    def stat(v):
        return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}

    def pipelined(moments):
        ctx.set_option("moments", moments)
        ctx.accum_reset(W, H)
        times = []
        for i in range(a.launches + 2):
            t0 = time.perf_counter()
            ctx.render_accumulate_pipelined(st, W, H, bg, 1 + i * a.frames * 1000003, 1000003, a.frames)
            dt = (time.perf_counter() - t0) * 1e3 / a.frames
            if i >= 2:
                times.append(dt)
        return stat(times)

    res = {"what": "cost of the second-moment plane", "scene": os.path.basename(path), "pixels": W * H, "launches": a.launches, "frames": a.frames}
    res["pipelined_ms_per_frame"] = {"moments0_first": pipelined(0), "moments1": pipelined(1), "moments0_again": pipelined(0)}
    p = res["pipelined_ms_per_frame"]
    res["pipelined_spread"] = abs(p["moments0_again"]["median_ms"] - p["moments0_first"]["median_ms"]) / p["moments0_first"]["median_ms"]
    res["pipelined_moments1_over_0"] = p["moments1"]["median_ms"] / (0.5 * (p["moments0_first"]["median_ms"] + p["moments0_again"]["median_ms"]))

    ctx.set_option("moments", 1)
    ctx.accum_reset(W, H)
    ctx.render_accumulate_pipelined(st, W, H, bg, 1, 1000003, 8)
    plain, fused = ctx.probe_frame_add(a.launches + 2)
    res["add"] = {"plain": stat(plain[2:]), "fused": stat(fused[2:]), "plain_bytes_per_pixel": 36, "fused_bytes_per_pixel": 52}
    for k, nbytes in (("plain", 36), ("fused", 52)):
        res["add"][k]["GB_per_s"] = nbytes * W * H / (res["add"][k]["median_ms"] * 1e-3) / 1e9

    dev = torch.device("cuda", 0)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev)

    def error(sigma, device):
        times = []
        for i in range(a.launches + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            r = ctx.error(st, W, H, 8, 1.0, sigma=sigma, device=device)
            wall = (time.perf_counter() - t0) * 1e3
            e1.record(stream)
            e1.synchronize()
            if i >= 2:
                times.append((e0.elapsed_time(e1), wall))
        out = stat([t[0] for t in times])
        out["wall_median_ms"] = float(np.median([t[1] for t in times]))
        return out, {k: v for k, v in r.items() if k != "sigma"}

    res["error"] = {"counts_only": error(False, False)[0], "counts_and_device_sigma": error(True, True)[0]}
    res["error"]["counts_and_host_sigma"], res["error_result_8_frames"] = error(True, False)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
