"""What adaptive sampling (dr_render_adaptive) buys and costs, on the C4 stand-in (the 1M-triangle heightfield bench.py renders) at 1920x1080, in one
process:
  until       Context.render_until (twice: the parent's code path, its second run gives the run-to-run spread) and Context.render_until_adaptive to
              the same tolerance and per-mille: frames' worth of samples (samples / grid pixels) and wall-clock time of each
  pass        one pass of --pass-frames frames with all, half and none of the tiles active (tolerance 0, the median over tiles of the tile-maximum
              sigma, 1e9), timed with HIP events on the context's stream -- at "none" the time is the selection, the split, the launch that finds
              every queue empty and the fold of nothing: the pass's fixed cost; beside them render_accumulate_pipelined of the same frames
  mse         the mean squared error of the displayed mean (0..255 units, all channels) against a mean of --reference-frames other frames: the
              adaptive render, and a uniform render of the same total samples rounded to whole frames

    python tools/adaptive_rate.py [--tolerance 1.0] [--permille 10] [--max-frames 256] [--pass-frames 8] [--reference-frames 512] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STRIDE = 1000003


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tolerance", type=float, default=1.0)
    ap.add_argument("--permille", type=int, default=10)
    ap.add_argument("--max-frames", type=int, default=256)
    ap.add_argument("--pass-frames", type=int, default=8)
    ap.add_argument("--reference-frames", type=int, default=512)
    ap.add_argument("--launches", type=int, default=5)
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
    gx, gy = W // 8, H // 8
    grid = 64 * gx * gy
    ctx.set_option("moments", 1)
    res = {"what": "adaptive sampling", "scene": os.path.basename(path), "grid_pixels": grid, "tolerance": a.tolerance, "permille": a.permille,
           "max_frames": a.max_frames}

    def mean_image(divide_by):
        acc, hist = ctx.accum_read().astype(np.float64), ctx.accum_history().astype(np.float64) + divide_by
        return (acc / np.maximum(hist, 1.0)[..., None])[:8 * gx, :8 * gy]

    # the long mean, from seeds no other run uses
    ctx.accum_reset(W, H)
    ctx.render_accumulate_pipelined(st, W, H, bg, 7 + 10 ** 6 * STRIDE, STRIDE, a.reference_frames)
    reference = mean_image(a.reference_frames)

    def uniform_until():
        ctx.accum_reset(W, H)
        t0 = time.perf_counter()
        frames, result = ctx.render_until(st, W, H, bg, 1, STRIDE, a.tolerance, a.permille, a.max_frames)
        return {"wall_ms": (time.perf_counter() - t0) * 1e3, "frames_worth": float(frames), "converged": bool(dr.Context.converged(result, a.permille)),
                "above": result["above"], "mse": float(np.mean((mean_image(frames) - reference) ** 2))}

    def adaptive_until():
        ctx.accum_reset(W, H)
        t0 = time.perf_counter()
        uniform, passes, samples, result = ctx.render_until_adaptive(st, W, H, bg, 1, STRIDE, a.tolerance, a.permille, a.max_frames)
        return {"wall_ms": (time.perf_counter() - t0) * 1e3, "frames_worth": uniform + samples / grid, "uniform_frames": uniform, "passes": passes,
                "converged": bool(dr.Context.converged(result, a.permille)), "above": result["above"], "mse": float(np.mean((mean_image(uniform) - reference) ** 2))}

    uniform_until()                                     # warm-up: the view's tile words and order, the pipeline's buffers
    res["render_until"] = [uniform_until(), uniform_until()]
    res["render_until_adaptive"] = [adaptive_until(), adaptive_until()]
    u, ad = res["render_until"], res["render_until_adaptive"]
    res["render_until_spread"] = abs(u[1]["wall_ms"] - u[0]["wall_ms"]) / u[0]["wall_ms"]
    res["adaptive_over_uniform_wall"] = ad[1]["wall_ms"] / u[1]["wall_ms"]
    res["adaptive_over_uniform_samples"] = ad[1]["frames_worth"] / u[1]["frames_worth"]
    # the uniform render of the adaptive run's samples, rounded to whole frames
    equal = max(1, int(round(ad[1]["frames_worth"])))
    ctx.accum_reset(W, H)
    ctx.render_accumulate_pipelined(st, W, H, bg, 1, STRIDE, equal)
    res["equal_samples"] = {"uniform_frames": equal, "uniform_mse": float(np.mean((mean_image(equal) - reference) ** 2)), "adaptive_frames_worth": ad[1]["frames_worth"],
                            "adaptive_mse": ad[1]["mse"]}

    # one pass at all / half / none of the tiles
    dev = torch.device("cuda", 0)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev)

    def timed(call):
        times = []
        for i in range(a.launches + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            out = call(i)
            e1.record(stream)
            e1.synchronize()
            if i >= 2:
                times.append(e0.elapsed_time(e1))
        return {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times))}, out

    ctx.accum_reset(W, H)
    ctx.render_accumulate_pipelined(st, W, H, bg, 1, STRIDE, 8)
    sigma = ctx.error(st, W, H, 8, 0.0, sigma=True)["sigma"][:8 * gy, :8 * gx]
    half = float(np.median(sigma.reshape(gy, 8, gx, 8).max(axis=(1, 3))))
    res["pass"] = {"frames": a.pass_frames}
    for name, tol in (("all", 0.0), ("half", half), ("none", 1e9)):
        # (max_samples 0 and a fixed divide_by: the mask of "half" moves a little from pass to pass as the active tiles' estimates settle)
        t, r = timed(lambda i: ctx.render_adaptive(st, W, H, bg, 99 + i * a.pass_frames * STRIDE, STRIDE, a.pass_frames, 8, tolerance=tol))
        t["active_tiles_last"], t["tiles"] = r["active_tiles"], r["tiles"]
        res["pass"][name] = t
    ctx.set_option("moments", 1)
    ctx.accum_reset(W, H)
    res["pass"]["pipelined_same_frames"] = timed(lambda i: ctx.render_accumulate_pipelined(st, W, H, bg, 99 + i * a.pass_frames * STRIDE, STRIDE, a.pass_frames))[0]
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
