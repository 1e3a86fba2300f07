"""Time of the temporal reprojection (dr_accum_reproject) over the full 1920x1080 grid of the C4 stand-in (the 1M-triangle heightfield bench.py
renders), with 4 frames in the accumulator: median of --launches calls, each timed with HIP events on the library's stream, after two warm-up
calls:
  cold   the guide cache misses: both views' first-hit AOVs are traced (two AOV passes, then the reprojection kernel)
  warm   every call's `from` view is the previous call's `to` view (a moving camera): one AOV pass
and, in the same run, the kernel time of one rendered frame (dr_stats over 16 accumulated frames) and the shares of the pixel classes of the
first move.  The camera moves sideways by 0.5 % of its distance to the look-at point per call.

    python tools/reproject_rate.py [--launches 10] [--json out.json]
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
    cam, look = st[0:3].astype(np.float64), st[3:6].astype(np.float64)
    fwd = look - cam
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right *= 0.005 * np.linalg.norm(fwd) / np.linalg.norm(right)

    def view(k):
        v = st.copy()
        v[0:3] = cam + k * right
        v[3:6] = look + k * right
        return v

    ctx.accum_reset(W, H)
    ctx.stats_reset()
    ctx.render_accumulate(st, W, H, sc.settings().background, 1, 1000003, 16)
    s = ctx.stats()
    frame_ms = s["kernel_ms"] / max(1, s["frames"])
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, sc.settings().background, 1, 1000003, 4)
    dev = torch.device("cuda", 0)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev)
    L = dr.lib()
    p = dr.reproject_params()
    first = {}

    def timed(pairs):
        times, passes = [], set()
        for i, (va, vb) in enumerate(pairs):
            r = dr.DrReprojectResult()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = L.dr_accum_reproject(ctx._h, va.ctypes.data_as(C.c_void_p), vb.ctypes.data_as(C.c_void_p), W, H, 4, C.byref(p), C.byref(r))
            if rc != 0:
                raise RuntimeError(L.dr_last_error().decode())
            e1.record(stream)
            e1.synchronize()
            if not first:
                first.update({k: int(getattr(r, k)) for k, _ in dr.DrReprojectResult._fields_})
            if i >= 2:
                times.append(e0.elapsed_time(e1))
                passes.add(ctx.get_option("reproject_aov_passes"))
        return {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times)), "aov_passes": sorted(passes)}

    n = a.launches + 2
    # cold: view 2i -> 2i + 1, the next call starts from a view nobody cached; warm: view i -> i + 1
    cold = timed([(view(2 * i + 100), view(2 * i + 101)) for i in range(n)])
    warm = timed([(view(i), view(i + 1)) for i in range(-1, n - 1)])
    res = {"what": "temporal reprojection of the accumulator", "scene": os.path.basename(path), "pixels": W * H, "launches": a.launches,
           "cold": cold, "warm": warm, "frame_kernel_ms": frame_ms, "first_move": first,
           "valid_share": first["valid"] / max(1, first["pixels"])}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
