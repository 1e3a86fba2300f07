"""Writes host arrays into the live device planes of a Context's accumulator -- the sums, the history plane and the second-moment plane -- through
dr_accum_device_ptr, dr_accum_history_device_ptr and dr_accum_moments_device_ptr, and reads them back.  A helper of tests/test_gpu_planes.py
(not a conftest).  A history plane exists only after a reprojection (history() makes one with an identity reprojection) and a second-moment
plane only after an accum_reset with option "moments" = 1; reprojecting swaps the buffers, so the pointers are asked for at every write."""
import ctypes as C

import numpy as np


def pointers(dr, ctx):
    """{"acc" | "hist" | "m2": (device pointer or None, bytes)} of the current buffers"""
    out = {}
    for key, name in (("acc", "dr_accum_device_ptr"), ("hist", "dr_accum_history_device_ptr"), ("m2", "dr_accum_moments_device_ptr")):
        ptr, nbytes = C.c_void_p(), C.c_uint64()
        assert getattr(dr.lib(), name)(ctx._h, C.byref(ptr), C.byref(nbytes)) == 0, name
        out[key] = (ptr.value, int(nbytes.value))
    return out


def poke(dr, ctx, acc=None, hist=None, m2=None):
    """acc int32[W, H, 3], hist int32[W, H], m2 uint64[W, H] (each or None) into the live planes.  The context's stream is drained before the
    copies and torch's after them, so the write is ordered against the library's work on either side.  The uint64 plane goes as int32 pairs."""
    import torch
    from dogeray_amd import multigpu
    W, H, _ = ctx._acc_shape
    ctx.synchronize()
    ptrs = pointers(dr, ctx)
    dev = torch.device("cuda", ctx.device)
    for key, arr, dtype, shape in (("acc", acc, np.int32, (W, H, 3)), ("hist", hist, np.int32, (W, H)), ("m2", m2, np.uint64, (W, H))):
        if arr is None:
            continue
        assert arr.dtype == dtype and arr.shape == shape, (key, arr.dtype, arr.shape)
        ptr, nbytes = ptrs[key]
        assert ptr and nbytes == arr.nbytes, "the accumulator has no %s plane of %d bytes (%r)" % (key, arr.nbytes, ptrs[key])
        words = np.ascontiguousarray(arr).view(np.int32).reshape(-1).copy()
        torch.as_tensor(multigpu._DevArray(ptr, words.size), device=dev).copy_(torch.from_numpy(words))
    torch.cuda.synchronize()


def peek(ctx):
    """(sums, history, second moments) as accum_read, accum_history and accum_moments return them"""
    return ctx.accum_read(), ctx.accum_history(), ctx.accum_moments()


def history(ctx, st, W, H):
    """gives the accumulator a history plane: an identity reprojection (it also rewrites the sums: poke them afterwards)"""
    ctx.reproject(st, st, W, H, 1)


def install(dr, ctx, acc=None, hist=None, m2=None):
    """poke, read back, assert that what was read is what was written, and return the planes READ BACK (a reference is fed with these, so a
    write that did not land cannot pass): (acc, hist, m2); a plane that was not written comes back as it is"""
    poke(dr, ctx, acc=acc, hist=hist, m2=m2)
    got = peek(ctx)
    for name, want, have in (("acc", acc, got[0]), ("hist", hist, got[1]), ("m2", m2, got[2])):
        assert want is None or np.array_equal(want, have), "%s: the plane read back differs from the plane written at %d values" % (name, int((want != have).sum()))
    return got
