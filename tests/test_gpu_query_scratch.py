"""The four queries on caller lists share one staging buffer, one scratch buffer of {t or d2 bits, slot} words and one cursor (dr_context
query_staging, query_scratch, query_cursor).  On the device path nothing waits between two calls, so a later call reuses -- or regrows -- memory whose
earlier reader may still be queued.  Every result here must equal, bit for bit, the same call made ALONE on a fresh context: trace with a surface
channel, trace_all with K = 2 and a surface channel, nearest with `point` and radiance with spp 1, at 129 rays (one more than the 128-ray chunk) through
the forced persistent kernels, back to back in both orders; then a host-path call of 1000 rays right behind a device-path call, which makes staging
and scratch grow while the earlier results are unread."""
import numpy as np
import pytest

import ray_cases as rc
import ray_checks as ck

pytestmark = pytest.mark.gpu
N, N_HOST = 129, 1000
FORCED = ("trace_kernel", "radiance_kernel", "allhits_kernel")

CALLS = {
    "trace": lambda c, o, d: c.trace(o, d, channels=("t", "object", "normal")),
    "trace_all": lambda c, o, d: c.trace_all(o, d, None, 2, channels=("count", "t", "object", "normal")),
    "nearest": lambda c, o, d: c.nearest(o, channels=("distance", "object", "point")),
    "radiance": lambda c, o, d: c.radiance(o, d, 1, 4, 1.0, -1, seed=7, channels=("radiance", "bounces")),
}


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    return dogeray_amd


def fresh(dr, L):
    c = dr.Context(0)
    ps = dr.Scene.load(L.path, "")
    ps.build_bvh()
    c.upload(ps)
    assert c.get_option("wide_depth") > 0      # the persistent kernels exist
    for k in FORCED:
        c.set_option(k, 2)
    return c


def as_numpy(out):
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in out.items()}


@pytest.fixture(scope="module")
def case(dr, tmp_path_factory):
    """the scene, the rays on the host and on the device, and every call's answer when it is the only call its context ever made"""
    import torch
    L = ck.loaded("grid_mixed", tmp_path_factory)
    dev = torch.device("cuda", 0)
    rays = {n: rc.mixed_rays(L.g, n) for n in (N, N_HOST)}
    tensors = tuple(torch.from_numpy(a).to(dev) for a in rays[N])
    alone = {}
    for name, call in CALLS.items():
        for key, args in (((name, "device"), tensors), ((name, "host"), rays[N_HOST])):
            c = fresh(dr, L)
            alone[key] = as_numpy(call(c, *args))
            c.close()
    assert (alone["trace", "device"]["t"] > 0).any() and (alone["trace_all", "device"]["count"] > 1).any()
    assert (alone["nearest", "device"]["object"] >= 0).any() and alone["radiance", "device"]["bounces"].max() > 1
    return L, rays, tensors, alone


def differing(got, want):
    """channels of `want` whose bits differ in `got`"""
    view = lambda a: ck.bits(a) if a.dtype == np.float32 else a
    return [k for k, w in want.items() if got[k].shape != w.shape or got[k].dtype != w.dtype or not np.array_equal(view(got[k]), view(w))]


@pytest.mark.parametrize("order", [tuple(CALLS), tuple(reversed(CALLS))], ids=["in order", "reversed"])
def test_back_to_back_device_calls_equal_each_call_alone(dr, case, order):
    L, _, tensors, alone = case
    c = fresh(dr, L)
    try:
        outs = [CALLS[name](c, *tensors) for name in order]      # queued one behind the other: nothing is read, nothing waits
        bad = ["%s: %s" % (name, ",".join(differing(as_numpy(out), alone[name, "device"]))) for name, out in zip(order, outs)
               if differing(as_numpy(out), alone[name, "device"])]
        assert not bad, " | ".join(bad)
    finally:
        c.close()


@pytest.mark.parametrize("first", list(CALLS))
def test_a_larger_host_call_right_behind_a_device_call(dr, case, first):
    """a small host-path call first, so that staging and scratch exist; then `first` on the device path, unread; then another query on the host path
    with 1000 rays: both buffers grow under the queued work"""
    L, rays, tensors, alone = case
    c = fresh(dr, L)
    try:
        CALLS["trace_all"](c, *rays[N])
        queued = CALLS[first](c, *tensors)
        second = "trace_all" if first != "trace_all" else "trace"
        grown = CALLS[second](c, *rays[N_HOST])
        assert not differing(as_numpy(queued), alone[first, "device"]), first
        assert not differing(grown, alone[second, "host"]), second
    finally:
        c.close()
