"""The shading step on the GPU, function by function: Context.kat_* (kernels_kat.hip: the per-element bodies of device_kat_shade.hpp over
device_rng.hpp, device_surface.hpp and device_shade.hpp, one element per lane) against the oracle's functions of the same steps on every case of
tests/shade_cases.py, bit for bit -- the cases tests/test_shade_host.py runs through the host build.  Where a hook has two forms (the plain functions
and what the persistent kernel runs: rand_points_merged, shade_prepare / shade_scatter, camera_prepare / camera_finish) both must equal the oracle.
This is where outside_unit's band (the square root behind the wave's branch) and the merged loop's second stage run on the device: the committed
states take them 25 and 19 times (tests/shade_checks.py sampler_preconditions asserts the counts on the oracle alone)."""
import pytest

import shade_checks as ck

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def impl(tmp_path_factory):
    import dogeray_amd as dr
    assert dr.device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    rts, tex = ck.files(tmp_path_factory)          # the files exist before this process touches the GPU
    scene = dr.Scene.load(rts, tex)
    scene.build_bvh()
    ctx = dr.Context(0).upload(scene)
    yield ck.Impl("gpu", ctx.kat_sample, ctx.kat_outside, ctx.kat_tex, ctx.kat_bounce, ctx.kat_miss, ctx.kat_camera, ctx.kat_store)
    ctx.close()


def test_samplers_plain_and_merged(impl):
    """2^20 states, kinds 0 / 2 / 3 mixed inside every wave as a phase of the persistent kernel mixes them"""
    ck.check_sampler(impl)


def test_outside_unit_around_one(impl):
    ck.check_outside(impl)


def test_texel_fetch_at_wrap_and_clamp_edges(impl, tmp_path_factory):
    ck.check_tex(impl, tmp_path_factory)


def test_one_bounce_every_branch(impl, tmp_path_factory):
    ck.check_bounce(impl, tmp_path_factory)


def test_background(impl, tmp_path_factory):
    ck.check_miss(impl, tmp_path_factory)


def test_camera_ray_plain_and_split(impl):
    ck.check_camera(impl)


def test_store_saturates_as_the_reference(impl):
    ck.check_store(impl)
