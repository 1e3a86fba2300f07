"""The shading step of the device functions, compiled for the host (tools/host_kernel.cpp hk_kat_*: the per-element bodies of device_kat_shade.hpp over
device_rng.hpp, device_surface.hpp and device_shade.hpp), against the oracle's functions of the same steps (orc_kat_*: the functions raycolor and pixel
call) on every case of tests/shade_cases.py, bit for bit.  No GPU: tests/test_gpu_shade.py sends the same cases through Context.kat_*.  What each set of
cases must reach is asserted on the oracle's output alone, before the comparison (tests/shade_checks.py)."""
import os
import sys

import pytest

import shade_checks as ck

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))


@pytest.fixture(scope="module")
def impl(tmp_path_factory):
    import host_kernel as hk
    hk.build()
    rts, tex = ck.files(tmp_path_factory)
    scene = hk.Scene(rts, tex)
    return ck.Impl("host", hk.kat_sample, hk.kat_outside, scene.kat_tex, scene.kat_bounce, scene.kat_miss, hk.kat_camera, hk.kat_store)


def test_samplers_plain_and_merged(impl):
    """rand_in_unit_sphere / rand_in_unit_disk and rand_points_merged: the same point and the same number of draws as the oracle's loops on 2^20 states,
    among them the ones that re-enter the merged loop and the ones whose squared length falls into outside_unit's band"""
    ck.check_sampler(impl)


def test_outside_unit_around_one(impl):
    ck.check_outside(impl)


def test_texel_fetch_at_wrap_and_clamp_edges(impl, tmp_path_factory):
    ck.check_tex(impl, tmp_path_factory)


def test_one_bounce_every_branch(impl, tmp_path_factory):
    """shade_hit and the persistent kernel's split (shade_prepare, rand_points_merged, shade_scatter) on every material, both primitive types and every
    variant of a triangle's normals and textures: the ray, the attenuation and the draws consumed"""
    ck.check_bounce(impl, tmp_path_factory)


def test_background(impl, tmp_path_factory):
    ck.check_miss(impl, tmp_path_factory)


def test_camera_ray_plain_and_split(impl):
    ck.check_camera(impl)


def test_store_saturates_as_the_reference(impl):
    ck.check_store(impl)
