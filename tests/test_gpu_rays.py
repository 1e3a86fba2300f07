"""The closest-hit walks on the GPU over the adversarial rays and degenerate scenes of tests/ray_cases.py, against the oracle's hit() -- t bit for
bit and the object index, no tolerance: every (scene, class) pair through dr_kat_hit (the counting build: threaded, ordered and wide walk, the wide
one over both trees) and through dr_kat_trace (the lean build that render launches time and ship: variant 0 the primitive-first leaf step behind a
wave ballot, variants 1, 3, 7 the persistent waves with SignMask, refill and exclusive node / leaf steps).  tests/test_rays_host.py proves without a
GPU that the classes reach the edges they are named for and runs every ray through the host build of the walks first."""
import numpy as np
import pytest

import ray_cases as rc
import ray_checks as ck

pytestmark = pytest.mark.gpu

TRACE_VARIANTS = (0, 1, 3, 7)


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    return dogeray_amd


@pytest.fixture(scope="module")
def ctx(dr, synth):          # synth first: the generated scenes exist before this process touches the GPU
    c = dr.Context(0)
    yield c
    c.close()


def upload(dr, ctx, L, wide_tree=2):
    """the scene resident with the tree of option wide_tree (which takes effect at an upload)"""
    ps = dr.Scene.load(L.path, "")
    ps.build_bvh()
    ctx.set_option("wide_tree", wide_tree)
    ctx.upload(ps)
    return ps


def check(failed, what, L, cls, t, idx):
    o, d, rt, ri = L.case(cls)
    bad = ck.mismatches(t, idx, rt, ri)
    if len(bad):
        failed.append("%s / %s %s: %d of %d rays differ -- %s" % (L.stem, cls, what, len(bad), len(o), ck.describe(o, d, t, idx, rt, ri, bad, limit=2)))


@pytest.mark.parametrize("stem", rc.STEMS)
def test_kat_hit_returns_the_oracles_hits(dr, ctx, tmp_path_factory, stem):
    L = ck.loaded(stem, tmp_path_factory)
    failed = []
    try:
        for tree, traversals in ((1, (2,)), (2, (0, 1, 2))):
            upload(dr, ctx, L, tree)
            for traversal in traversals:
                ctx.set_traversal(traversal)
                for cls, _ in rc.PAIRS[stem]:
                    o, d = L.case(cls)[:2]
                    check(failed, "traversal %d wide_tree %d" % (traversal, tree), L, cls, *ctx.kat_hit(o, d))
        # the scene's precondition, where the product itself says it (wide_tree 2 is resident, traversal 2 asked for)
        own, depth = ctx.get_option("wide_own_bounds"), ctx.get_option("wide_depth")
        if stem == "grid_small": assert own == L.g.n
        if stem == "grid_mixed": assert own == rc.GRID_MIXED_SMALL and 0 <= 2 * own - L.g.n <= 2
        if stem == "stadium": assert depth == 17
        if stem == "far_refused": assert depth == 0 and ctx.get_option("traversal") == 0      # build_wide refused: the threaded walk answers for traversal 2
        else: assert depth >= 1 and ctx.get_option("traversal") == 2
    finally:
        ctx.set_option("wide_tree", 2)
        ctx.set_traversal(dr.TRAVERSAL_WIDE)
    assert not failed, " | ".join(failed)


@pytest.mark.parametrize("stem", [s for s in rc.STEMS if s != "far_refused"])
def test_kat_trace_returns_the_oracles_hits(dr, ctx, tmp_path_factory, stem):
    L = ck.loaded(stem, tmp_path_factory)
    failed = []
    try:
        for tree in (2, 1):
            upload(dr, ctx, L, tree)
            for variant in TRACE_VARIANTS:
                for cls, _ in rc.PAIRS[stem]:
                    o, d = L.case(cls)[:2]
                    check(failed, "trace variant %d wide_tree %d" % (variant, tree), L, cls, *ctx.kat_trace(o, d, variant))
    finally:
        ctx.set_option("wide_tree", 2)
    assert not failed, " | ".join(failed)


def test_ray_counts_around_the_probes_chunks(dr, ctx, tmp_path_factory):
    """n = 1 .. 1000 rays of one mixed class: the probe's 128-ray chunks, its `my < n && my < chunk_end` tail, the one-ray-per-lane kernels' `i >= n`
    early return beside lanes whose LDS stack is live"""
    L = ck.loaded("grid_mixed", tmp_path_factory)
    upload(dr, ctx, L)
    failed = []
    for n in rc.RAY_COUNTS:
        o, d = rc.mixed_rays(L.g, n)
        rt, ri = L.orc.kat_hit(o, d)
        assert rt[-1] > 0 and rt[0] > 0                    # (tests/test_rays_host.py: the salts of mixed_rays) a dropped head or tail is a dropped HIT
        for what, (t, idx) in (("kat_trace 1", ctx.kat_trace(o, d, 1)), ("kat_trace 7", ctx.kat_trace(o, d, 7)), ("kat_trace 0", ctx.kat_trace(o, d, 0)), ("kat_hit", ctx.kat_hit(o, d))):
            assert len(t) == n and len(idx) == n
            bad = ck.mismatches(t, idx, rt, ri)
            if len(bad):
                failed.append("%d rays, %s: %d differ -- %s" % (n, what, len(bad), ck.describe(o, d, t, idx, rt, ri, bad, limit=2)))
    assert not failed, " | ".join(failed)


def test_the_refused_scene_has_no_trace_and_falls_back(dr, ctx, tmp_path_factory):
    L = ck.loaded("far_refused", tmp_path_factory)
    upload(dr, ctx, L)
    ctx.set_traversal(dr.TRAVERSAL_WIDE)
    assert ctx.get_option("wide_depth") == 0
    o, d, rt, ri = L.case("axis")
    for variant in (0, 1):
        with pytest.raises(dr.DogerayError) as e:
            ctx.kat_trace(o, d, variant)
        assert e.value.code == dr.ERR_INVALID and "wide tree" in str(e.value)
    t, idx = ctx.kat_hit(o, d)                                # traversal 2 asked for: the threaded walk answers
    assert len(ck.mismatches(t, idx, rt, ri)) == 0 and (rt > 0).mean() > 0.05
    with pytest.raises(dr.DogerayError):
        ctx.kat_trace(o, d, 8)                                # (and a variant that does not exist is refused before anything is launched)
