"""tests/merge_cases.py without a GPU: every class has the pattern it was made for -- stated as a function of its inputs, so the GPU run
(tests/test_gpu_store_merged.py) cannot pass a class for want of it --, and the reference (per pixel, int64, wrapped once) agrees with a second,
deliberately naive formulation: one lane after the other, wrapped to int32 after every add.  The integers a lane adds are the oracle's kat_store of
its colour, as in the GPU test."""
import numpy as np
import pytest

import merge_cases as mc
import shade_checks as ck


@pytest.fixture(scope="module")
def ints():
    cache = {}

    def of(name):
        if name not in cache:
            v = mc.lane_integers(mc.case(name), ck.orc().kat_store)
            v.flags.writeable = False
            cache[name] = v
        return cache[name]
    return of


@pytest.mark.parametrize("name", list(mc.CLASSES))
def test_the_class_has_its_pattern(ints, name):
    mc.check_property(name, ints(name))


@pytest.mark.parametrize("name", list(mc.CLASSES))
def test_the_case_is_a_well_formed_call(name):
    """whole waves; pixels inside the frame; the decoy of every wave stores nothing; one key, one pixel among the storing lanes of the call; keys
    not negative; guards as documented -- what dr_kat_store_merged would refuse is not in a case"""
    c = mc.case(name)
    assert c.store_me.shape == c.key_.shape == c.x.shape == c.y.shape == (c.n_waves, 64) and c.color.shape == (c.n_waves, 64, 3)
    assert c.lds_in.shape == (c.n_waves, mc.ROWS, 64) and c.acc.shape == (c.W, mc.H, 3) and c.acc.dtype == np.int32
    assert ((c.x >= 0) & (c.x < c.W) & (c.y >= 0) & (c.y < mc.H)).all()
    m = c.mask
    assert (c.key_[m] >= 0).all()
    pixel_of = {}
    for k, x, y in zip(c.key_[m].tolist(), c.x[m].tolist(), c.y[m].tolist()):
        assert pixel_of.setdefault(k, (x, y)) == (x, y), "key %d names two pixels" % k
    if not c.shared:
        w = np.arange(c.n_waves)[:, None]
        assert (c.x // c.band == w).all(), "a lane outside its wave's band"
        decoy_x, decoy_y = (w + 1) * c.band - 1, mc.H - 1
        assert not (m & (c.x == decoy_x) & (c.y == decoy_y)).any() and ((c.x == decoy_x) & (c.y == decoy_y))[~m].all()
    assert (c.lds_in[:, 0] == mc.GUARD + np.arange(64)).all() and (c.lds_in[:, mc.ROWS - 1] == ~(mc.GUARD + np.arange(64))).all()


@pytest.mark.parametrize("name", list(mc.CLASSES))
def test_the_reference_is_the_naive_sum(ints, name):
    c = mc.case(name)
    ref = mc.reference(c, ints(name))
    assert ref.dtype == np.int32 and np.array_equal(ref, mc.reference_naive(c, ints(name)))
    assert c.mask.any() == (not np.array_equal(ref, c.acc)), "storing lanes change the accumulator"


def test_the_cases_are_the_seeds():
    """built twice, the same bytes: nothing in a case depends on the order the classes are asked for"""
    for name in ("fuzz", "collisions", "stale_lds"):
        a = mc.case(name)
        build, _, kw = mc.CLASSES[name]
        b = build(mc.Case(name, np.random.default_rng([mc.SEED, list(mc.CLASSES).index(name)]), **kw))
        for f in ("store_me", "key_", "x", "y", "color", "lds_in", "acc"):
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (name, f)


def test_the_fuzz_shares():
    shares = mc.fuzz_kinds(mc.case("fuzz"))
    print(shares)
    assert set(shares) == set(mc.FUZZ_KINDS) and min(shares.values()) >= 0.10, shares


def test_wrap32():
    a = np.array([0, 2 ** 31 - 1, 2 ** 31, -2 ** 31, -2 ** 31 - 1, 2 ** 32, 64 * (2 ** 31 - 1)], np.int64)
    assert mc.wrap32(a).tolist() == [0, 2 ** 31 - 1, -2 ** 31, -2 ** 31, 2 ** 31 - 1, 0, -64]


def test_the_wrapper_judges_shapes_before_the_library(monkeypatch):
    """Context.kat_store_merged is not in KAT_HOOKS (its accumulator goes in and out): it keeps the marshaller's rule -- a misshapen array is a
    ValueError that names it, before any library is asked for"""
    import dogeray_amd as dr

    class Touched(Exception):
        pass

    def touched():
        raise Touched()
    monkeypatch.setattr(dr, "lib", touched)
    ctx = dr.Context.__new__(dr.Context)      # no device behind it
    ctx._h = None
    c = mc.case("one_lane")
    good = dict(zip(("store_me", "key", "x", "y", "color"), c.lanes(0, 2)), acc=c.acc, lds_in=c.lds_in[:2])
    call = lambda **kw: (lambda a: ctx.kat_store_merged(2, a["store_me"], a["key"], a["x"], a["y"], a["color"], 1, a["acc"], a["lds_in"]))(dict(good, **kw))
    bad = {"key": good["key"][:-1], "x": good["x"][:-1], "y": np.zeros((128, 2), np.int32), "color": good["color"][:, :2], "acc": c.acc[:, :, :2],
           "lds_in": c.lds_in[:3]}
    for name, a in bad.items():
        with pytest.raises(ValueError) as e:
            call(**{name: a})
        assert str(e.value).startswith("kat_store_merged: %s must be [" % name), (name, str(e.value))
    with pytest.raises(Touched):
        call()
