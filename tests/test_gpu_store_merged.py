"""The stores of a batched launch on lane patterns the test chooses (dr_kat_store_merged; dogeray_amd/csrc/device_shade.hpp): form 0 store_pixel with
every storing lane adding on its own, form 1 store_pixels_merged (DPP: a turn and a wave_sum per distinct key -- only the variant libraries ship it),
form 2 store_pixels_merged_lds (five LDS words per slot: what every default launch of more than one frame stores through).  The cases and the
reference are tests/merge_cases.py: whole waves of 64 lanes, a class per edge the merge was written around, and a reference that adds the storing
lanes' integers -- the oracle's kat_store of their colours -- per pixel in int64 and wraps once.  tests/test_merge_cases_host.py holds, without a GPU,
that every class has its pattern.  A class is one call per form; every comparison is integer equality.

What this does not claim: the hook compiles the merge functions into a small kernel of its own, so it pins the source's logic for every lane pattern,
not the instruction schedule the compiler gives the same source inside render_persistent_kernel.  That stays the business of the end-to-end byte
comparisons (tests/test_gpu_sample_order.py and the batch tests)."""
import ctypes as C

import numpy as np
import pytest

import merge_cases as mc
import shade_checks as ck

pytestmark = pytest.mark.gpu

I32 = np.int32
FORMS = (0, 1, 2)
FORM_NAME = {0: "form 0 (store_pixel)", 1: "form 1 (store_pixels_merged)", 2: "form 2 (store_pixels_merged_lds)"}
NAMES = list(mc.CLASSES)


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    return dogeray_amd


@pytest.fixture(scope="module")
def ctx(dr):
    c = dr.Context(0)          # no scene: the stores read the sample scale alone
    yield c
    c.close()


@pytest.fixture(scope="module")
def want():
    """class -> the reference accumulator, computed once"""
    cache = {}

    def of(name):
        if name not in cache:
            c = mc.case(name)
            ints = mc.lane_integers(c, ck.orc().kat_store)
            mc.check_property(name, ints)
            ref = mc.reference(c, ints)
            ref.flags.writeable = False
            cache[name] = ref
        return cache[name]
    return of


def run(ctx, c, form, first=0, last=None, acc=None):
    return ctx.kat_store_merged(form, *c.lanes(first, last), c.spp, c.acc if acc is None else acc, c.lds_in[first:last])


@pytest.fixture(scope="module")
def got(ctx):
    """(class, form) -> (accumulator, LDS rows) of the hook, run once"""
    cache = {}

    def of(name, form):
        if (name, form) not in cache:
            cache[name, form] = run(ctx, mc.case(name), form)
        return cache[name, form]
    return of


def first_difference(c, acc, ref):
    """the first pixel that differs, its wave, and the lanes that store into it with their keys"""
    x, y = (int(v) for v in np.argwhere((acc != ref).any(axis=2))[0])
    on = np.argwhere(c.mask & (c.x == x) & (c.y == y))
    lanes = ", ".join("wave %d lane %d key %d (slot %d)" % (w, l, c.key_[w, l], c.key_[w, l] & 63) for w, l in on[:70])
    wave = "every wave" if c.shared else "wave %d" % (x // c.band)
    more = "" if c.shared or on.size == 0 else "; the wave's storing lanes by key: %s" % {
        int(k): np.flatnonzero(c.mask[on[0][0]] & (c.key_[on[0][0]] == k)).tolist() for k in np.unique(c.key_[on[0][0]][c.mask[on[0][0]]])}
    return "%d pixels differ; first (%d, %d) of %s: got %s, want %s, started at %s; stored by [%s]%s" % (
        int((acc != ref).any(axis=2).sum()), x, y, wave, acc[x, y].tolist(), ref[x, y].tolist(), c.acc[x, y].tolist(), lanes or "no lane (the decoy, or a pixel nothing stores)", more)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_the_accumulator_is_the_plain_sum(got, want, name, form):
    c, ref = mc.case(name), want(name)
    acc, _ = got(name, form)
    assert acc.shape == ref.shape and acc.dtype == I32
    same = np.array_equal(acc, ref)
    print("%s, %s: %d waves, %d storing lanes, %s" % (name, FORM_NAME[form], c.n_waves, int(c.mask.sum()), "equal" if same else "DIFFERENT"))
    assert same, "class %s, %s: %s" % (name, FORM_NAME[form], first_difference(c, acc, ref))


@pytest.mark.parametrize("name", NAMES)
def test_the_three_forms_return_the_same_bytes(got, name):
    a = [got(name, f)[0].tobytes() for f in FORMS]
    if a[0] == a[1] == a[2]:
        return
    odd = [f for f in FORMS if sum(a[f] == a[g] for g in FORMS) == 1]
    assert False, "class %s: %s" % (name, "all three differ" if len(odd) == 3 else FORM_NAME[odd[0]] + " is the odd one out: " +
                                    first_difference(mc.case(name), got(name, odd[0])[0], got(name, (odd[0] + 1) % 3)[0]))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_the_lds_rows(got, name, form):
    """the guards as they came, for every form; forms 0 and 1 touch no LDS word; form 2 only the five words of the slots that a storing lane's key
    addresses"""
    c = mc.case(name)
    _, rows = got(name, form)
    assert rows.shape == c.lds_in.shape and rows.dtype == I32
    where = lambda bad: "wave %d row %d column %d" % tuple(int(v) for v in np.argwhere(bad)[0])
    for r in (0, mc.ROWS - 1):
        bad = rows[:, r:r + 1] != c.lds_in[:, r:r + 1]
        assert not bad.any(), "class %s, %s: guard row %d written (%s)" % (name, FORM_NAME[form], r, where(bad))
    bad = rows != c.lds_in
    if form == 2:
        bad = bad & mc.untouched_slots(c)[:, None, :]
        assert not bad.any(), "class %s, %s: a slot no storing lane addresses was written (%s)" % (name, FORM_NAME[form], where(bad))
        addressed = ~mc.untouched_slots(c)
        assert (rows[:, mc.ROW_KEY][addressed] & 63 == np.argwhere(addressed)[:, 1]).all(), "an addressed slot holds a key of its own"
    else:
        assert not bad.any(), "class %s, %s: LDS written (%s)" % (name, FORM_NAME[form], where(bad))


# ------------------------------------------------------------------ staging
@pytest.mark.parametrize("form", FORMS)
def test_five_waves_are_four_and_one(ctx, form):
    """a workgroup boundary: the fifth wave is the first of the second workgroup.  The waves of across_waves all store into the same two pixels."""
    c = mc.case("across_waves")
    whole = run(ctx, c, form, 0, 5)
    head = run(ctx, c, form, 0, 4)
    tail = run(ctx, c, form, 4, 5, acc=head[0])
    assert not np.array_equal(head[0], c.acc) and not np.array_equal(tail[0], head[0])
    assert np.array_equal(whole[0], tail[0]), first_difference(c, whole[0], tail[0])
    assert whole[1].shape == (5, mc.ROWS, 64) and np.array_equal(whole[1], np.concatenate([head[1], tail[1]]))


@pytest.mark.parametrize("form", FORMS)
def test_no_lanes_return_the_accumulator_as_given(ctx, form):
    c = mc.case("one_pixel")
    acc, rows = run(ctx, c, form, 0, 0)
    assert acc.dtype == I32 and np.array_equal(acc, c.acc) and rows.shape == (0, mc.ROWS, 64)


def test_refusals_leave_the_arrays_alone(dr, ctx):
    """every refusal of the contract (include/dogeray_amd.h dr_kat_store_merged) through ctypes: DR_ERR_INVALID, a message, and acc and lds_out as they
    were -- the checks run on the host before anything is staged, so a pixel outside the frame never reaches the kernel, which has no test of its own"""
    f = dr.lib().dr_kat_store_merged
    c = mc.case("collisions")
    W = c.band
    lanes = [np.array(a) for a in c.lanes(0, 1)]
    first = int(np.flatnonzero(lanes[0])[0])
    other = int(np.flatnonzero(lanes[0] & (lanes[1] != lanes[1][first]))[0])
    assert lanes[0][[first, other]].all() and (lanes[2][first], lanes[3][first]) != (lanes[2][other], lanes[3][other])
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    fresh = lambda: (np.full(W * mc.H * 3 * 4, 0x5a, np.uint8).view(I32), np.full(mc.ROWS * 64 * 4, 0x5a, np.uint8).view(I32))

    def call(form=2, n=64, spp=1, w=W, h=mc.H, edit=None, null=None):
        arrays = [a.copy() for a in lanes]
        if edit:
            edit(*arrays)
        acc, out = fresh()
        ptrs = arrays + [acc, np.array(c.lds_in[0]), out]
        if null is not None:
            ptrs[null] = None
        rc = f(ctx._h, form, n, *[p(a) for a in ptrs[:5]], spp, w, h, p(ptrs[5]), p(ptrs[6]), p(ptrs[7]))
        untouched = all(a.tobytes() == b.tobytes() for a, b in zip((acc, out), fresh()))
        return rc, dr.lib().dr_last_error(), untouched

    for form in FORMS:
        rc, _, untouched = call(form=form)
        assert rc == 0 and not untouched, "a well-formed call writes acc and lds_out"

    def set_(k, lane, v):
        def edit(*arrays):
            arrays[k][lane] = v
        return edit
    refused = {
        "form -1": dict(form=-1), "form 3": dict(form=3), "n_lanes 63": dict(n=63), "n_lanes 1": dict(n=1), "spp 0": dict(spp=0), "spp -1": dict(spp=-1),
        "W 0": dict(w=0), "H 0": dict(h=0), "W -1": dict(w=-1),
        "H one row short": dict(h=int(lanes[3][lanes[0] != 0].max())),
        "x = W": dict(edit=set_(2, first, W)), "x = -1": dict(edit=set_(2, first, -1)), "x = 2^31 - 1": dict(edit=set_(2, first, 2 ** 31 - 1)),
        "y = H": dict(edit=set_(3, first, mc.H)), "y = -1": dict(edit=set_(3, first, -1)), "y = -2^31": dict(edit=set_(3, first, -2 ** 31)),
        "a negative key": dict(edit=set_(1, first, -1)),
        "one key, two pixels": dict(edit=set_(1, other, int(lanes[1][first]))),
    }
    for what, kw in refused.items():
        for form in FORMS if "form" not in kw else (kw["form"],):
            rc, msg, untouched = call(**dict(kw, form=form))
            assert rc == dr.ERR_INVALID and msg.startswith(b"store_merged: "), (what, form, rc, msg)
            assert untouched, "%s: a refused call leaves the caller's arrays alone" % what
    for k in range(8):
        rc, msg, untouched = call(null=k)
        assert rc == dr.ERR_INVALID and msg == b"null argument" and untouched, (k, rc, msg)

    def one_pixel(store_me, key, x, y, color):      # allowed: two keys for one pixel are two groups that add to the same words
        x[:], y[:] = x[first], y[first]
    for form in FORMS:
        rc, _, untouched = call(form=form, edit=one_pixel)
        assert rc == 0 and not untouched
