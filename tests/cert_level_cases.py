"""The scenes and views of the graded grazing certificate's tests (option cert_levels), shared by the host and the GPU test:
hf_small scaled by 0.1 and by 0.02 -- its triangles enter the wide tree with their own bounds -- seen low and grazing, from straight above, through
a wide lens and from the scene's own camera, at 320x192 and 160x96."""
import numpy as np

SCALES = (0.1, 0.02)
SIZES = ((320, 192), (160, 96))
VIEWS = ("graze", "top", "wide", "scene")
LADDER = (0.25, 0.5, 1.0, 2.0, 4.0)      # option cert_levels = 1: cert_factor times these, each at least 1


def view(base13, name, scale):
    """settings13 of view `name` from the scene's own (pack_settings13), for hf_small scaled by `scale`"""
    st = np.array(base13, np.float32).copy()
    if name == "scene":
        return st
    st[7] = np.float32(20.0)                                 # |d| of a camera ray as long as the bench view's
    if name == "graze":
        st[1] = st[4] + np.float32(3.0 * scale)              # the eye a fraction of the scene's height above the target: the hill backs edge-on
    elif name == "top":
        st[0] = st[3] + np.float32(0.01 * scale); st[2] = st[5]; st[1] = st[4] + np.float32(30.0 * scale)
    elif name == "wide":
        st[1] = st[4] + np.float32(1.0 * scale); st[6] = np.float32(0.1)      # a wide lens: the tile projection's lens term
    else:
        raise KeyError(name)
    return st


def ladder(cert_factor):
    """the ladder's steps in units of the 1e-4 cut-off"""
    return [max(1.0, cert_factor * m) for m in LADDER]


def mask_bits(words, ntiles):
    """hk_cert_check's mask words (tile bits, then the "every tile" word) as one bool per tile"""
    nwords = (ntiles + 31) // 32
    if words[nwords]:
        return np.ones(ntiles, bool)
    return np.unpackbits(words[:nwords].view(np.uint8), bitorder="little")[:ntiles].astype(bool)
