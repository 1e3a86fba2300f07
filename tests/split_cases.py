"""The split of a launch's tile order (dogeray_amd/csrc/device_split.hpp order_split_plain), independent of the source under test: the stable partition
restated in numpy, and the one generator of its cases.  Shared by tests/test_sky_tiles_host.py and tests/test_adaptive_host.py (the host build's
hk_sky_split / hk_subset_split), tests/test_gpu_order_split.py (the kernel, through dr_kat_order_split) and whoever needs the partition of a pass."""
import numpy as np

MAX_REGIONS = 8
ENTRY_SHIFT = 3
KINDS = ("random", "none", "all", "region", "random", "random")      # of a case's kept tiles: "region" empties one whole region


def partition(order, region_start, kept, regions):
    """(launch_order, launch_region_start int32[17], dropped tiles): the kept tiles of the order (None: the identity) in the order they had; region
    r's compacted start is the number of kept tiles at the positions in front of region_start[r], [regions] the kept tiles, the split counts [9 ..]
    0; the dropped tiles in ascending tile number"""
    kept = np.asarray(kept) != 0
    tiles = len(kept)
    order = np.arange(tiles, dtype=np.int32) if order is None else np.asarray(order, np.int32)
    stays = kept[order]
    before = np.concatenate([[0], np.cumsum(stays)])      # kept tiles in front of position i
    lrs = np.zeros(2 * MAX_REGIONS + 1, np.int32)
    lrs[:regions + 1] = before[np.minimum(np.asarray(region_start[:regions + 1], np.int64), tiles)]
    return order[stays].astype(np.int32), lrs, np.nonzero(~kept)[0].astype(np.int32)


def bands(tiles, regions):
    """make_params' regions of the identity order"""
    return np.array([(tiles * r + regions - 1) // regions for r in range(regions + 1)], np.int32)


class Case:
    """kind, identity; order (None: the identity), rs int32[regions + 1], kept bool[tiles]; emptied: the region a "region" case empties, else None"""

    def __init__(self, kind, identity, order, rs, kept, emptied):
        self.kind, self.identity, self.order, self.rs, self.kept, self.emptied = kind, identity, order, rs, kept, emptied

    def rs_in(self):
        """region_start as a caller holds it, 17 ints: what lies behind [regions] is not read"""
        return np.concatenate([self.rs, np.full(2 * MAX_REGIONS + 1 - len(self.rs), 7, np.int32)])

    def held(self, r):
        """the tiles at region r's positions"""
        full = np.arange(len(self.kept), dtype=np.int32) if self.order is None else self.order
        return full[self.rs[r]:self.rs[r + 1]]


def cases(rng, regions, tiles):
    """the six kinds x (a permuted order with random cuts -- empty regions, and regions that start at `tiles`, among them --, the identity with
    make_params' bands): twelve cases"""
    for kind in KINDS:
        for identity in (False, True):
            if identity:
                rs, order = bands(tiles, regions), None
            else:
                cuts = np.sort(rng.integers(0, tiles + 1, regions - 1)).astype(np.int32)
                rs = np.concatenate([[0], cuts, [tiles]]).astype(np.int32)
                order = rng.permutation(tiles).astype(np.int32)
            kept = rng.random(tiles) < rng.random()
            if kind == "none": kept[:] = False
            if kind == "all": kept[:] = True
            c = Case(kind, identity, order, rs, kept, int(rng.integers(0, regions)) if kind == "region" else None)
            if kind == "region": kept[c.held(c.emptied)] = False
            yield c


def flags(kept):
    """the adaptive side's key: a byte per tile"""
    return np.asarray(kept).astype(np.uint8)


def words(rng, kept):
    """the sky side's key: a word per tile, entry code << ENTRY_SHIFT | grade -- code -1 for the dropped (sky) tiles, a record (or the root) for the kept"""
    code = np.where(kept, rng.integers(0, 1 << 20, len(kept)) * rng.integers(0, 2, len(kept)), -1).astype(np.int64)
    return ((code << ENTRY_SHIFT) | rng.integers(0, 6, len(kept))).astype(np.int64).astype(np.uint32)
