"""The plain reference of the persistent kernel's tile-order feedback (DESIGN.md 4.3 "the order's contract"; dogeray_amd/csrc/kernels_aux.hip
tile_cost_kernel and tile_order_kernel), in Python integers and numpy sorts: no waves, ballots, histograms or scans.  It is written from the
contract, not from the kernel, and it is the only thing the device results are compared with; every comparison is between integers and exact.
Shared by tests/test_tile_order_host.py and tests/test_gpu_tile_order.py.

  tile_cost[t]  the maximum of the tile's 64 pixel costs
  rb[r]         ceil(r * ntiles / regions): region r owns tiles [rb[r], rb[r + 1])
  threshold     floor(sum(cost) * heavy_factor / ntiles) for heavy_factor > 0 (exact integers), 0 for heavy_factor < 0; heavy_factor == 0: no
                tile is heavy.  A tile is heavy iff cost > threshold; class = min(cost >> 4, 255)
  order         region after region: the region's heavy tiles by descending class (inside a class the device places them with atomics: any order,
                compared after sorting each class's run by tile number), then its light tiles, ascending
  starts        region_start[r] = rb[r], r <= regions
  counts        region_start[MAX_REGIONS + 1 + r] = min(#{heavy t in r: cost >> 4 >= split_steps >> 4}, split_limit // regions) if split_steps > 0
                else 0, r < regions
Words the persistent kernel never reads (regions < r <= MAX_REGIONS, counts of regions >= regions) are not compared."""
import numpy as np

MAX_REGIONS = 8
CLASSES = 256
WORDS = 2 * MAX_REGIONS + 1


def tile_cost(pixel_cost, ntiles):
    """uint32[ntiles]: the maximum over each tile's 64 words of the flat plane"""
    return np.ascontiguousarray(pixel_cost, dtype=np.uint32).ravel()[:ntiles * 64].reshape(ntiles, 64).max(axis=1)


def region_bounds(ntiles, regions):
    return [-((-r * ntiles) // regions) for r in range(regions + 1)]


def total_cost(cost):
    """the exact sum of a uint32 array as a Python int"""
    c = np.asarray(cost, dtype=np.uint32).astype(np.int64)
    return int((c >> 16).sum()) * 65536 + int((c & 0xffff).sum())


def threshold(cost, heavy_factor):
    """The cost a heavy tile exceeds, a Python int; None: no tile is heavy"""
    if heavy_factor == 0:
        return None
    if heavy_factor < 0:
        return 0
    return total_cost(cost) * heavy_factor // len(cost)


def heavy_mask(cost, heavy_factor):
    thr = threshold(cost, heavy_factor)
    if thr is None or thr >= 2 ** 32:
        return np.zeros(len(cost), dtype=bool)
    return np.asarray(cost, dtype=np.uint32).astype(np.int64) > thr


def classes(cost):
    return np.minimum(np.asarray(cost, dtype=np.uint32) >> 4, CLASSES - 1).astype(np.int64)


class Reference:
    """order (each class's run sorted by tile number), label[p] (the class at a heavy position p, -1 at a light one), rb, counts, heavy, cls"""

    def __init__(self, cost, regions, heavy_factor, split_steps, split_limit):
        cost = np.asarray(cost, dtype=np.uint32)
        n = len(cost)
        self.ntiles, self.regions = n, regions
        self.rb = region_bounds(n, regions)
        self.threshold = threshold(cost, heavy_factor)
        self.heavy = heavy_mask(cost, heavy_factor)
        self.cls = classes(cost)
        order, label, counts, long_ones = [], [], [], []
        for r in range(regions):
            t = np.arange(self.rb[r], self.rb[r + 1], dtype=np.int64)
            h = t[self.heavy[t]]
            h = h[np.lexsort((h, -self.cls[h]))]                   # descending class, then tile number
            order += [h, t[~self.heavy[t]]]
            label += [self.cls[h], np.full(len(t) - len(h), -1, dtype=np.int64)]
            long_ones.append(int(((cost[h] >> 4).astype(np.int64) >= (split_steps >> 4)).sum()) if split_steps > 0 else 0)
            counts.append(min(long_ones[-1], split_limit // regions))
        self.order = np.concatenate(order).astype(np.int32)
        self.label = np.concatenate(label)
        self.counts = counts
        self.long_ones = long_ones                  # before the limit

    def normalised(self, order):
        """`order` with every run of one class sorted by tile number.  The runs are the reference's: positions of one region over which its
        label stays the same (a run ends at a region bound even where the next region begins with the same class)"""
        out = np.array(order, dtype=np.int64)
        cut = np.zeros(self.ntiles + 1, dtype=bool)
        cut[1:self.ntiles] = np.diff(self.label) != 0
        cut[self.rb] = True
        edges = np.flatnonzero(cut)
        for lo, hi in zip(edges[:-1], edges[1:]):
            if self.label[lo] >= 0:
                out[lo:hi] = np.sort(out[lo:hi])
        return out.astype(np.int32)


def first_difference(ref, order, region_start):
    """None when a device result (order int32[ntiles], region_start int32[17]) is the reference's, else a description of the first difference"""
    n, regions = ref.ntiles, ref.regions
    order = np.asarray(order)
    region_start = np.asarray(region_start)
    if order.shape != (n,):
        return "order has shape %r, not (%d,)" % (order.shape, n)
    if region_start.shape != (WORDS,):
        return "region_start has shape %r" % (region_start.shape,)
    bad = np.flatnonzero((order < 0) | (order >= n))
    if len(bad):
        return "order[%d] = %d is no tile (%d entries outside [0, %d), -1 = never written)" % (bad[0], order[bad[0]], len(bad), n)
    seen = np.bincount(order, minlength=n)
    if (seen != 1).any():
        t = int(np.flatnonzero(seen != 1)[0])
        return "tile %d appears %d times in the order (%d tiles missing, %d more than once)" % (t, seen[t], int((seen == 0).sum()), int((seen > 1).sum()))
    for r in range(regions + 1):
        if int(region_start[r]) != ref.rb[r]:
            return "region_start[%d] = %d, expected %d" % (r, region_start[r], ref.rb[r])
    for r in range(regions):
        lo, hi = ref.rb[r], ref.rb[r + 1]
        out = np.flatnonzero((order[lo:hi] < lo) | (order[lo:hi] >= hi))
        if len(out):
            return "position %d (region %d) holds tile %d of another region" % (lo + out[0], r, order[lo + out[0]])
    label = np.where(ref.heavy[order], ref.cls[order], -1)
    bad = np.flatnonzero(label != ref.label)
    if len(bad):
        p = int(bad[0])
        say = lambda v: "light" if v < 0 else "heavy of class %d" % v
        return "position %d holds tile %d (%s), expected a tile that is %s" % (p, order[p], say(label[p]), say(ref.label[p]))
    light = ref.label < 0
    bad = np.flatnonzero(light & (order != ref.order))
    if len(bad):
        p = int(bad[0])
        return "light tiles out of their natural order: position %d holds tile %d, expected %d" % (p, order[p], ref.order[p])
    norm = ref.normalised(order)
    bad = np.flatnonzero(norm != ref.order)
    if len(bad):
        p = int(bad[0])
        return "after sorting each class's run: position %d holds tile %d, expected %d" % (p, norm[p], ref.order[p])
    for r in range(regions):
        got = int(region_start[MAX_REGIONS + 1 + r])
        if got != ref.counts[r]:
            return "split count of region %d = %d, expected %d" % (r, got, ref.counts[r])
    return None
