#!/usr/bin/env python3
"""Regenerates tests/golden/shade_sampler_seeds.json: generator states for the rejection samplers' known-answer tests (tests/shade_cases.py) that the 2^20
states of the seed formula do not hold -- states in which the plain loop ACCEPTS a candidate whose approximate squared length, as the merged loop's 32-bit
classification forms it, is 1 or more.  They are what the 2^-16 in the merged loop's threshold is for; a loop that rejected at 1 would draw another point
for them.  About one candidate in a hundred million is one, so they are searched for: the seeds i >= 2^20 of the same formula (i * 0x9E3779B97F4A7C15 + 12345)
without a warm-up, the generator restated in numpy, the first candidate of each classified by tests/shade_checks.py candidate() for either kind.  The tests
check every state of the list again, on the oracle's words.  Run from the repo root:  python tests/golden/make_shade_seeds.py [states to scan [processes]]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shade_cases as sc          # noqa: E402
import shade_checks as ck         # noqa: E402

U32 = np.uint32


class Xorwow:
    """cuRAND's XORWOW on arrays of states: curand_init(seed, 0, 0) and curand()"""

    def __init__(self, seed):
        s0 = (seed & np.uint64(0xFFFFFFFF)).astype(U32) ^ U32(0xaad26b49)
        s1 = (seed >> np.uint64(32)).astype(U32) ^ U32(0xf7dcefdd)
        t0, t1 = U32(1099087573) * s0, U32(2591861531) * s1
        self.d = U32(6615241) + t1 + t0
        self.v = [U32(123456789) + t0, U32(362436069) ^ t0, U32(521288629) + t1, U32(88675123) ^ t1, U32(5783321) + t0]

    def next(self, mask=None):
        v = self.v
        t = v[0] ^ (v[0] >> U32(2))
        new = (v[4] ^ (v[4] << U32(4))) ^ (t ^ (t << U32(1)))
        nv = [v[1], v[2], v[3], v[4], new]
        nd = self.d + U32(362437)
        if mask is not None:
            nv = [np.where(mask, a, b) for a, b in zip(nv, v)]
            nd = np.where(mask, nd, self.d)
        self.v, self.d = nv, nd
        return self.v[4] + self.d


def scan(first, count):
    """the seeds i * 0x9E3779B97F4A7C15 + 12345, i in [first, first + count), without a warm-up: their FIRST candidate as a sphere lane (six words) and as
    a disk lane (the first four of them) draws it"""
    i = np.arange(first, first + count, dtype=np.uint64)
    seed = i * np.uint64(sc.GOLDEN_RATIO) + np.uint64(12345)
    g = Xorwow(seed)
    w = [g.next() for _ in range(6)]
    out = []
    for kind in (3, 2):
        d2, rejected, d2a = ck.candidate(w, np.full(count, kind == 3))
        out += [{"seed": int(s), "warm": 0, "kind": kind} for s in seed[~rejected & (d2a >= np.float32(1))]]
    return out


def scan_chunk(first):
    with np.errstate(over="ignore"):
        return scan(first, 1 << 20)


if __name__ == "__main__":
    from multiprocessing import Pool
    total = int(sys.argv[1]) if len(sys.argv) > 1 else 1024 << 20
    out = []
    with Pool(int(sys.argv[2]) if len(sys.argv) > 2 else 8) as pool:
        for k, found in enumerate(pool.imap(scan_chunk, range(sc.SAMPLER_N, sc.SAMPLER_N + total, 1 << 20))):
            out += found
            if k % 64 == 63:
                print("scanned %d M states, %d found" % (k + 1, len(out)), flush=True)
    with open(os.path.join(ROOT, "tests", "golden", "shade_sampler_seeds.json"), "w") as f:
        json.dump({"what": "states whose accepted candidate has an approximate squared length >= 1 (make_shade_seeds.py)", "states": out}, f, indent=1)
        f.write("\n")
