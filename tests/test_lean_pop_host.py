"""The lean six-wave build's pop (dogeray_amd/csrc/device_wide.hpp wide_pop_lean) against wide_pop, through tools/host_kernel.cpp: the same headers
compiled for the host.  On every word and stack state a walk can reach -- a word is first child << 8 | leaf mask << 4 | pending mask with a pending
mask that is never empty and a first child of 1 or more (record 0 is the root) --

  * the register word `top` non-zero: all 15 pending masks x all 16 leaf masks, first children at both ends of the 24-bit range;
  * `top` zero with the same words as the newest of the stack: the pop reads it from there;
  * the stack pointer 0, 1 and WIDE_STACK (16), with the word the pop may read at sp - 1 and other words below it;
  * `top` zero and the stack empty: the walk is over (LANE_DONE, -1);

the next record, the remaining word and the stack pointer must be equal.  No GPU.

What this does not run: the host build compiles the two primitives the pop rests on as plain C++ (tools/host_kernel/host_prims.hpp lowest_bit,
at_least_minus_one), not the device's inline v_ffbl_b32 and v_max_i32.  That v_ffbl_b32 of 0 is -1 and that the max of -2 and -1 is -1 on the GPU is
exercised by tests/test_gpu_lean_pop.py, whose every walk ends with a pop from an empty stack."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

WIDE_STACK = 16
BASES = (1, 2, 3, 0x1234, 0x7FFFFF, 0x800000, 0xFFFFFC)      # first children: the smallest (record 0 is the root), and around the index's 24 bits
SPS = (0, 1, WIDE_STACK)


def words():
    return np.array([(b << 8) | (leaf << 4) | pend for b in BASES for leaf in range(16) for pend in range(1, 16)], dtype=np.uint32)


@pytest.fixture(scope="module")
def states():
    """(top uint32[n], sp int32[n], stack uint32[n, 16]): every word as `top` and as the stack's newest word under an empty `top`, at every stack pointer"""
    W = words()
    other = np.uint32((0x55 << 8) | (0x3 << 4) | 0x5)      # what the rest of the stack holds: a word no case pops
    top, sp, stack = [], [], []
    for s in SPS:
        for w in W:      # the register word holds the pending children: the stack is not read
            top.append(w); sp.append(s); stack.append(np.full(WIDE_STACK, other, np.uint32))
        if s > 0:
            for w in W:      # the register word is empty: the newest stack word is popped
                st = np.full(WIDE_STACK, other, np.uint32)
                st[s - 1] = w
                top.append(0); sp.append(s); stack.append(st)
        else:
            top.append(0); sp.append(0); stack.append(np.full(WIDE_STACK, other, np.uint32))      # nothing left
    return np.array(top, np.uint32), np.array(sp, np.int32), np.array(stack, np.uint32)


@pytest.fixture(scope="module")
def both(states):
    import host_kernel
    host_kernel.build()
    return host_kernel.lean_pop(*states)


def test_the_cases_cover_the_issue(states):
    top, sp, stack = states
    nz = top != 0
    assert {(int(w) & 15, (int(w) >> 4) & 15) for w in top[nz]} == {(p, l) for p in range(1, 16) for l in range(16)}
    popped = stack[~nz & (sp > 0), :][np.arange((~nz & (sp > 0)).sum()), sp[~nz & (sp > 0)] - 1]
    assert {(int(w) & 15, (int(w) >> 4) & 15) for w in popped} == {(p, l) for p in range(1, 16) for l in range(16)}
    for s in SPS:
        assert (nz & (sp == s)).any() and (~nz & (sp == s)).any()


def test_wide_pop_is_what_the_header_says(states, both):
    """the reference form itself against a plain restatement: the lowest pending child of the newest word, or -1"""
    top, sp, stack = states
    plain = both[0]
    for i in range(len(top)):
        w, s = int(top[i]), int(sp[i])
        if w == 0:
            if s == 0:
                assert tuple(plain[i]) == (-1, 0, 0)
                continue
            s -= 1
            w = int(stack[i, s])
        j = (w & -w).bit_length() - 1
        assert j < 4
        node = (((w >> 8) + j) << 1) | ((w >> (4 + j)) & 1)
        rest = w & (w - 1)
        rest = rest if rest & 15 else 0
        assert (int(plain[i, 0]), int(plain[i, 1]) & 0xFFFFFFFF, int(plain[i, 2])) == (node, rest, s)


def test_lean_pop_equals_wide_pop(states, both):
    plain, lean = both
    bad = np.nonzero((plain != lean).any(axis=1))[0]
    assert bad.size == 0, "first difference at top %#x sp %d: wide_pop %r, wide_pop_lean %r" % (
        states[0][bad[0]], states[1][bad[0]], tuple(plain[bad[0]]), tuple(lean[bad[0]]))
