"""export._place on the host: the first-fit arena a plan file's activation blocks live in (planer_amd/export.py; the run side,
csrc/plan_exec.hip, adds each offset to ONE allocation, so two blocks that are live together and share a byte are a wrong
answer nothing else reports).  `check_placement` is what tests/test_gpu_plan_file_kinds.py holds the real event list of every
exported net to; here it runs on event lists made by hand and by a seeded generator.

An event list is what export._Recorder keeps: ("alloc", id, bytes) | ("free", id) | ("call", ...), in order.  A block lives from
its alloc to its free; a `pinned` id (the plan's inputs and outputs) is never freed, whatever the list says.

What first fit guarantees, and `check_placement` asserts:
  * the arena grows only when no hole fits: at an alloc that is placed at the old top T, no gap between the live blocks below T
    holds the block (a placement that forgets a free fails here, and nowhere else);
  * hence the size bound.  Let A = 256 be the alignment, s the aligned size of the block that makes the arena grow, and L, k the
    bytes and the number of the blocks live at that moment.  [0, T) is those k blocks and the gaps between them, at most k + 1
    (holes are coalesced: two gaps have a live block between them), each a multiple of A and smaller than s, so at most s - A:
    T <= L + (k + 1)(s - A), and the new top is T + s.  The top moves at no other time, so
        arena <= max over allocs of  L + s + (k + 1)(s - A).
    With M the peak of the live bytes (aligned sizes; L + s <= M), S_max and S_min the largest and smallest aligned size and
    K >= k + 1 the peak number of live blocks, K S_min <= M gives the closed form
        arena <= M (1 + (S_max - A) / S_min).
"""
import numpy as np
import pytest

from planer_amd.export import _ALIGN, _place


def aligned(nbytes):
    return (max(int(nbytes), 1) + _ALIGN - 1) // _ALIGN * _ALIGN


def check_placement(events, pinned, offsets, arena, what=""):
    """`offsets`, `arena` = _place(events, pinned) keep every promise in the module docstring.  -> (peak live bytes, blocks)."""
    pinned = set(pinned)
    live, top, peak, bound, sizes, peak_count = {}, 0, 0, 0, [], 0            # live: id -> (offset, aligned bytes)
    for t, ev in enumerate(events):
        if ev[0] == "alloc":
            _, bid, nbytes = ev
            need = aligned(nbytes)
            assert bid in offsets and bid not in live, (what, "event %d: block %r placed twice or not at all" % (t, bid))
            off = offsets[bid]
            assert off % _ALIGN == 0, (what, "block %r at %d: not %d-aligned" % (bid, off, _ALIGN))
            for other, (o, sz) in live.items():
                assert off + need <= o or o + sz <= off, (
                    what, "event %d: block %r [%d, %d) overlaps block %r [%d, %d), which is still live" % (t, bid, off, off + need, other, o, o + sz))
            held, count = sum(sz for _, sz in live.values()), len(live)
            if off >= top:                                  # the arena grows: no hole below the old top held the block
                assert off == top, (what, "event %d: block %r at %d leaves a gap above the top %d" % (t, bid, off, top))
                at = 0
                for o, sz in sorted(live.values()) + [(top, 0)]:
                    assert o - at < need, (what, "event %d: the arena grows by block %r (%d bytes) although [%d, %d) is free"
                                           % (t, bid, need, at, o))
                    at = max(at, o + sz)
            bound = max(bound, held + need + (count + 1) * (need - _ALIGN))
            live[bid] = (off, need)
            sizes.append(need)
            top = max(top, off + need)
            peak, peak_count = max(peak, held + need), max(peak_count, count + 1)
        elif ev[0] == "free" and ev[1] not in pinned:
            assert ev[1] in live, (what, "event %d frees block %r, which is not live" % (t, ev[1]))
            del live[ev[1]]
    assert arena == top, (what, "arena %d, the highest block ends at %d" % (arena, top))
    assert arena <= bound, (what, "arena %d above what first fit guarantees for this list, %d" % (arena, bound))
    if sizes:
        assert arena <= peak * (1 + (max(sizes) - _ALIGN) / min(sizes)), (what, arena, peak, max(sizes), min(sizes))
    return peak, len(sizes)


def _checked(events, pinned=()):
    offsets, arena = _place(events, set(pinned))
    check_placement(events, pinned, offsets, arena)
    return offsets, arena


def test_interleaved_allocations_and_frees_reuse_the_holes():
    A = _ALIGN
    events = [("alloc", 0, 3 * A), ("alloc", 1, A), ("alloc", 2, 2 * A), ("free", 0), ("alloc", 3, 2 * A), ("call", "pl_x", []),
              ("alloc", 4, A), ("free", 2), ("alloc", 5, 2 * A), ("free", 1), ("free", 4), ("alloc", 6, 2 * A)]
    offsets, arena = _checked(events)
    assert offsets == {0: 0, 1: 3 * A, 2: 4 * A, 3: 0, 4: 2 * A, 5: 4 * A, 6: 2 * A} and arena == 6 * A


def test_sizes_are_rounded_up_and_zero_byte_blocks_take_a_slot_of_their_own():
    events = [("alloc", 0, 0), ("alloc", 1, 1), ("alloc", 2, 255), ("alloc", 3, 256), ("alloc", 4, 257), ("alloc", 5, 0),
              ("free", 0), ("alloc", 6, 0), ("free", 4), ("alloc", 7, 300)]
    offsets, arena = _checked(events)
    assert [offsets[i] for i in range(8)] == [0, 256, 512, 768, 1024, 1536, 0, 1024] and arena == 1792
    assert len({offsets[i] for i in (1, 2, 3, 5, 6, 7)}) == 6           # live together: no two at one address, the empty ones included


def test_a_pinned_block_is_never_reused_whatever_the_list_frees():
    A = _ALIGN
    events = [("alloc", 0, A), ("alloc", 1, 4 * A), ("alloc", 2, A), ("free", 1), ("free", 0), ("alloc", 3, 4 * A), ("alloc", 4, A),
              ("free", 2), ("alloc", 5, A)]
    offsets, arena = _checked(events, pinned={1})
    assert offsets[3] == 6 * A and offsets[4] == 0 and offsets[5] == 5 * A and arena == 10 * A
    unpinned, small = _checked(events)
    assert unpinned[3] == 0 and unpinned[4] == 4 * A and small == 6 * A    # (blocks 0 and 1 freed: one hole of 5 A)


def test_three_neighbours_coalesce_into_one_hole():
    A = _ALIGN
    events = [("alloc", i, A) for i in range(5)] + [("free", 1), ("free", 3), ("free", 2), ("alloc", 5, 3 * A)]
    offsets, arena = _checked(events)
    assert offsets[5] == A and arena == 5 * A                           # freed in the order left, right, middle: one hole of 3 A
    events = [("alloc", i, A) for i in range(5)] + [("free", 1), ("free", 3), ("alloc", 5, 2 * A)]
    offsets, arena = _checked(events)
    assert offsets[5] == 5 * A and arena == 7 * A                       # two holes of A with a live block between them: no fit


def random_events(seed, n=2000):
    """A seeded list of n events: sizes from 0 to 64 KiB with the alignment's neighbours among them, frees of random live blocks,
    calls in between, and every eighth block pinned -- its free is in the list all the same."""
    r = np.random.default_rng(seed)
    events, live, pinned, nid = [], [], set(), 0
    while len(events) < n:
        u = r.random()
        if u < 0.1:
            events.append(("call", "pl_x", []))
        elif u < 0.55 or not live:
            size = int(r.choice([0, 1, 255, 256, 257, 512, int(r.integers(1, 4096)), int(r.integers(4096, 65536))]))
            events.append(("alloc", nid, size))
            live.append(nid)
            if nid % 8 == 5:
                pinned.add(nid)
            nid += 1
        else:
            events.append(("free", live.pop(int(r.integers(len(live))))))
    return events, pinned


@pytest.mark.parametrize("seed", range(4))
def test_random_event_lists(seed):
    events, pinned = random_events(seed)
    offsets, arena = _place(events, pinned)
    peak, blocks = check_placement(events, pinned, offsets, arena, "seed %d" % seed)
    assert blocks > 700 and peak > 1 << 18               # (the generator's own reach: hundreds of blocks, dozens live at a time)


def test_the_checker_sees_a_block_freed_early_and_a_free_forgotten():
    """What check_placement is for: offsets computed from a list in which one free comes early put two live blocks on the same
    bytes, and offsets computed from a list that lacks one free grow the arena past a hole that fits."""
    events, pinned = random_events(7, 400)
    frees = [t for t, ev in enumerate(events) if ev[0] == "free" and ev[1] not in pinned]
    with pytest.raises(AssertionError, match="overlaps"):
        for cut in frees:                                   # (one early free is only seen where something takes the bytes)
            born = next(i for i, ev in enumerate(events) if ev[0] == "alloc" and ev[1] == events[cut][1])
            early = events[:born + 1] + [events[cut]] + events[born + 1:cut] + events[cut + 1:]
            check_placement(events, pinned, *_place(early, pinned))
    with pytest.raises(AssertionError, match="although|guarantees"):
        for cut in frees:
            check_placement(events, pinned, *_place(events[:cut] + events[cut + 1:], pinned))
