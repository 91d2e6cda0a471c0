"""tests/host_fed_ring.py's schedule() and RingOrder, no GPU: what the host-fed tests feed their rings and in which order the
batches come back."""
import numpy as np
import pytest

import host_fed_ring as HR

CASES = [(11, 3, 4, 0), (11, 3, 4, 1), (6, 2, 4, 50), (6, 2, 4, 51), (1, 3, 4, 2), (2, 3, 1, 3), (40, 4, 7, 4), (5, 1, 2, 5)]


@pytest.mark.parametrize("nbatches,depth,max_batch,seed", CASES)
def test_every_batch_completes_once_and_in_order(nbatches, depth, max_batch, seed):
    s = HR.schedule(nbatches, depth, max_batch, seed)
    assert s["completes"] == list(range(nbatches))
    assert [e[1] for e in s["events"] if e[0] == "queue"] == list(range(nbatches))
    assert [e[1] for e in s["events"] if e[0] == "complete"] == list(range(nbatches))
    assert all(slot == i % depth for _, i, slot in s["events"])


@pytest.mark.parametrize("nbatches,depth,max_batch,seed", CASES)
def test_no_slot_is_reused_before_it_completes(nbatches, depth, max_batch, seed):
    busy, most = {}, 0
    for what, i, slot in HR.schedule(nbatches, depth, max_batch, seed)["events"]:
        if what == "queue":
            assert slot not in busy, f"batch {i} queued on slot {slot} while batch {busy.get(slot)} is in flight"
            busy[slot] = i
        else:
            assert busy.pop(slot) == i
        most = max(most, len(busy))
    assert not busy
    assert most == min(depth, nbatches)   # the ring does fill: depth batches in flight at once


@pytest.mark.parametrize("nbatches,depth,max_batch,seed", CASES)
def test_contents_on_a_slot_alternate_and_counts_cover_the_range(nbatches, depth, max_batch, seed):
    batches = HR.schedule(nbatches, depth, max_batch, seed)["batches"]
    assert len(batches) == nbatches
    for i, (c, n) in enumerate(batches):
        assert 0 <= c < HR.NCONTENTS and 1 <= n <= max_batch
        if i >= depth and depth > 1:
            assert c != batches[i - depth][0], f"slot {i % depth} gets content {c} twice in a row (batches {i - depth}, {i})"
        if i >= 1:
            assert c != batches[i - 1][0]
    counts = [n for _, n in batches]
    if nbatches >= max_batch:
        assert set(counts) == set(range(1, max_batch + 1))
    if max_batch > 1:
        assert counts[-1] < max_batch, "the last batch is not ragged"
    assert batches == HR.schedule(nbatches, depth, max_batch, seed)["batches"]   # a pure function of its arguments


def test_two_contents_differ_in_every_frame():
    """Frame f of two different contents is of two different kinds, so a stale map is never the right one by chance."""
    w, h = 64, 48
    for ch in (1, 3):
        sets = [HR.content_frames(c, w, h, ch, 4) for c in range(HR.NCONTENTS)]
        assert sets[0].shape == ((4, h, w) if ch == 1 else (4, h, w, 3)) and sets[0].dtype == np.uint8
        for a in range(HR.NCONTENTS):
            for b in range(a + 1, HR.NCONTENTS):
                for f in range(4):
                    assert not np.array_equal(sets[a][f], sets[b][f])
                    assert HR.KINDS[(a + f) % 4] != HR.KINDS[(b + f) % 4]


def test_split_host_out_finds_maps_and_the_rest():
    w, h, n, row, fs = 5, 3, 2, 8, 30
    raw = np.full(4 * fs, HR.POISON, np.uint8)
    want = np.arange(n * h * w, dtype=np.uint8).reshape(n, h, w)
    for f in range(n):
        for y in range(h):
            raw[f * fs + y * row: f * fs + y * row + w] = want[f, y]
    maps, rest = HR.split_host_out(raw, n, w, h, row, fs)
    assert np.array_equal(maps, want) and rest.size == raw.size - want.size and (rest == HR.POISON).all()
    HR.check_batch(raw, want, w, h, row, fs, "clean")
    raw[fs - 1] = 0   # the gap behind frame 0
    with pytest.raises(AssertionError, match="outside"):
        HR.check_batch(raw, want, w, h, row, fs, "gap written")
    raw[fs - 1] = HR.POISON
    raw[row + 1] ^= 1
    with pytest.raises(AssertionError, match="map 0 row 1 column 1"):
        HR.check_batch(raw, want, w, h, row, fs, "wrong byte")
