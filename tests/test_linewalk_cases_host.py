"""tests/linewalk_cases.py on its own: the Python reference of the line walk's tables (line_tables) on inputs small enough
to write the answer down by hand, and the case list - that it reaches the fourteen instantiations launch_lines_t
(csrc/welldup_lines.hip) can launch and every regime the tests of the emulator and of the GPU rely on.  No GPU."""
import numpy as np

import linewalk_cases as lc

OWNER = 1 << 31


def _csr(lists, levels=1):
    centre = np.array([c for c, _ in lists], dtype=np.int32)
    sizes = [len(w) for _, w in lists]
    start = np.concatenate([[0], np.cumsum(sizes)])
    off = np.array([[int(start[t] + c) for c in lc.cuts_of(sizes[t], levels)] for t in range(len(lists))], dtype=np.int32)
    return centre, off, np.array([w for _, ws in lists for w in ws], dtype=np.int32)


def test_tables_of_two_targets_by_hand():
    # target 0 (centre 9): wells 5, 3, 7;  target 1 (centre 8): wells 3, 6.  By well: 3 (t0 s1), 3 (t1 s0), 5 (t0 s0), 6 (t1 s1), 7 (t0 s2)
    centre, off, nbr = _csr([(9, [5, 3, 7]), (8, [3, 6])])
    tb = lc.line_tables(centre, off, nbr, 2)
    assert tb["pw"].tolist() == [3, 3, 5, 6, 7]
    # blocks of two pairs: {t0 s1, t1 s0}, {t0 s0, t1 s1}, {t0 s2}; a target's number within its block is the order it is met in
    assert tb["blk"].tolist() == [[0, 2, 0, 2], [2, 2, 2, 2], [4, 1, 4, 1]]
    assert tb["pm"].tolist() == [(0 << 16) | 1, (1 << 16) | 0, (0 << 16) | 0, (1 << 16) | 1, (0 << 16) | 2]
    assert tb["btgt"].tolist() == [0 | OWNER, 1 | OWNER, 0, 1, 0]  # the first block to hold a pair of a target owns it
    assert tb["bcen"].tolist() == [9, 8, 9, 8, 9]
    assert tb["boff"].tolist() == [[0, 3], [3, 5], [0, 3], [3, 5], [0, 3]]
    assert tb["tmax"] == 4
    # one block: the targets in the order of their first pair by well
    tb = lc.line_tables(centre, off, nbr, 0)
    assert tb["blk"].tolist() == [[0, 5, 0, 2]] and tb["btgt"].tolist() == [0 | OWNER, 1 | OWNER]
    assert tb["pm"].tolist() == [1, 1 << 16, 0, (1 << 16) | 1, 2]


def test_equal_wells_stay_in_target_then_slot_order():
    # well 4 three times: target 0 slot 2, target 1 slot 0, target 2 slot 1 - and target 2 comes first in nothing
    centre, off, nbr = _csr([(20, [9, 8, 4]), (21, [4, 1]), (22, [7, 4])])
    tb = lc.line_tables(centre, off, nbr, 100)
    assert tb["pw"].tolist() == [1, 4, 4, 4, 7, 8, 9]
    assert tb["btgt"].tolist() == [1 | OWNER, 0 | OWNER, 2 | OWNER]
    assert tb["pm"].tolist() == [(0 << 16) | 1, (1 << 16) | 2, (0 << 16) | 0, (2 << 16) | 1, (2 << 16) | 0, (1 << 16) | 1, (1 << 16) | 0]


def test_the_cut_at_256_targets_comes_before_the_pair_limit():
    # 300 targets of one slot, wells descending with the target: block 0 holds targets 299 .. 44 (256 of them), block 1 the rest
    centre, off, nbr = _csr([(1000 + t, [500 - t]) for t in range(300)])
    tb = lc.line_tables(centre, off, nbr, 5000)
    assert tb["blk"].tolist() == [[0, 256, 0, 256], [256, 44, 256, 44]] and tb["tmax"] == 256
    assert (tb["btgt"] == (np.arange(299, -1, -1) | OWNER)).all()
    assert (tb["pm"] == np.concatenate([np.arange(256), np.arange(44)]) << 16).all()
    # a 257th target's pair ends the block even where the block's own targets have pairs behind it
    centre, off, nbr = _csr([(1000 + t, [t]) for t in range(256)] + [(2000, [300]), (2001, [400, 301])])
    tb = lc.line_tables(centre, off, nbr, 5000)
    assert tb["blk"].tolist() == [[0, 256, 0, 256], [256, 3, 256, 2]]
    assert tb["btgt"][256:].tolist() == [256 | OWNER, 257 | OWNER]


def test_where_the_walk_does_not_apply():
    centre, off, nbr = _csr([(5000, list(range(4096)))])
    assert lc.line_tables(centre, off, nbr, 0) is None             # 4096 slots: one more than the tag's 12 bits
    centre, off, nbr = _csr([(5000, list(range(4095)))])
    tb = lc.line_tables(centre, off, nbr, 0)
    assert tb["blk"].tolist() == [[0, 4095, 0, 1]] and int(tb["pm"].max()) == 4094
    centre = np.array([3, 4], dtype=np.int32)
    off = np.array([[0, 2, 2], [2, 3, 4]], dtype=np.int32)        # an empty ring
    assert lc.line_tables(centre, off, np.array([1, 2, 5, 6], dtype=np.int32), 0) is None


def test_the_case_list_reaches_every_instantiation_and_every_regime():
    cases = lc.cases()
    want = {"k_scan_lines<%s, %d, 0>" % (s, b) for s in ("false", "true") for b in (2, 3, 5, 6, 8)} | \
        {"k_scan_lines<true, 4, 0, 4>", "k_scan_lines<false, 5, -1>", "k_scan_lines<true, 5, -1>", "k_scan_lines<true, 8, -1, 4>"}
    assert {c.kernel for c in cases if c.kernel} == want and len(want) == 14
    for fam in lc.FAMILIES:
        for layout in lc.LAYOUTS:
            mine = [c for c in cases if c.fam == fam and c.layout == layout]
            tags = set().union(*(c.tags for c in mine))
            missing = set(lc.TAGS) - tags
            # 254 mismatches are the Hamming family's; a target of 4096 slots in the interleaved layout is an error, not a case
            assert missing <= ({"k254"} if fam == "lev2" else set()) | ({"notapply"} if layout == "il" else set()), (fam, layout, missing)
    for c in cases:
        assert 257 <= c.n <= 4099 and c.levels <= 8 and c.line_pairs >= 1
        if "notapply" in c.tags:
            assert c.tables is None and c.blocks == 0 and c.kernel is None
            continue
        tb = c.tables
        assert c.blocks >= 1 and (np.diff(tb["pw"]) >= 0).all() and tb["tmax"] % 4 == 0
        assert (tb["blk"][:, 1] <= c.line_pairs).all() and (tb["blk"][:, 3] <= lc.K_LW_TARGETS).all()
        if "split" in c.tags:
            assert c.split_targets() > 0, c.name
        if "lastword" in c.tags:                                   # t = T - 1 alone in the last word of the mask's stride
            assert c.T % 4 == 1 and ((c.T + 3) // 4) % 32 == 0, c.name
        if "bufend" in c.tags:                                     # a last block of one pair: pw's last entry
            assert tb["blk"][-1].tolist()[:2] == [tb["pw"].shape[0] - 1, 1] and c.line_pairs in (127, 129, 511, 513), c.name
        if "cut256" in c.tags:                                     # a block full of targets, and local target 255 has a duplicate
            assert tb["blk"][0, 3] == 256 and tb["blk"][0, 1] < c.line_pairs and int(tb["pm"].max() >> 16) == 255, c.name
            t255 = int(tb["btgt"][255] & 0x7FFFFFFF)
            assert (lc.truth(c)["hits"][:, 1] == t255).any() and c.L > c.B1, c.name
        if "slot4095" in c.tags:
            hits = lc.truth(c)["hits"]
            assert c.lvl_off[0, -1] - c.lvl_off[0, 0] == 4095 and {0, 4093, 4094} <= set(hits[:, 2].tolist()) and c.L > c.B1, c.name
        if "hitcap" in c.tags and c.name.endswith("K100"):
            assert 0 < c.hit_cap < lc.truth(c)["hits"].shape[0], c.name
        if "k254" in c.tags:
            assert c.kk == 254 and c.L == 300 and 254 in lc.truth(c)["hits"][:, 3], c.name
        if "ties" in c.tags:
            assert not c.per_target and c.hit_cap < 0 and np.bincount(c.nbr).max() >= 5 and np.isin(c.centre, c.nbr).any(), c.name
    grids = {c.blocks * len(c.tiles) for c in cases if "grid" in c.tags}
    assert {1, 7, 9, 17} <= grids, grids
