"""Reads that put many concurrent unions on few roots, and many claims on few slots, in numpy: the kinds of
tools/emu_reads.h (which feeds the kernels' sources on the CPU under shuffled schedules: tests/test_near_emu.py,
tests/test_readclasses_emu.py) for the GPU (tests/test_gpu_contention.py).
  families   about 12 centres, every well 0 to 3 substituted cycles (N among the substitutes) from its centre:
             hundreds of equal reads per class and of near reads per cluster, all on a dozen roots
  chain      `length` reads, each one cycle from the last, at wells in random order or with ids strictly descending
             along the chain (every union hooks a fresh root under the next: the deepest forest there is); the other
             wells read something random
  probe edge index reads of a lane whose groups' representatives all begin their probes at one entry of k_li_tally's
             table in LDS (csrc/lane_index.inc): as many groups as a probe path is long, one more, a few more
An id space is a tile, or the tiles of a lane end to end (`split` cuts it into the lane's tiles).
Test plumbing only; tests/test_contention_inputs.py checks what is promised here."""
from __future__ import annotations

import numpy as np

CENTRES = 12
MAX_SUBS = 3
LI_SLOTS = 512                 # kLiSlots, kLiProbe (csrc/lane_index.inc) and kLaneRun (csrc/lane_pass.inc):
LI_PROBE = 8                   # tests/test_laneindex_emu.py holds them, and li_home below, against the sources
LANE_RUN = 8192


def _bytes_of(rng, codes):
    """codes uint8 [n, L] (0..3 a base, 4 N) -> plane bytes: 0 for N, else the base under quality bits that are not 0"""
    quality = rng.integers(1, 64, codes.shape).astype(np.uint8)
    return np.where(codes == 4, 0, (quality << 2) | (codes & 3)).astype(np.uint8)


def _random_codes(rng, n, L, n_rate=0.02):
    codes = rng.integers(0, 4, (n, L)).astype(np.uint8)
    codes[rng.random((n, L)) < n_rate] = 4
    return codes


def families(seed, n, L):
    """-> (reads uint8 [n, L] bytes, centre int64 [n]: the family of every well)"""
    rng = np.random.default_rng(seed)
    centres = _random_codes(rng, CENTRES, L, 0.05)
    which = rng.integers(0, CENTRES, n)
    codes = centres[which]
    subs = rng.integers(0, MAX_SUBS + 1, n)
    for s in range(MAX_SUBS):                                          # well w gets subs[w] substitutions
        hit = np.flatnonzero(subs > s)
        codes[hit, rng.integers(0, L, hit.size)] = rng.integers(0, 5, hit.size)
    return _bytes_of(rng, codes), which


def chain(seed, n, L, length=100, descending=False):
    """-> (reads uint8 [n, L] bytes, wells int64 [length]: the chain's wells in chain order).  Step i changes cycle
    i % L to another base, so consecutive reads differ in exactly one cycle."""
    rng = np.random.default_rng(seed)
    length = min(length, n)
    codes = _random_codes(rng, n, L)
    wells = rng.permutation(n)[:length]
    if descending:
        wells = np.sort(wells)[::-1]
    read = rng.integers(0, 4, L).astype(np.uint8)
    for i, w in enumerate(wells.tolist()):
        if i:
            read[i % L] = (read[i % L] + 1 + rng.integers(0, 3)) % 4
        codes[w] = read
    return _bytes_of(rng, codes), wells.astype(np.int64)


def filters(seed, n, keep=()):
    """filter bytes [n]: nine in ten pass, the wells of `keep` all do; bits above bit 0 are noise"""
    rng = np.random.default_rng(seed)
    filt = (rng.integers(0, 128, n) << 1).astype(np.uint8)
    filt |= (rng.random(n) < 0.9).astype(np.uint8)
    filt[np.asarray(keep, dtype=np.int64)] |= 1
    return filt


def split(reads, filt, n_tiles):
    """an id space of n_tiles * n wells -> (per tile reads [n, L], per tile filter [n])"""
    n = reads.shape[0] // n_tiles
    assert n * n_tiles == reads.shape[0]
    return [reads[t * n:(t + 1) * n] for t in range(n_tiles)], [filt[t * n:(t + 1) * n] for t in range(n_tiles)]


def line_rings(n, levels=2):
    """targets for a tile whose wells lie in a row: level l of well w holds w - l - 1 and w + l + 1 where they exist
    -> (centre int32 [n], lvl_off int32 [n, levels + 1], nbr int32 [P])"""
    lvl_off, nbr = [], []
    for w in range(n):
        row = [len(nbr)]
        for l in range(levels):
            nbr.extend(m for m in (w - l - 1, w + l + 1) if 0 <= m < n)
            row.append(len(nbr))
        lvl_off.append(row)
    return np.arange(n, dtype=np.int32), np.array(lvl_off, dtype=np.int32), np.array(nbr, dtype=np.int32)


def li_home(ids):
    """the entry of k_li_tally's table in LDS at which the probes of the group with representative `ids` begin: a copy
    of li_home() of csrc/lane_index.inc (tests/test_laneindex_emu.py compares it with what the kernel's own gives)"""
    ids = np.asarray(ids, dtype=np.uint64)
    return (((ids * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(23)).astype(np.int64) & (LI_SLOTS - 1)


def probe_edge_index(seed, n, I, groups, n_tiles=2):
    """Index reads of a lane of n_tiles tiles of n wells, tile indices 0 .. n_tiles - 1 all added, with exactly `groups`
    groups: their representatives - the smallest PF global id of each - lie in the first run of tile 0 and share
    li_home(); the wells below the first of them fail the filter, and every later well carries the key of a
    representative below it (on the other tiles: of any).  -> (index reads per tile uint8 [n, I] bytes, filters per
    tile uint8 [n], reps int64 [groups] ascending, the shared entry)"""
    rng = np.random.default_rng(seed)
    run = np.arange(min(n, LANE_RUN))
    home = li_home(run)
    best = None
    for h in range(LI_SLOTS):
        at = run[home == h]
        if at.size >= groups and (best is None or at[groups - 1] < best[groups - 1]):
            best = at
    assert best is not None, "no %d wells of a run share an entry" % groups
    reps = best[:groups].astype(np.int64)
    keys = np.zeros((0, I), dtype=np.uint8)
    while keys.shape[0] < groups:                                      # distinct reads, an N now and then
        keys = np.unique(np.concatenate([keys, _random_codes(rng, groups, I, 0.05)]), axis=0)
    keys = keys[rng.permutation(keys.shape[0])[:groups]]
    gid = np.arange(n_tiles * n)
    below = np.searchsorted(reps, gid, side="right")                   # the representatives at or below a well
    which = (rng.random(gid.size) * np.maximum(below, 1)).astype(np.int64)
    which[reps] = np.arange(groups)
    pf = (below > 0) & (rng.random(gid.size) < 0.9)
    pf[reps] = True
    filt = (rng.integers(0, 128, gid.size) << 1).astype(np.uint8) | pf.astype(np.uint8)
    idx = _bytes_of(rng, keys[which])
    tiles, filts = split(idx, filt, n_tiles)
    return tiles, filts, reps, int(li_home(reps[:1])[0])
