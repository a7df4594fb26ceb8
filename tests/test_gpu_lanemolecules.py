"""The molecules of a lane as arrays and the best well of each of them on the GPU (LaneDups.umi(molecules=True),
umi_molecules, keep(by_molecule=True); include/welldup_lanemolecules.h) against the host reference of
tests/lanemolecules_ref.py on the labels of tests/lanedups_ref.py / lanenear_ref.py: the UMI rows cell for cell those of
LaneDups.umi, mol and molmem word for word, the keep rows and every mask byte, nothing approximate, and the identities
the header states.

Shapes: 3 tiles of 8193 and of 9000 wells - a run of kLaneRun and a well, a run and a bit - in a lane with room for
four, 30 scanned cycles, UMI reads of 8 and 11 cycles; families of 2, 3, 64, 65, 71, 200 and 257 wells planted across
the tiles and across a run's boundary, so that max_family 70 and 256 each leave a family of max_family + 1 wells
Large; E = 0, 1 and 3.  "E >= U" needs a UMI read of at most WD_LANEUMI_MAX_E = 3 cycles, which is what wd_lane_umi
takes for E: identity 6 is checked on a lane with a UMI read of 3 cycles at E = 3."""
import ctypes
import io
import os
import re
import shutil
from contextlib import redirect_stdout

import numpy as np
import pytest

from laneconsensus_ref import families_of
from lanedups_ref import lane_dups
from lanekeep_ref import check_keep_identities, lane_keep
from lanemolecules_ref import check_molecule_arrays, check_molecule_identities, lane_keep_molecules, lane_molecules
from lanenear_ref import lane_near_dups
from laneumi_ref import FAMILIES, LARGE, LARGE_WELLS, MOLECULES, REDUNDANT, SIZE, WELLS, check_umi_identities, lane_umi
from test_gpu_lanekeep import EDGES, RUN, _finish, _host_tiles, _other_base, _plant, _random_tiles, _requalify, _tables, _upload
from test_gpu_lanekeep import _same as _same_keep
from test_gpu_laneumi import _bytes, _chain, _umi_batch, _umi_tiles
from well_duplicates_amd import _lib
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import bcl, report, synth
from well_duplicates_amd.scanner import LaneDups, Scanner

pytestmark = pytest.mark.gpu

CYCLES = 30
INDEX = [2, 0, 3]                                                     # slot -> tile index; index 1 is never added
MAX_TILES = 4
SIZES = (2, 3, 64, 65, 71, 200, 257)
INVALID = 0xFFFFFFFF


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    yield s
    s.close()


def _planted_lane(n, k, u, seed):
    """-> reads, filts, umi bytes per slot, and the reference's (tiles, umi_tiles, finish lane row, finish tile rows,
    labels).  Random reads with qualities of their own; pairs and triples by test_gpu_lanekeep._plant (at K >= 1 with
    a mismatch); then the families of SIZES, equal reads (at K >= 1 a quarter of the members one cycle off) whose wells
    lie anywhere on the three tiles - the family of 64 also on both sides of a run's boundary and on a tile's last
    well.  The UMIs by family: the families of 65 and 200 are chains one cycle apart, wells permuted along the chain;
    a pair is equal, one apart or unrelated; the others hold a few UMIs and their one-cycle errors, N among them."""
    rng = np.random.default_rng(seed)
    reads, filts = _random_tiles(rng, 3, n, CYCLES)
    for src, dst, count in ((0, 1, 150), (1, 2, 150), (0, 0, 80), (2, 0, 100), (1, 1, 60)):
        _plant(reads, rng, src, dst, count, k)
    free = rng.permutation(3 * n).tolist()
    edge = sorted({0 * n + RUN - 1, 0 * n + RUN, 1 * n + RUN - 1, 1 * n + n - 1, 2 * n + n - 1, 2 * n + RUN})      # (slot * n + well)
    taken = set(edge)
    for size in SIZES:
        wells = list(edge) if size == 64 else []
        while len(wells) < size:
            g = free.pop()
            if g not in taken:
                taken.add(g)
                wells.append(g)
        read = rng.integers(4, 256, CYCLES).astype(np.uint8)
        for i, g in enumerate(wells):
            copy = _requalify(read, rng.integers(0, 64, CYCLES).astype(np.uint8) << 2)
            if k and i % 4 == 1:
                c = int(rng.integers(0, CYCLES))
                copy[c] = _other_base(copy[c])
            reads[g // n][g % n] = copy
            filts[g // n][g % n] = 1
    tiles = _host_tiles(reads, filts, INDEX)
    fin_lane, fin_tiles, labels = lane_dups(tiles, n, MAX_TILES) if k == 0 else lane_near_dups(tiles, n, MAX_TILES, k)
    fams = families_of(labels)
    got_sizes = sorted(m.size for _, m in fams)
    assert got_sizes[-5:] == list(SIZES[2:]) and set(got_sizes[:-5]) <= {2, 3, 4} and got_sizes.count(2) > 300, got_sizes[-8:]
    assert sum(1 for _, m in fams if len(set((m // n).tolist())) > 1) > 200       # families across tiles
    flat = labels.reshape(-1)
    boundary = [INDEX[g // n] * n + g % n for g in edge]
    assert len({int(flat[g]) for g in boundary}) == 1 and flat[boundary[0]] != INVALID      # one family over the run's boundary
    codes = np.where(rng.random((flat.size, u)) < 0.025, 4, rng.integers(0, 4, (flat.size, u))).astype(np.uint8)
    for root, m in fams:
        if m.size in (65, 200):
            codes[rng.permutation(m)] = _chain(rng, u, m.size)
        elif m.size == 2:
            p = rng.random()
            if p < 0.7:
                codes[m[1]] = codes[m[0]]
            if 0.4 <= p < 0.7:
                c = int(rng.integers(0, u))
                codes[m[1], c] = (codes[m[1], c] + 1 + int(rng.integers(0, 3))) % 4
        else:
            centres = rng.integers(0, 4, (8 if m.size > 200 else 3, u)).astype(np.uint8)
            us = centres[rng.integers(0, len(centres), m.size)]
            for j in np.flatnonzero(rng.random(m.size) < 0.3).tolist():
                us[j, rng.integers(0, u)] = rng.integers(0, 5)
            codes[m] = us
    umi_bytes = [_bytes(rng, codes[ti * n:(ti + 1) * n]) for ti in INDEX]
    return reads, filts, umi_bytes, (tiles, _umi_tiles(umi_bytes, INDEX), fin_lane, fin_tiles, labels)


def _lane(sc, tb, utb, calls, hash_bits=0):
    """an accumulator with a quality part and a UMI part, fed call by call"""
    ld = LaneDups(sc, tb.N, MAX_TILES, tb.L, hash_bits=hash_bits)
    try:
        ld.qual_begin(EDGES)
        ld.umi_begin(utb.L)
        for slots in calls:
            idx = [INDEX[s] for s in slots]
            ld.umi_add(_tables(utb, slots), idx)
            ld.add_tables(idx, _tables(tb, slots))
            ld.qual_add(_tables(tb, slots), idx)
    except Exception:
        ld.close()
        raise
    return ld


def _same_rows(got, want, what=""):
    for g, w, name in zip(got, want, ("lane row", "tile rows")):
        assert g.shape == w.shape and (g == w).all(), (what, name, g[g != w], w[g != w], np.argwhere(g != w)[:8])


def _same_arrays(got, want, what=""):
    for g, w, name in zip(got, want, ("mol", "molmem")):
        assert g.dtype == np.uint32 and g.shape == w.shape and (g == w).all(), (what, name, np.argwhere(g != w)[:8], g[g != w][:8], w[g != w][:8])


# ---- 1: rows, arrays and masks against the reference --------------------------------------------------
@pytest.mark.parametrize("n,u,k", [(8193, 8, 0), (9000, 11, 1), (9000, 8, 0)])
def test_molecules_and_keep_match_reference_however_the_tiles_are_fed(sc, n, u, k):
    reads, filts, umi_bytes, (tiles, umi_tiles, fin_lane, fin_tiles, labels) = _planted_lane(n, k, u, 100 * k + u)
    combos = [(e, mf) for mf in (70, 256) for e in (0, 1, 3)]
    want_u = {c: lane_umi(tiles, umi_tiles, n, MAX_TILES, labels, *c) for c in combos}
    want_m = {c: lane_molecules(umi_tiles, n, MAX_TILES, labels, *c) for c in combos}
    want_k = {c: lane_keep_molecules(tiles, n, MAX_TILES, want_m[c][0], EDGES, 15) for c in combos}
    family = lane_keep(tiles, n, MAX_TILES, labels, EDGES, 15)
    for c in combos:
        check_molecule_arrays(*want_m[c], labels)
        check_umi_identities(*want_u[c], c[0], U=u, finish_lane=fin_lane)
        check_keep_identities(want_k[c][0], want_k[c][1], EDGES, 15, sum_singles=want_k[c][3])
        check_molecule_identities(want_u[c][0], want_k[c][0], fin_lane, family_keep_lane=family[0], masks=want_k[c][2],
                                  family_masks=family[2])
    # the ground: at max_family 70 the families of 71, 200 and 257 wells are Large, at 256 the last alone; pairs that
    # are one molecule and pairs that are two; molecules of 65 and more wells at E >= 1 (the chains); by molecule fewer
    # wells are dropped, many molecules' best is not their first well
    u70, u256 = want_u[(1, 70)][0], want_u[(1, 256)][0]
    print("K %d: U at E 1, max_family 256: %s; K: %s; by family: %s" % (k, u256.tolist(), want_k[(1, 256)][0].tolist(), family[0].tolist()))
    assert (u70[LARGE], u70[LARGE_WELLS], u256[LARGE], u256[LARGE_WELLS]) == (3, 71 + 200 + 257, 1, 257)
    assert u256[SIZE + 7] >= 2 and want_u[(0, 256)][0][SIZE + 7] == 0 and u256[SIZE + 1] > 100 and u256[SIZE] > 200
    assert want_u[(0, 256)][0][MOLECULES] > u256[MOLECULES] > want_u[(3, 256)][0][MOLECULES] > u256[FAMILIES]
    assert 0 < want_k[(1, 256)][0][2] < family[0][2] - 100 and want_k[(1, 256)][0][7] > 50
    assert (want_k[(0, 256)][0][2] < want_k[(1, 256)][0][2] < want_k[(3, 256)][0][2]) and want_k[(1, 70)][0][2] > want_k[(1, 256)][0][2]
    tb = _upload(sc, reads, filts)
    utb = _umi_batch(sc, umi_bytes, filts)
    try:
        for bits, calls in ((0, [[0, 1, 2]]), (2 if k else 1, [[2], [0, 1]])):
            ld = _lane(sc, tb, utb, calls, hash_bits=bits)
            try:
                rows = _finish(ld, k, bits)
                qhist = ld.qualities(0)[2]
                got_family = ld.keep(15, masks=True)
                _same_keep(got_family, family, "by family")
                for i, c in enumerate(combos):
                    if i % 2:                                          # whatever the region held before (identity 9)
                        sc.memset(ld.d_mol, 0x5A + i, ld.mol_bytes)
                    got_m = ld.umi(*c, molecules=True)
                    got_u = ld.umi(*c)
                    _same_rows(got_m, got_u, c)                        # cell for cell the rows of wd_lane_umi
                    _same_rows(got_m, want_u[c], c)
                    _same_arrays(ld.umi_molecules(), want_m[c], (bits, c))
                    assert ld.molecule_part() == c
                    got_k = ld.keep(15, masks=True, by_molecule=True)
                    _same_keep(got_k, want_k[c], (bits, c))
                    assert (got_k[1][1] == 0).all()                    # a tile index never added
                    check_keep_identities(got_k[0], got_k[1], EDGES, 15, finish_tiles=rows[1], qhist=qhist,
                                          sum_singles=want_k[c][3])
                    check_molecule_identities(got_m[0], got_k[0], rows[0], family_keep_lane=got_family[0], masks=got_k[2],
                                              family_masks=got_family[2])
                    _same_keep(ld.keep(15, by_molecule=True), want_k[c])         # twice, and without the masks
                # after other passes, and again after a call of the plain umi with another E: the part is the last
                # umi(molecules=True)'s
                last = combos[-1]
                ld.gc(0)
                ld.consensus(k, 256)
                ld.umi(0, 2)
                assert ld.molecule_part() == last
                _same_keep(ld.keep(15, masks=True), family)
                _same_keep(ld.keep(15, masks=True, by_molecule=True), want_k[last])
                _same_arrays(ld.umi_molecules(), want_m[last])
            finally:
                ld.close()
    finally:
        utb.free()
        tb.free()


# ---- 2: E >= U gives the families back (identity 6) ---------------------------------------------------
def test_at_e_not_below_u_the_keep_by_molecule_is_the_keep_by_family(sc):
    n, u, e = 8193, 3, 3
    reads, filts, umi_bytes, (tiles, umi_tiles, fin_lane, fin_tiles, labels) = _planted_lane(n, 0, u, 33)
    want_m = lane_molecules(umi_tiles, n, MAX_TILES, labels, e, 1024)
    family = lane_keep(tiles, n, MAX_TILES, labels, EDGES, 15)
    assert (want_m[0] == labels).all() and family[0][6] > 400 and family[0][7] > 100
    split = lane_molecules(umi_tiles, n, MAX_TILES, labels, 2, 1024)
    assert (split[0] != labels).sum() > 30                            # (one cycle less and the families split)
    tb = _upload(sc, reads, filts)
    utb = _umi_batch(sc, umi_bytes, filts)
    ld = _lane(sc, tb, utb, [[1], [2, 0]])
    try:
        rows = _finish(ld, 0)
        got_u = ld.umi(e, 1024, molecules=True)
        check_umi_identities(*got_u, e, U=u, finish_lane=rows[0])
        assert got_u[0][MOLECULES] == got_u[0][FAMILIES] and got_u[0][LARGE] == 0
        _same_arrays(ld.umi_molecules(), want_m)
        by_family, by_molecule = ld.keep(15, masks=True), ld.keep(15, masks=True, by_molecule=True)
        _same_keep(by_family, family)
        _same_keep(by_molecule, by_family)                             # the rows and every mask byte
        ld.umi(2, 1024, molecules=True)
        _same_arrays(ld.umi_molecules(), split)
        assert ld.keep(15, by_molecule=True)[0][2] < by_family[0][2]
    finally:
        ld.close()
        utb.free()
        tb.free()


# ---- 3: the lane rebuilt from the masks (identity 8) --------------------------------------------------
@pytest.mark.parametrize("k", [0, 1])
def test_the_lane_rebuilt_from_the_masks_has_no_redundant_molecule(sc, k):
    n, u, e = 8193, 8, 1
    reads, filts, umi_bytes, (tiles, umi_tiles, fin_lane, fin_tiles, labels) = _planted_lane(n, k, u, 7 + k)
    tb = _upload(sc, reads, filts)
    utb = _umi_batch(sc, umi_bytes, filts)
    ld = _lane(sc, tb, utb, [[0, 1, 2]])
    try:
        _finish(ld, k)
        before = ld.umi(e, 1024, molecules=True)[0]
        lane, trow, masks = ld.keep(15, masks=True, by_molecule=True)
        by_family = ld.keep(15)[0]
    finally:
        ld.close()
        tb.free()
    assert before[LARGE] == 0 and before[REDUNDANT] > 500 and lane[2] == before[REDUNDANT] < by_family[2] - 100
    kept = [filts[s] & masks[INDEX[s]] for s in range(3)]
    assert all(((filts[s] & 1) >= masks[INDEX[s]]).all() for s in range(3))               # only PF wells are kept
    tb = _upload(sc, reads, kept)
    ld = _lane(sc, tb, utb, [[2], [1], [0]])
    try:
        after = _finish(ld, k)[0]
        assert after[0] == lane[1] and after[3] == by_family[2] - lane[2]                 # what the UMI kept is redundant by the read alone
        got = ld.umi(e, 1024, molecules=True)[0]
        assert got[LARGE] == 0 and got[REDUNDANT] == 0 and got[MOLECULES] == got[WELLS] > 0
        again = ld.keep(15, masks=True, by_molecule=True)              # and keeping again keeps everything
        assert again[0][:4].tolist() == [lane[1], lane[1], 0, 0] and again[0][6] == 0
        assert all((again[2][INDEX[s]] == kept[s] & 1).all() for s in range(3))
    finally:
        ld.close()
        utb.free()
        tb.free()


# ---- 4: call discipline -------------------------------------------------------------------------------
def _raw_umi(sc, ld, e, mf, scratch, scratch_bytes, mol, mol_bytes, missing=None):
    out = [np.full(_lib.LANEUMI_LANE_COLS, -1, dtype=np.int64), np.full((ld.max_tiles, _lib.LANEUMI_TILE_COLS), -1, dtype=np.int64)]
    ptr = [None if i == missing else a.ctypes.data_as(ctypes.c_void_p) for i, a in enumerate(out)]
    rc = sc._lib.wd_lane_umi_molecules(ld._h, e, mf, ctypes.c_void_p(scratch), scratch_bytes, *ptr, ctypes.c_void_p(mol), mol_bytes)
    return (rc,) + tuple(out)


def _raw_keep(sc, ld, min_q, scratch, scratch_bytes, keep=None):
    out = [np.full(_lib.LANEKEEP_LANE_COLS, -1, dtype=np.int64), np.full((ld.max_tiles, _lib.LANEKEEP_TILE_COLS), -1, dtype=np.int64)]
    rc = sc._lib.wd_lane_keep_molecules(ld._h, min_q, ctypes.c_void_p(scratch), scratch_bytes,
                                        *[a.ctypes.data_as(ctypes.c_void_p) for a in out], keep)
    return (rc,) + tuple(out)


def _untouched(res):
    return all((a == -1).all() for a in res[1:])


def test_call_discipline(sc):
    n, u, k, e, mf = 8193, 8, 0, 1, 256
    reads, filts, umi_bytes, (tiles, umi_tiles, fin_lane, fin_tiles, labels) = _planted_lane(n, k, u, 55)
    want_u = lane_umi(tiles, umi_tiles, n, MAX_TILES, labels, e, mf)
    want_m = lane_molecules(umi_tiles, n, MAX_TILES, labels, e, mf)
    want_k = lane_keep_molecules(tiles, n, MAX_TILES, want_m[0], EDGES, 15)
    need_u, need_k = sc.lane_umi_scratch_bytes(MAX_TILES, n), sc.lane_keep_scratch_bytes(MAX_TILES, n)
    need_m = sc.lane_molecules_bytes(MAX_TILES, n)
    assert need_m == 2 * ((4 * MAX_TILES * n + 255) // 256 * 256)
    d_scratch = sc.malloc(max(need_u, need_k) + need_m)               # (a region inside the scratch: the overlap)
    d_mol = sc.malloc(need_m)
    sc.memset(d_scratch, 0xA5, max(need_u, need_k) + need_m)
    sc.memset(d_mol, 0x77, need_m)
    region = lambda: sc.d2h(d_mol, need_m, np.uint8)
    host = np.full(need_m, 0x33, dtype=np.uint8)
    tb = _upload(sc, reads, filts)
    utb = _umi_batch(sc, umi_bytes, filts)
    ld = _lane(sc, tb, utb, [[0, 1, 2]])
    try:
        res = _raw_umi(sc, ld, e, mf, d_scratch, need_u, d_mol, need_m)            # before any finish
        assert res[0] == _lib.ERR_ARG and _untouched(res) and b"finish" in sc._lib.wd_last_error(sc._ctx)
        with pytest.raises(ValueError):
            ld.keep(15, by_molecule=True)                              # no umi(molecules=True) yet
        with pytest.raises(ValueError):
            ld.umi_molecules()
        _finish(ld, k)
        assert ld.molecule_part() is None
        part = [ctypes.c_int(-7), ctypes.c_int(-7)]
        assert sc._lib.wd_lane_molecules_part(ld._h, *[ctypes.byref(v) for v in part]) == _lib.ERR_ARG
        assert b"no molecule part" in sc._lib.wd_last_error(sc._ctx) and [v.value for v in part] == [-7, -7]
        res = _raw_keep(sc, ld, 15, d_scratch, need_k)                 # no molecule part
        assert res[0] == _lib.ERR_ARG and _untouched(res) and b"wd_lane_umi_molecules" in sc._lib.wd_last_error(sc._ctx)
        ld.umi(e, mf)                                                  # the plain pass leaves none
        assert _raw_keep(sc, ld, 15, d_scratch, need_k)[0] == _lib.ERR_ARG
        # refused: what wd_lane_umi refuses, and a region that is null, short, in host memory or inside the scratch
        for bad in ((-1, mf, d_scratch, need_u, d_mol, need_m), (4, mf, d_scratch, need_u, d_mol, need_m),
                    (e, 1, d_scratch, need_u, d_mol, need_m), (e, 1025, d_scratch, need_u, d_mol, need_m),
                    (e, mf, 0, need_u, d_mol, need_m), (e, mf, d_scratch, need_u - 1, d_mol, need_m),
                    (e, mf, d_scratch, need_u, 0, need_m), (e, mf, d_scratch, need_u, d_mol, need_m - 1),
                    (e, mf, d_scratch, need_u, d_mol, 0), (e, mf, d_scratch, need_u, host.ctypes.data, need_m),
                    (e, mf, d_scratch, need_u + need_m, d_scratch + need_u, need_m),
                    (e, mf, d_scratch + 256, need_u, d_scratch, need_m)):
            res = _raw_umi(sc, ld, *bad)
            assert res[0] == _lib.ERR_ARG and _untouched(res), bad
        assert b"overlaps the scratch" in sc._lib.wd_last_error(sc._ctx)
        for missing in range(2):
            res = _raw_umi(sc, ld, e, mf, d_scratch, need_u, d_mol, need_m, missing=missing)
            assert res[0] == _lib.ERR_ARG and _untouched(res)
        assert (region() == 0x77).all() and (host == 0x33).all()       # nothing changed on error
        assert _raw_keep(sc, ld, 15, d_scratch, need_k)[0] == _lib.ERR_ARG
        first = _raw_umi(sc, ld, e, mf, d_scratch, need_u, d_mol, need_m)          # the caller's region, dirty
        assert first[0] == _lib.OK
        _same_rows(first[1:], want_u)
        at = (4 * MAX_TILES * n + 255) // 256 * 256
        got = [sc.d2h(d_mol + o, 4 * MAX_TILES * n, np.uint32).reshape(MAX_TILES, n) for o in (0, at)]
        _same_arrays(got, want_m)
        res = _raw_keep(sc, ld, 15, d_scratch, need_k)
        assert res[0] == _lib.OK
        _same_rows(res[1:], want_k[:2])
        for bad in ((-1, d_scratch, need_k), (64, d_scratch, need_k), (15, 0, need_k), (15, d_scratch, need_k - 256),
                    (15, d_mol, need_k)):                              # wd_lane_keep's refusals; a scratch over the region
            res = _raw_keep(sc, ld, *bad)
            assert res[0] == _lib.ERR_ARG and _untouched(res), bad
        _same_arrays([sc.d2h(d_mol + o, 4 * MAX_TILES * n, np.uint32).reshape(MAX_TILES, n) for o in (0, at)], want_m)
        assert ld.molecule_part() == (e, mf)
        assert sc._lib.wd_lane_molecules_part(ld._h, None, ctypes.byref(part[1])) == _lib.ERR_ARG and ld.molecule_part() == (e, mf)
        # a call that fails forgets the part: refused for its max_e, and for a null row before anything else is looked at
        assert _raw_umi(sc, ld, 4, mf, d_scratch, need_u, d_mol, need_m)[0] == _lib.ERR_ARG
        assert _raw_keep(sc, ld, 15, d_scratch, need_k)[0] == _lib.ERR_ARG and ld.molecule_part() is None
        for missing in range(2):
            assert _raw_umi(sc, ld, 0, 64, d_scratch, need_u, d_mol, need_m)[0] == _lib.OK and ld.molecule_part() == (0, 64)
            assert _raw_umi(sc, ld, e, mf, d_scratch, need_u, d_mol, need_m, missing=missing)[0] == _lib.ERR_ARG
            assert ld.molecule_part() is None and _raw_keep(sc, ld, 15, d_scratch, need_k)[0] == _lib.ERR_ARG
        assert _raw_umi(sc, ld, e, mf, d_scratch, need_u, d_mol, need_m)[0] == _lib.OK
        assert _raw_keep(sc, ld, 15, d_scratch, need_k)[0] == _lib.OK
        # a second finish is refused, and the part is stale from then on - also where the finish is refused for a null row
        rows = np.zeros(64, dtype=np.int64).ctypes.data_as(ctypes.c_void_p)
        assert sc._lib.wd_lane_dups_finish(ld._h, None, rows, None) == _lib.ERR_ARG and ld.molecule_part() is None
        assert _raw_umi(sc, ld, e, mf, d_scratch, need_u, d_mol, need_m)[0] == _lib.OK and ld.molecule_part() == (e, mf)
        assert sc._lib.wd_lane_near_dups_finish(ld._h, 1, None, 0, 0, rows, rows, None, None, rows, None) == _lib.ERR_ARG
        assert ld.molecule_part() is None
        assert _raw_umi(sc, ld, e, mf, d_scratch, need_u, d_mol, need_m)[0] == _lib.OK
        with pytest.raises(ValueError):
            ld.finish()
        assert ld.molecule_part() is None
        res = _raw_keep(sc, ld, 15, d_scratch, need_k)
        assert res[0] == _lib.ERR_ARG and _untouched(res) and b"wd_lane_umi_molecules" in sc._lib.wd_last_error(sc._ctx)
        _same_rows(ld.umi(e, mf, molecules=True), want_u)              # the accumulator's own region, and the part again
        _same_keep(ld.keep(15, masks=True, by_molecule=True), want_k)
        with pytest.raises(ValueError):                                # the near finish, refused as a second one
            ld.finish(hamming=1)
        with pytest.raises(ValueError):
            ld.keep(15, by_molecule=True)
        # another lane in the same workspaces: the region is kept, the part is not
        ld.restart()
        for slots in ([1], [0, 2]):
            idx = [INDEX[s] for s in slots]
            ld.add_tables(idx, _tables(tb, slots))
            ld.qual_add(_tables(tb, slots), idx)
            ld.umi_add(_tables(utb, slots), idx)
        _finish(ld, k)
        with pytest.raises(ValueError):
            ld.keep(15, by_molecule=True)
        _same_rows(ld.umi(e, mf, molecules=True), want_u)
        _same_keep(ld.keep(15, masks=True, by_molecule=True), want_k)
        ld.close()
        with pytest.raises(ValueError):
            ld.umi(e, mf, molecules=True)
        with pytest.raises(ValueError):
            ld.keep(15, by_molecule=True)
    finally:
        ld.close()
        utb.free()
        tb.free()
        sc.free(d_scratch)
        sc.free(d_mol)


def test_a_lane_without_tiles_or_wells(sc):
    ld = LaneDups(sc, 701, 3, 37)
    try:
        ld.qual_begin(EDGES)
        ld.umi_begin(8)
        ld.finish()
        lane, trow = ld.umi(1, 256, molecules=True)
        assert not lane.any() and not trow.any()
        mol, molmem = ld.umi_molecules()
        assert mol.shape == (3, 701) and (mol == INVALID).all() and not molmem.any()
        lane, trow, masks = ld.keep(15, masks=True, by_molecule=True)
        assert not lane.any() and not trow.any() and masks == {}
    finally:
        ld.close()
    ld = LaneDups(sc, 0, 3, 37)
    try:
        ld.qual_begin(EDGES)
        ld.umi_begin(8)
        ld.finish()
        lane, trow = ld.umi(0, 2, molecules=True)
        assert not lane.any() and not trow.any() and ld.umi_molecules()[0].shape == (3, 0)
        lane, trow = ld.keep(0, by_molecule=True)
        assert not lane.any() and not trow.any()
    finally:
        ld.close()


# ---- 5: the CLI ---------------------------------------------------------------------------------------
def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def test_cli_keep_umi_block_and_filter_files(tmp_path):
    """The run directory of test_gpu_laneumi.py's CLI test, one lane: tile 1103's files are tile 1101's but for the last
    cycle, which is tile 1102's.  Cycles 0-15 are scanned, 15-24 are the UMI: every well of 1103 is a copy of its well
    on 1101 whose UMI differs at the last cycle or not at all.  At E = 0 the copies whose UMI differs are molecules of
    their own: with --lane-dups-keep-umi the filter files clear fewer PF bits than without, and exactly the
    reference's; the UMI block and everything above it are byte for byte what they are without the flag."""
    rows, cols, levels, L, scan, lane = 36, 70, 3, 24, 15, 1
    n = rows * cols
    x, y = synth.honeycomb_pixels(rows, cols)
    spec = synth.SynthSpec(seed=35, n_clusters=n, row=cols, plant_per_64k=8000, nocall_per_64k=500, plant_far=True)
    run_dir = str(tmp_path / "run")
    names = ["1101", "1102", "1103", "1104"]
    synth.write_run_dir(spec, run_dir, [lane], names, list(range(L)), slocs=synth.slocs_bytes(x, y))
    source = lambda t, c: "1101" if t == "1103" and c < L - 1 else "1102" if t == "1103" else t
    ldir = os.path.join(run_dir, "Data", "Intensities", "BaseCalls", "L%03d" % lane)
    shutil.copy(os.path.join(ldir, "s_%d_1101.filter" % lane), os.path.join(ldir, "s_%d_1103.filter" % lane))
    for c in range(L):
        cdir = os.path.join(ldir, "C%d.1" % (c + 1))
        shutil.copy(os.path.join(cdir, "s_%d_%s.bcl.gz" % (lane, source("1103", c))),
                    os.path.join(cdir, "s_%d_1103.bcl.gz" % lane))
    planes = lambda t, cs: [synth.plane_bytes(spec, lane, int(source(t, c)), c) for c in cs]
    filters = [synth.filter_bytes(spec, lane, int(t if t != "1103" else "1101")) for t in names]
    tiles = [(i, planes(t, range(scan)), filters[i]) for i, t in enumerate(names)]
    umi_tiles = [(i, planes(t, range(scan, L))) for i, t in enumerate(names)]
    edges = cwd.DEFAULT_QUALITY_BINS
    labels = lane_dups(tiles, n, 4)[2]
    mol = lane_molecules(umi_tiles, n, 4, labels, 0, 256)[0]
    by_family, by_molecule = lane_keep(tiles, n, 4, labels, edges, 15), lane_keep_molecules(tiles, n, 4, mol, edges, 15)
    assert by_family[0][2] - by_molecule[0][2] > 500 and by_molecule[0][2] > 500
    text = io.StringIO()
    report.write_lane_keep(str(lane), report.LaneKeepCounts.from_rows(by_molecule[0], by_molecule[1], names, 0, 15, edges, scan,
                                                                      by="molecule"), verbose=True, out=text)
    want = text.getvalue()
    assert "\tMolecules: %d\t" % by_molecule[0][6] in want and want.rstrip("\n").split("\n")[-3].endswith("\tBy: molecule")
    argv = ["-s", "hiseq_x", "-r", run_dir, "-t", "1101,1102,1103,1104", "-i", str(lane), "-l", str(levels),
            "--cycles", "0-%d" % scan, "-q", "--all-wells", "--lane-dups", "--lane-dups-umi", "%d-%d" % (scan, L),
            "--lane-dups-umi-mismatches", "0", "--lane-dups-keep"]
    out = {flag: str(tmp_path / ("dedup_" + flag)) for flag in ("family", "molecule")}
    plain = _main(argv + ["--lane-dups-keep-out", out["family"]])
    run = _main(argv + ["--lane-dups-keep-out", out["molecule"], "--lane-dups-keep-umi", "--tile-batch", "3"])
    assert "By:" not in plain and "\tFamilies: %d\t" % by_family[0][6] in plain
    cut = lambda s: s[:s.index("\nLaneKeep: ")]
    assert cut(run) == cut(plain) and "LaneUmiSummary: 1" in cut(run)                  # the UMI block and everything above it
    assert run.endswith(want) and run == cut(run) + want
    cleared = {}
    for flag, ref in (("family", by_family), ("molecule", by_molecule)):
        written = sorted(os.listdir(os.path.join(out[flag], "L%03d" % lane)))
        assert written == ["s_%d_%s.filter" % (lane, t) for t in names]
        cleared[flag] = 0
        for i, t in enumerate(names):
            got = bcl.Tile(os.path.join(out[flag], "L%03d" % lane), t).read_filter()
            assert (got & 1 == ref[2][i]).all() and (got & 0xFE == filters[i] & 0xFE).all(), (flag, t)
            cleared[flag] += int(((filters[i] & 1) > (got & 1)).sum())
    assert cleared["molecule"] == by_molecule[0][2] < cleared["family"] == by_family[0][2]
    m = re.search(r"LaneKeepSummary: 1\t.*\tDropped: (\d+) ", run)
    assert m and int(m.group(1)) == cleared["molecule"]
