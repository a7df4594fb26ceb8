"""Host reference of the molecules of a lane as arrays and of the keep by molecule
(include/welldup_lanemolecules.h) in numpy and plain Python: the families read off the labels (laneconsensus_ref.
families_of), a gathered family's molecules by laneumi_ref.molecules_of - a union by brute force over all pairs -, mol
and molmem written down from them as the header's table says, and the keep by molecule lanekeep_ref.lane_keep called
with mol in the place of the labels (it never looks at a members array).  The labels come from lanedups_ref.lane_dups
or lanenear_ref.lane_near_dups - the device's own labels are never used.
Test plumbing only: what LaneDups.umi(molecules=True) and LaneDups.keep(by_molecule=True) compute on the GPU is
compared against this."""
from __future__ import annotations

import numpy as np

import lanekeep_ref
import laneumi_ref
from laneconsensus_ref import families_of
from tiledups_ref import INVALID


def lane_molecules(umi_tiles, n, max_tiles, labels, max_e, max_family):
    """umi_tiles: [(tile_index, [U planes of n bytes])], labels uint32 [max_tiles, n] -> (mol, molmem), uint32
    [max_tiles, n] each."""
    assert 0 <= max_e <= laneumi_ref.MAX_E and 2 <= max_family <= laneumi_ref.MAX_FAMILY
    codes, _ = laneumi_ref.umi_codes(umi_tiles, n, max_tiles)
    flat = np.asarray(labels, dtype=np.uint32).reshape(-1)
    assert flat.size == max_tiles * n
    ids = np.arange(flat.size, dtype=np.uint32)
    mol = np.where(flat == INVALID, np.uint32(INVALID), ids).astype(np.uint32)      # not PF, or a Single until a family says otherwise
    molmem = np.zeros(flat.size, dtype=np.uint32)
    for root, m in families_of(labels):
        if m.size > max_family:                                        # Large: one molecule, as the finish left it
            mol[m] = root
            molmem[root] = m.size - 1
            continue
        for positions in laneumi_ref.molecules_of(codes[m], max_e):
            wells = m[positions]                                       # (positions ascend with the ids: wells[0] is the first well)
            mol[wells] = wells[0]
            molmem[wells[0]] = len(wells) - 1
    return mol.reshape(max_tiles, n), molmem.reshape(max_tiles, n)


def lane_keep_molecules(tiles, n, max_tiles, mol, edges, min_q):
    """lanekeep_ref.lane_keep with the molecules for the families -> (lane row, tile rows, masks, the summed scores of
    the molecules of one well)."""
    return lanekeep_ref.lane_keep(tiles, n, max_tiles, mol, edges, min_q)


def check_molecule_arrays(mol, molmem, labels):
    """What the header says of any (mol, molmem): the form the finish leaves label and members in, inside the families."""
    mol, molmem = (np.asarray(v, dtype=np.uint32).reshape(-1) for v in (mol, molmem))
    flat = np.asarray(labels, dtype=np.uint32).reshape(-1)
    assert ((mol == INVALID) == (flat == INVALID)).all()
    pf = np.flatnonzero(flat != INVALID)
    first = mol[pf].astype(np.int64)
    assert (first <= pf).all() and (mol[first] == first).all()         # a first well is the smallest id, and its own first
    assert (flat[first] == flat[pf]).all()                             # a molecule lies inside one family
    size = np.bincount(first, minlength=flat.size)
    assert (molmem[first] == size[first] - 1).all()
    assert (molmem[pf[first != pf]] == 0).all() and (molmem[flat == INVALID] == 0).all()


def check_molecule_identities(umi_lane, keep_lane, finish_lane, family_keep_lane=None, masks=None, family_masks=None):
    """Identities 1 - 4 and 7 of the header.  umi_lane: U; keep_lane: K; finish_lane: F (PF, Classes, InLane and
    Redundant are columns 0 .. 3: the Singles are PF - InLane); family_keep_lane, family_masks: wd_lane_keep's on the
    same lane.  The subset of identity 7 is asserted with ties too: a family's kept well has the largest score of the
    family and the smallest id among equals, so it has both within its molecule, a subset of the family - whatever a
    family keeps, its molecule keeps, and what the molecules drop the families drop."""
    U, K, F = (np.asarray(v) for v in (umi_lane, keep_lane, finish_lane))
    L = laneumi_ref
    singles = int(F[0] - F[1] - F[3])
    assert K[0] == K[1] + K[2] == F[0]                                                      # 1
    assert K[2] == U[L.REDUNDANT] + U[L.LARGE_WELLS] - U[L.LARGE]                          # 2
    assert K[6] == U[L.MOLECULES] - U[L.SIZE] + U[L.LARGE]                                 # 3
    assert K[1] == singles + U[L.MOLECULES] + U[L.LARGE]                                   # 4
    if family_keep_lane is not None:                                                        # 7
        assert K[2] <= np.asarray(family_keep_lane)[2]
    if masks is not None or family_masks is not None:
        assert masks is not None and family_masks is not None and sorted(masks) == sorted(family_masks)
        for t, m in masks.items():
            assert m.shape == family_masks[t].shape and (m >= family_masks[t]).all()       # what the family keeps, the molecules keep
