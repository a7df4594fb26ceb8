"""Tally reducer and report printer for the scan path.

Host-side mirror of `output_writer` (count_well_duplicates.py:27-153).  The device
returns, per tile, the integer block

    [valid, wells[0..n), dups[0..n), hit[0..n), first[0..n), last[0..n)]      (n = levels)

where for every valid target with per-level dup counts d[l] and hit mask m = {l : d[l] > 0}
    wells[l] += len(ring l)     dups[l] += d[l]     hit[l] += (l in m)
    first[min(m)] += 1          last[max(m)] += 1                (nothing if m is empty)
and the reference's accumulated columns are prefix / suffix sums of those histograms:
    AccO[l] = sum(first[0..l])  (count_well_duplicates.py:80-84, inside-out)
    AccI[l] = sum(last[l..n))   (count_well_duplicates.py:85-89, outside-in)
All of it is integer arithmetic; the only floating point is the printed ratios, which stay
on the host as Python floats evaluated in the reference's order (:115-123, :135-153).

Known divergence: with valid targets but zero duplicates in a lane the
reference dies with ZeroDivisionError at :115-117 after printing the per-tile lines.
This printer reports 0.00 % instead; pass strict=True to get the reference's exception.
"""
from __future__ import annotations

import math
import sys
from dataclasses import dataclass, field
from fractions import Fraction
from typing import Dict, List, Optional, Sequence

TALLY = 0    # count_well_duplicates.py:17
LENGTH = 1   # count_well_duplicates.py:18


@dataclass
class TileCounts:
    """Per-tile integer tallies for `levels` levels."""
    targets: int = 0
    wells: List[int] = field(default_factory=list)
    dups: List[int] = field(default_factory=list)
    hit: List[int] = field(default_factory=list)
    first: List[int] = field(default_factory=list)
    last: List[int] = field(default_factory=list)

    @property
    def levels(self) -> int:
        return len(self.wells)

    @classmethod
    def zeros(cls, levels: int) -> "TileCounts":
        z = lambda: [0] * levels
        return cls(0, z(), z(), z(), z(), z())

    @classmethod
    def from_block(cls, block: Sequence[int], levels: int) -> "TileCounts":
        """Decode one row of the device counter block (include/welldup.h, wd_count_tiles)."""
        b = [int(v) for v in block]
        assert len(b) == 1 + 5 * levels
        cut = lambda k: b[1 + k * levels: 1 + (k + 1) * levels]
        return cls(b[0], cut(0), cut(1), cut(2), cut(3), cut(4))

    @classmethod
    def from_target_stats(cls, tile_counts, levels: int) -> "TileCounts":
        """Reduce the reference's per-target list [[(tally, length)] * levels] * targets."""
        c = cls.zeros(levels)
        c.targets = len(tile_counts)
        for targ in tile_counts:
            mask = [bool(targ[lev][TALLY]) for lev in range(levels)]
            for lev in range(levels):
                c.wells[lev] += targ[lev][LENGTH]
                c.dups[lev] += targ[lev][TALLY]
                c.hit[lev] += mask[lev]
            if any(mask):
                c.first[mask.index(True)] += 1
                c.last[levels - 1 - mask[::-1].index(True)] += 1
        return c

    def acco(self) -> List[int]:
        out, run = [], 0
        for v in self.first:
            run += v
            out.append(run)
        return out

    def acci(self) -> List[int]:
        out, run = [], 0
        for v in reversed(self.last):
            run += v
            out.append(run)
        return out[::-1]


def write_report(lane, sample_size, tiles: Dict[str, TileCounts], levels: int = 0,
                 verbose: bool = False, out=None, strict: bool = False) -> None:
    """Print the per-tile (verbose) and per-lane report exactly as the reference does.

    tiles: {tile id string: TileCounts}; printed in sorted string order (:63).
    levels: 0 = infer from the first tile with a valid target (:41-47); if no tile has
            one, no per-level line is printed at all.
    """
    out = out or sys.stdout
    if not levels:
        for tc in tiles.values():
            if tc.targets > 0:
                levels = tc.levels
                break

    tot_targets = 0
    tot = TileCounts.zeros(levels)
    tot_acco = [0] * levels
    tot_acci = [0] * levels

    for tile in sorted(tiles.keys()):
        tc = tiles[tile]
        tot_targets += tc.targets
        if verbose:
            print("Lane: %s\tTile: %s\tTargets: %i/%i" % (lane, tile, tc.targets, sample_size),
                  file=out)
        if tc.levels != levels:
            # Only a tile with no valid target may lack level data.  Truncating a
            # histogram to fewer levels is not possible (AccI needs per-target data):
            # callers reduce with the wanted level count instead.
            if tc.targets != 0:
                raise ValueError("tile %s holds %d levels, report wants %d"
                                 % (tile, tc.levels, levels))
            tc = TileCounts.zeros(levels)
        acco, acci = tc.acco(), tc.acci()
        for lev in range(levels):
            if verbose:
                print("Level: %i\tWells: %i\tDups: %i\tHit: %i\tAccO: %i\tAccI: %i" % (
                    lev + 1, tc.wells[lev], tc.dups[lev], tc.hit[lev], acco[lev], acci[lev]),
                    file=out)
            tot.wells[lev] += tc.wells[lev]
            tot.dups[lev] += tc.dups[lev]
            tot.hit[lev] += tc.hit[lev]
            tot_acco[lev] += acco[lev]
            tot_acci[lev] += acci[lev]

    # "Picard-equivalent" percentages, operation order as :111-125
    if tot_acci:
        grand_tot_hits = tot_acci[0]
        grand_tot_dups = sum(tot.dups)
        if strict or (grand_tot_dups + grand_tot_hits) != 0:
            peds = (grand_tot_hits *
                    (1 - grand_tot_hits / (grand_tot_dups + grand_tot_hits)) /
                    tot_targets)
            peds2 = (grand_tot_hits *
                     (1 - grand_tot_hits / (2 * grand_tot_dups)) /
                     tot_targets)
        else:
            peds = peds2 = 0          # reference: ZeroDivisionError
    else:
        grand_tot_hits = peds = peds2 = 0

    print("LaneSummary: %s\tTiles: %i\tTargets: %i/%i" % (
        lane, len(tiles), tot_targets, sample_size * len(tiles)), file=out)

    for lev in range(levels):
        if strict or tot_targets:
            r_dups = tot.dups[lev] / tot.wells[lev]
            r_hit = tot.hit[lev] / tot_targets
            r_acco = tot_acco[lev] / tot_targets
            r_acci = tot_acci[lev] / tot_targets
        else:
            r_dups = r_hit = r_acco = r_acci = 0.0
        print("Level: %i\tWells: %i\tDups: %i (%.5f)\t" % (
            lev + 1, tot.wells[lev], tot.dups[lev], r_dups) +
            "Hit: %i (%.5f)\tAccO: %i (%.5f)\tAccI: %i (%.5f)" % (
                tot.hit[lev], r_hit, tot_acco[lev], r_acco, tot_acci[lev], r_acci),
            file=out)

    raw_dup_rate = grand_tot_hits / tot_targets if grand_tot_hits else 0.0

    print(file=out)
    print("Overall duplication (Acc/Targets): {:.2%}".format(raw_dup_rate), file=out)
    print("Picard-equivalent duplication v1:  {:.2%}".format(peds), file=out)
    print("Picard-equivalent duplication v2:  {:.2%}".format(peds2), file=out)


def output_writer(lane, sample_size, lane_dupl, levels=0, verbose=False, out=None,
                  strict=False):
    """Reference signature (count_well_duplicates.py:27): report from per-target stats.

    lane_dupl: {tile: [[(tally, length)] * levels] * valid_targets}.  With `levels` given,
    only the first `levels` entries of each target are reduced, as the reference does.
    """
    if not levels:
        for atile in lane_dupl.values():
            if len(atile) > 0:
                levels = len(atile[0])
                break
    tiles = {tile: TileCounts.from_target_stats(tc, levels) for tile, tc in lane_dupl.items()}
    write_report(lane, sample_size, tiles, levels=levels, verbose=verbose, out=out,
                 strict=strict)


SIZE_BIN_NAMES = ("2", "3", "4", "5", "6", "7", "8", "9+")


@dataclass
class DupSetCounts:
    """Duplicate sets of one tile, or of several added up (include/welldup_sets.h, wd_dup_sets):
    PF wells, and per level (cumulative: the graph of the edges of level <= l) the sets of >= 2 wells,
    the wells in them and the redundant wells (InSets - Sets); size bins of the outermost level's sets."""
    pf: int = 0
    sets: List[int] = field(default_factory=list)
    in_sets: List[int] = field(default_factory=list)
    redundant: List[int] = field(default_factory=list)
    sizes: List[int] = field(default_factory=lambda: [0] * len(SIZE_BIN_NAMES))

    @property
    def levels(self) -> int:
        return len(self.sets)

    @classmethod
    def zeros(cls, levels: int) -> "DupSetCounts":
        return cls(0, [0] * levels, [0] * levels, [0] * levels, [0] * len(SIZE_BIN_NAMES))

    @classmethod
    def from_block(cls, block: Sequence[int], levels: int) -> "DupSetCounts":
        """Decode one out_sets row: [PF, Sets[levels], InSets[levels], Redundant[levels], size bins]."""
        b = [int(v) for v in block]
        assert len(b) == 1 + 3 * levels + len(SIZE_BIN_NAMES)
        cut = lambda k: b[1 + k * levels: 1 + (k + 1) * levels]
        return cls(b[0], cut(0), cut(1), cut(2), b[1 + 3 * levels:])

    def __add__(self, other: "DupSetCounts") -> "DupSetCounts":
        if self.levels != other.levels:
            raise ValueError("duplicate sets of %d and %d levels" % (self.levels, other.levels))
        add = lambda a, b: [x + y for x, y in zip(a, b)]
        return DupSetCounts(self.pf + other.pf, add(self.sets, other.sets), add(self.in_sets, other.in_sets),
                            add(self.redundant, other.redundant), add(self.sizes, other.sizes))

    def exact_duplication(self) -> float:
        """Redundant wells of the outermost level / PF wells (0 without PF wells)."""
        return self.redundant[-1] / self.pf if self.pf and self.levels else 0.0


def write_dup_sets(lane, counts: Dict[str, DupSetCounts], verbose: bool = False, out=None, levels: int = 0) -> None:
    """The duplicate-set block that follows a lane's report under --dup-sets: per-tile lines (verbose, in
    sorted tile order as write_report), the lane's sums, the set sizes and the exact duplication."""
    out = out or sys.stdout
    if not levels:
        levels = next((c.levels for c in counts.values()), 0)
    tot = DupSetCounts.zeros(levels)
    print(file=out)
    for tile in sorted(counts.keys()):
        dc = counts[tile]
        tot = tot + dc
        if verbose:
            print("DupSets: %s\tTile: %s\tPF wells: %i" % (lane, tile, dc.pf), file=out)
            for lev in range(levels):
                print("Level: %i\tSets: %i\tInSets: %i\tRedundant: %i" % (
                    lev + 1, dc.sets[lev], dc.in_sets[lev], dc.redundant[lev]), file=out)
    print("DupSetsSummary: %s\tTiles: %i\tPF wells: %i" % (lane, len(counts), tot.pf), file=out)
    for lev in range(levels):
        r_in = tot.in_sets[lev] / tot.pf if tot.pf else 0.0
        r_red = tot.redundant[lev] / tot.pf if tot.pf else 0.0
        print("Level: %i\tSets: %i\tInSets: %i (%.5f)\tRedundant: %i (%.5f)" % (
            lev + 1, tot.sets[lev], tot.in_sets[lev], r_in, tot.redundant[lev], r_red), file=out)
    print("SetSizes (level %i): %s" % (levels, "\t".join(
        "%s: %i" % (name, n) for name, n in zip(SIZE_BIN_NAMES, tot.sizes))), file=out)
    print("Exact duplication (Redundant/PF wells): {:.2%}".format(tot.exact_duplication()), file=out)


CLASS_BIN_NAMES = ("2", "3", "4", "5", "6", "7", "8", ">=9")


@dataclass
class TileDupCounts:
    """Read classes of one tile, or of several added up (include/welldup_tiledups.h, wd_tile_dups): PF wells,
    the classes of >= 2 PF wells with equal reads, the wells in them, the redundant wells (InClasses - Classes);
    per level (cumulative) the wells in classes with a classmate in their rings and the sizes of those wells'
    rings; size bins of the classes.  even_den = InClasses * (wells of the tile - 1): what RingWells is divided
    by for the share a classmate placed anywhere on the tile would have in the rings (0 = tile size not given)."""
    pf: int = 0
    classes: int = 0
    in_classes: int = 0
    redundant: int = 0
    local: List[int] = field(default_factory=list)
    ring_wells: List[int] = field(default_factory=list)
    sizes: List[int] = field(default_factory=lambda: [0] * len(CLASS_BIN_NAMES))
    even_den: int = 0

    @property
    def levels(self) -> int:
        return len(self.local)

    @classmethod
    def zeros(cls, levels: int) -> "TileDupCounts":
        return cls(0, 0, 0, 0, [0] * levels, [0] * levels, [0] * len(CLASS_BIN_NAMES), 0)

    @classmethod
    def from_block(cls, block: Sequence[int], levels: int, wells: int = 0) -> "TileDupCounts":
        """Decode one out_rows row: [PF, Classes, InClasses, Redundant, Local[levels], RingWells[levels], size
        bins]; wells: the wells of the tile (PF or not), for the evenly-spread figure."""
        b = [int(v) for v in block]
        assert len(b) == 4 + 2 * levels + len(CLASS_BIN_NAMES)
        return cls(b[0], b[1], b[2], b[3], b[4:4 + levels], b[4 + levels:4 + 2 * levels], b[4 + 2 * levels:],
                   b[2] * (int(wells) - 1) if wells > 1 else 0)

    def to_block(self) -> List[int]:
        return [self.pf, self.classes, self.in_classes, self.redundant] + self.local + self.ring_wells + self.sizes

    def __add__(self, other: "TileDupCounts") -> "TileDupCounts":
        if self.levels != other.levels:
            raise ValueError("tile duplicates of %d and %d levels" % (self.levels, other.levels))
        add = lambda a, b: [x + y for x, y in zip(a, b)]
        return TileDupCounts(self.pf + other.pf, self.classes + other.classes, self.in_classes + other.in_classes,
                             self.redundant + other.redundant, add(self.local, other.local),
                             add(self.ring_wells, other.ring_wells), add(self.sizes, other.sizes),
                             self.even_den + other.even_den)

    def tile_duplication(self) -> float:
        """Redundant wells / PF wells (0 without PF wells)."""
        return self.redundant / self.pf if self.pf else 0.0

    def local_share(self) -> float:
        """Wells in classes with a classmate in their rings (outermost level) / wells in classes."""
        return self.local[-1] / self.in_classes if self.in_classes and self.levels else 0.0


def write_tile_dups(lane, counts: Dict[str, TileDupCounts], verbose: bool = False, out=None, levels: int = 0) -> None:
    """The block that follows a lane's report (and its duplicate-set block) under --tile-dups: per-tile lines
    (verbose, in sorted tile order as write_report), the lane's sums, the class sizes, the duplication of the
    tiles as a whole and the share of it that is local."""
    out = out or sys.stdout
    if not levels:
        levels = next((c.levels for c in counts.values()), 0)
    tot = TileDupCounts.zeros(levels)
    print(file=out)
    for tile in sorted(counts.keys()):
        tc = counts[tile]
        tot = tot + tc
        if verbose:
            print("TileDups: %s\tTile: %s\tPF wells: %i\tClasses: %i\tInClasses: %i\tRedundant: %i" % (
                lane, tile, tc.pf, tc.classes, tc.in_classes, tc.redundant), file=out)
            for lev in range(levels):
                print("Level: %i\tLocal: %i\tRingWells: %i" % (lev + 1, tc.local[lev], tc.ring_wells[lev]), file=out)
    print("TileDupsSummary: %s\tTiles: %i\tPF wells: %i\tClasses: %i\tInClasses: %i (%.5f)\tRedundant: %i (%.5f)" % (
        lane, len(counts), tot.pf, tot.classes, tot.in_classes, tot.in_classes / tot.pf if tot.pf else 0.0,
        tot.redundant, tot.redundant / tot.pf if tot.pf else 0.0), file=out)
    for lev in range(levels):
        print("Level: %i\tLocal: %i (%.5f of InClasses)\tEvenly spread: %.5f" % (
            lev + 1, tot.local[lev], tot.local[lev] / tot.in_classes if tot.in_classes else 0.0,
            tot.ring_wells[lev] / tot.even_den if tot.even_den else 0.0), file=out)
    print("ClassSizes: %s" % "\t".join("%s: %i" % (name, n) for name, n in zip(CLASS_BIN_NAMES, tot.sizes)), file=out)
    print("Tile duplication (Redundant/PF wells): {:.2%}".format(tot.tile_duplication()), file=out)
    print("Local share at level {} (Local/InClasses): {:.2%}".format(levels, tot.local_share()), file=out)


@dataclass
class TileNearCounts:
    """Near-duplicate read clusters of one tile, or of several added up (include/welldup_tilenear.h,
    wd_tile_near_dups): PF wells, the clusters of >= 2 PF wells linked by Hamming distance <= K, the wells in
    them, the redundant wells (InClusters - Clusters), the pairs of distinct reads within K; per level
    (cumulative) the wells in clusters with a well of their cluster in their rings and the sizes of those wells'
    rings; size bins of the clusters.  even_den as TileDupCounts, over the wells in clusters."""
    pf: int = 0
    clusters: int = 0
    in_clusters: int = 0
    redundant: int = 0
    near_pairs: int = 0
    local: List[int] = field(default_factory=list)
    ring_wells: List[int] = field(default_factory=list)
    sizes: List[int] = field(default_factory=lambda: [0] * len(CLASS_BIN_NAMES))
    even_den: int = 0

    @property
    def levels(self) -> int:
        return len(self.local)

    @classmethod
    def zeros(cls, levels: int) -> "TileNearCounts":
        return cls(0, 0, 0, 0, 0, [0] * levels, [0] * levels, [0] * len(CLASS_BIN_NAMES), 0)

    @classmethod
    def from_block(cls, block: Sequence[int], levels: int, wells: int = 0) -> "TileNearCounts":
        """Decode one out_rows row: [PF, Clusters, InClusters, Redundant, NearPairs, Local[levels],
        RingWells[levels], size bins]; wells: the wells of the tile (PF or not)."""
        b = [int(v) for v in block]
        assert len(b) == 5 + 2 * levels + len(CLASS_BIN_NAMES)
        return cls(b[0], b[1], b[2], b[3], b[4], b[5:5 + levels], b[5 + levels:5 + 2 * levels], b[5 + 2 * levels:],
                   b[2] * (int(wells) - 1) if wells > 1 else 0)

    def to_block(self) -> List[int]:
        return ([self.pf, self.clusters, self.in_clusters, self.redundant, self.near_pairs] + self.local +
                self.ring_wells + self.sizes)

    def __add__(self, other: "TileNearCounts") -> "TileNearCounts":
        if self.levels != other.levels:
            raise ValueError("tile near-duplicates of %d and %d levels" % (self.levels, other.levels))
        add = lambda a, b: [x + y for x, y in zip(a, b)]
        return TileNearCounts(self.pf + other.pf, self.clusters + other.clusters, self.in_clusters + other.in_clusters,
                              self.redundant + other.redundant, self.near_pairs + other.near_pairs,
                              add(self.local, other.local), add(self.ring_wells, other.ring_wells),
                              add(self.sizes, other.sizes), self.even_den + other.even_den)

    def tile_duplication(self) -> float:
        """Redundant wells / PF wells (0 without PF wells)."""
        return self.redundant / self.pf if self.pf else 0.0

    def local_share(self) -> float:
        """Wells in clusters with a well of their cluster in their rings (outermost level) / wells in clusters."""
        return self.local[-1] / self.in_clusters if self.in_clusters and self.levels else 0.0


def write_tile_near_dups(lane, k: int, counts: Dict[str, TileNearCounts], verbose: bool = False, out=None,
                         levels: int = 0, equal: Optional[TileDupCounts] = None) -> None:
    """The block that follows a lane's --tile-dups block under --tile-dups-hamming K, of the same shape, for the
    clusters at Hamming distance <= K.  equal: the lane's sums of the --tile-dups block, whose tile duplication
    is printed beside that of the clusters."""
    out = out or sys.stdout
    if not levels:
        levels = next((c.levels for c in counts.values()), 0)
    tot = TileNearCounts.zeros(levels)
    print(file=out)
    for tile in sorted(counts.keys()):
        tc = counts[tile]
        tot = tot + tc
        if verbose:
            print("TileNearDups: %s\tTile: %s\tHamming: %i\tPF wells: %i\tClusters: %i\tInClusters: %i\tRedundant: %i\t"
                  "NearPairs: %i" % (lane, tile, k, tc.pf, tc.clusters, tc.in_clusters, tc.redundant, tc.near_pairs),
                  file=out)
            for lev in range(levels):
                print("Level: %i\tLocal: %i\tRingWells: %i" % (lev + 1, tc.local[lev], tc.ring_wells[lev]), file=out)
    print("TileNearDupsSummary: %s\tTiles: %i\tHamming: %i\tPF wells: %i\tClusters: %i\tInClusters: %i (%.5f)\t"
          "Redundant: %i (%.5f)\tNearPairs: %i" % (
              lane, len(counts), k, tot.pf, tot.clusters, tot.in_clusters, tot.in_clusters / tot.pf if tot.pf else 0.0,
              tot.redundant, tot.redundant / tot.pf if tot.pf else 0.0, tot.near_pairs), file=out)
    for lev in range(levels):
        print("Level: %i\tLocal: %i (%.5f of InClusters)\tEvenly spread: %.5f" % (
            lev + 1, tot.local[lev], tot.local[lev] / tot.in_clusters if tot.in_clusters else 0.0,
            tot.ring_wells[lev] / tot.even_den if tot.even_den else 0.0), file=out)
    print("ClusterSizes: %s" % "\t".join("%s: %i" % (name, n) for name, n in zip(CLASS_BIN_NAMES, tot.sizes)), file=out)
    line = "Tile duplication at Hamming <= {} (Redundant/PF wells): {:.2%}".format(k, tot.tile_duplication())
    if equal is not None:
        line += "\tby equality: {:.2%}".format(equal.tile_duplication())
    print(line, file=out)
    print("Local share at level {} (Local/InClusters): {:.2%}".format(levels, tot.local_share()), file=out)


LANE_ROW_COLS = 6 + len(CLASS_BIN_NAMES)
LANE_TILE_COLS = 5


def library_size(reads: int, distinct: int) -> Optional[float]:
    """The Lander-Waterman estimate other duplicate markers print: the X that solves
    distinct / X = 1 - exp(-reads / X), found by bisection; None when no read is redundant (no X is large
    enough) or there is no read at all."""
    n, c = float(reads), float(distinct)
    if c <= 0 or c >= n:
        return None
    f = lambda x: -x * math.expm1(-n / x) - c        # increasing in x; f(c) < 0, f(x) -> n - c > 0
    lo, hi = c, 2.0 * c
    while f(hi) <= 0.0:
        lo, hi = hi, 2.0 * hi
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if f(mid) <= 0.0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


@dataclass
class LaneDupCounts:
    """Read classes across all tiles of a lane (include/welldup_lanedups.h, the LaneDups accumulator): the lane
    row's columns, and per tile (by the tile's name) [PF, InLane, InTile, TileRedundant, LaneRedundant]."""
    pf: int = 0
    classes: int = 0
    in_classes: int = 0
    redundant: int = 0
    cross_tile_classes: int = 0
    tile_spans: int = 0
    sizes: List[int] = field(default_factory=lambda: [0] * len(CLASS_BIN_NAMES))
    tiles: Dict[str, List[int]] = field(default_factory=dict)

    @classmethod
    def from_rows(cls, lane_row: Sequence[int], tile_rows: Sequence[Sequence[int]], tile_names: Sequence) -> "LaneDupCounts":
        """lane_row and tile_rows as LaneDups.finish returns them; tile_names[i]: the name of tile index i (an
        index beyond the names, or a name of None, was never a tile of the lane and is left out)."""
        b = [int(v) for v in lane_row]
        assert len(b) == LANE_ROW_COLS
        tiles = {}
        for name, row in zip(tile_names, tile_rows):
            assert len(row) == LANE_TILE_COLS
            if name is not None:
                tiles[name] = [int(v) for v in row]
        return cls(b[0], b[1], b[2], b[3], b[4], b[5], b[6:], tiles)

    def to_rows(self):
        """-> (lane row, tile rows in sorted order of the tiles' names)"""
        return ([self.pf, self.classes, self.in_classes, self.redundant, self.cross_tile_classes, self.tile_spans] +
                list(self.sizes), [list(self.tiles[t]) for t in sorted(self.tiles)])

    @property
    def within_tiles(self) -> int:
        """Redundant wells with a classmate of smaller well index on their own tile: InClasses - TileSpans."""
        return self.in_classes - self.tile_spans

    @property
    def across_tiles(self) -> int:
        """The rest of Redundant, TileSpans - Classes: first wells of their class on a tile it did not begin on."""
        return self.tile_spans - self.classes

    def lane_duplication(self) -> float:
        """Redundant wells / PF wells (0 without PF wells)."""
        return self.redundant / self.pf if self.pf else 0.0

    def library_size(self) -> Optional[float]:
        return library_size(self.pf, self.pf - self.redundant)


def write_lane_dups(lane, counts: LaneDupCounts, verbose: bool = False, out=None) -> None:
    """The block that follows a lane's report (and its --dup-sets / --tile-dups blocks) under --lane-dups: per-tile
    lines (verbose, in sorted tile order as write_report), the lane's classes, their sizes, the redundant wells
    split into those within tiles and those across tiles, the duplication of the lane and the library size it
    lets one estimate."""
    out = out or sys.stdout
    c = counts
    print(file=out)
    if verbose:
        for tile in sorted(c.tiles):
            t = c.tiles[tile]
            print("LaneDups: %s\tTile: %s\tPF wells: %i\tInLane: %i\tInTile: %i\tTileRedundant: %i\tLaneRedundant: %i" % (
                lane, tile, t[0], t[1], t[2], t[3], t[4]), file=out)
    print("LaneDupsSummary: %s\tTiles: %i\tPF wells: %i\tClasses: %i\tInClasses: %i (%.5f)\tRedundant: %i (%.5f)\t"
          "CrossTileClasses: %i\tTileSpans: %i" % (
              lane, len(c.tiles), c.pf, c.classes, c.in_classes, c.in_classes / c.pf if c.pf else 0.0, c.redundant,
              c.redundant / c.pf if c.pf else 0.0, c.cross_tile_classes, c.tile_spans), file=out)
    print("ClassSizes: %s" % "\t".join("%s: %i" % (name, n) for name, n in zip(CLASS_BIN_NAMES, c.sizes)), file=out)
    share = lambda v: v / c.redundant if c.redundant else 0.0
    print("Redundant within tiles: %i (%.5f of Redundant)\tacross tiles: %i (%.5f of Redundant)" % (
        c.within_tiles, share(c.within_tiles), c.across_tiles, share(c.across_tiles)), file=out)
    print("Lane duplication (Redundant/PF wells): {:.2%}".format(c.lane_duplication()), file=out)
    size = c.library_size()
    print("Estimated library size (distinct/X = 1 - exp(-PF/X)): %s" % ("n/a" if size is None else "%.0f" % size),
          file=out)


LANE_NEAR_ROW_COLS = LANE_ROW_COLS + 1


@dataclass
class LaneNearCounts(LaneDupCounts):
    """Near-duplicate read clusters across all tiles of a lane (include/welldup_lanenear.h): LaneDupCounts with
    "class" read as "cluster" (classes = Clusters, in_classes = InClusters, cross_tile_classes =
    CrossTileClusters), and the pairs of distinct reads of the lane within the distance."""
    near_pairs: int = 0

    @classmethod
    def from_rows(cls, lane_row: Sequence[int], tile_rows: Sequence[Sequence[int]], tile_names: Sequence) -> "LaneNearCounts":
        """lane_row (NearPairs in front of the size bins) and tile_rows as LaneDups.finish(hamming=K) returns them"""
        b = [int(v) for v in lane_row]
        assert len(b) == LANE_NEAR_ROW_COLS
        base = LaneDupCounts.from_rows(b[:6] + b[7:], tile_rows, tile_names)
        return cls(base.pf, base.classes, base.in_classes, base.redundant, base.cross_tile_classes, base.tile_spans,
                   base.sizes, base.tiles, b[6])

    def to_rows(self):
        lane, tiles = LaneDupCounts.to_rows(self)
        return lane[:6] + [self.near_pairs] + lane[6:], tiles


def write_lane_near_dups(lane, k: int, counts: LaneNearCounts, verbose: bool = False, out=None,
                         equal: Optional[LaneDupCounts] = None) -> None:
    """The block that follows a lane's --lane-dups block under --lane-dups-hamming K, of the same shape, for the
    clusters at Hamming distance <= K.  equal: the lane's classes, whose duplication is printed beside that of the
    clusters."""
    out = out or sys.stdout
    c = counts
    print(file=out)
    if verbose:
        for tile in sorted(c.tiles):
            t = c.tiles[tile]
            print("LaneNearDups: %s\tTile: %s\tHamming: %i\tPF wells: %i\tInLane: %i\tInTile: %i\tTileRedundant: %i\t"
                  "LaneRedundant: %i" % (lane, tile, k, t[0], t[1], t[2], t[3], t[4]), file=out)
    print("LaneNearDupsSummary: %s\tTiles: %i\tHamming: %i\tPF wells: %i\tClusters: %i\tInClusters: %i (%.5f)\t"
          "Redundant: %i (%.5f)\tCrossTileClusters: %i\tTileSpans: %i\tNearPairs: %i" % (
              lane, len(c.tiles), k, c.pf, c.classes, c.in_classes, c.in_classes / c.pf if c.pf else 0.0, c.redundant,
              c.redundant / c.pf if c.pf else 0.0, c.cross_tile_classes, c.tile_spans, c.near_pairs), file=out)
    print("ClusterSizes: %s" % "\t".join("%s: %i" % (name, n) for name, n in zip(CLASS_BIN_NAMES, c.sizes)), file=out)
    share = lambda v: v / c.redundant if c.redundant else 0.0
    print("Redundant within tiles: %i (%.5f of Redundant)\tacross tiles: %i (%.5f of Redundant)" % (
        c.within_tiles, share(c.within_tiles), c.across_tiles, share(c.across_tiles)), file=out)
    line = "Lane duplication at Hamming <= {} (Redundant/PF wells): {:.2%}".format(k, c.lane_duplication())
    if equal is not None:
        line += "\tby equality: {:.2%}".format(equal.lane_duplication())
    print(line, file=out)
    size = c.library_size()
    print("Estimated library size (distinct/X = 1 - exp(-PF/X)): %s" % ("n/a" if size is None else "%.0f" % size),
          file=out)


LANE_INDEX_GROUP_COLS = 5
LANE_INDEX_LANE_COLS = 5


def index_bases(key: int, lengths: Sequence[int]) -> str:
    """An index key (include/welldup_laneindex.h: ten 3-bit codes per 32-bit word, the first word low) as bases,
    the index cycle ranges - lengths[i] cycles each - joined by '+'."""
    codes = [(int(key) >> (32 * (c // 10) + 3 * (c % 10))) & 7 for c in range(sum(lengths))]
    text = "".join("ACGTN"[min(c, 4)] for c in codes)
    parts, at = [], 0
    for n in lengths:
        parts.append(text[at:at + n])
        at += n
    return "+".join(parts)


@dataclass
class LaneIndexCounts:
    """A lane's duplication per index read (include/welldup_laneindex.h, LaneDups.index_finish): the lane index
    row's columns, the listed groups - (index read as bases, [PF, InLane, InGroup, GroupRedundant, Mixed]) by
    (-PF, key) - the Other row, and from the lane row the labels belong to its PF wells and its classes."""
    groups: int = 0
    listed: int = 0
    group_spans: int = 0
    mixed_classes: int = 0
    mixed_wells: int = 0
    other: List[int] = field(default_factory=lambda: [0] * LANE_INDEX_GROUP_COLS)
    rows: List = field(default_factory=list)
    pf: int = 0
    classes: int = 0

    @classmethod
    def from_rows(cls, lane_index_row: Sequence[int], other: Sequence[int], group_rows: Sequence[Sequence[int]],
                  keys: Sequence[int], lengths: Sequence[int], pf: int, classes: int) -> "LaneIndexCounts":
        """The four results of LaneDups.index_finish, in any order of the groups; lengths: the cycles of every
        index range; pf, classes: the lane row's PF wells and classes (clusters under --lane-dups-hamming)."""
        b = [int(v) for v in lane_index_row]
        assert len(b) == LANE_INDEX_LANE_COLS and len(other) == LANE_INDEX_GROUP_COLS and len(group_rows) == len(keys)
        order = sorted(range(len(keys)), key=lambda i: (-int(group_rows[i][0]), int(keys[i])))
        rows = []
        for i in order:
            assert len(group_rows[i]) == LANE_INDEX_GROUP_COLS
            rows.append((index_bases(keys[i], lengths), [int(v) for v in group_rows[i]]))
        assert b[1] == len(rows)
        return cls(b[0], b[1], b[2], b[3], b[4], [int(v) for v in other], rows, int(pf), int(classes))

    @property
    def within_libraries(self) -> int:
        """The sum of GroupRedundant: wells with a classmate of smaller global id in their own group."""
        return sum(r[3] for _, r in self.rows) + self.other[3]

    @property
    def across_libraries(self) -> int:
        """GroupSpans - Classes: first wells of their class in a group the class did not begin in."""
        return self.group_spans - self.classes


def write_lane_index_dups(lane, counts: LaneIndexCounts, hamming: int = 0, out=None) -> None:
    """The block that follows a lane's other blocks under --lane-dups-index: a line per listed group (library), the
    Other line, the summary.  hamming = K > 0: computed on the clusters at Hamming distance <= K, and says so."""
    out = out or sys.stdout
    c = counts
    ham = "\tHamming: %i" % hamming if hamming else ""
    share = lambda v, of: v / of if of else 0.0

    def line(name, r, size):
        print("LaneIndexDups: %s%s\tIndex: %s\tPF wells: %i (%.5f)\tInGroup: %i\tGroupRedundant: %i (%.5f)\t"
              "Library size: %s\tMixed: %i (%.5f)" % (lane, ham, name, r[0], share(r[0], c.pf), r[2], r[3], share(r[3], r[0]),
                                                      size, r[4], share(r[4], r[0])), file=out)
    print(file=out)
    for name, r in c.rows:
        size = library_size(r[0], r[0] - r[3])
        line(name, r, "n/a" if size is None else "%.0f" % size)
    line("Other", c.other, "n/a")
    red = c.within_libraries + c.across_libraries
    print("LaneIndexDupsSummary: %s%s\tGroups: %i\tListed: %i\tRedundant within libraries: %i (%.5f of Redundant)\t"
          "across libraries: %i (%.5f of Redundant)\tMixed%s: %i" % (
              lane, ham, c.groups, c.listed, c.within_libraries, share(c.within_libraries, red), c.across_libraries,
              share(c.across_libraries, red), "Clusters" if hamming else "Classes", c.mixed_classes), file=out)


LANE_MISMATCH_MAX_D = 7
LANE_MISMATCH_DIST_NAMES = ["0", "1", "2", "3", "4", "5", "6", "7", ">=8"]
LANE_MISMATCH_LANE_COLS = 4 + len(LANE_MISMATCH_DIST_NAMES)
LANE_MISMATCH_TILE_COLS = 4
CODE_NAMES = "ACGTN"


@dataclass
class LaneMismatchCounts:
    """Where a lane's duplicate copies differ (include/welldup_lanemismatch.h, LaneDups.mismatches): every redundant
    well against its root under the clusters at Hamming distance <= k.  The lane row's columns, per tile (by the
    tile's name) [Pairs, Profiled, Mismatches, WithN], sub[c][a][b] over the pairs with d <= max_d, and the number
    of every scanned cycle as --cycles counts them."""
    k: int = 0
    max_d: int = 0
    pairs: int = 0
    profiled: int = 0
    mismatches: int = 0
    with_n: int = 0
    dist: List[int] = field(default_factory=lambda: [0] * len(LANE_MISMATCH_DIST_NAMES))
    tiles: Dict[str, List[int]] = field(default_factory=dict)
    sub: List = field(default_factory=list)
    cycles: List[int] = field(default_factory=list)

    @classmethod
    def from_rows(cls, lane_row: Sequence[int], tile_rows: Sequence[Sequence[int]], sub, tile_names: Sequence, k: int,
                  max_d: int, cycles: Optional[Sequence[int]] = None) -> "LaneMismatchCounts":
        """The three results of LaneDups.mismatches(max_d); tile_names as LaneDupCounts.from_rows takes them; cycles:
        the scanned cycles' numbers (default 0, 1, ..)."""
        b = [int(v) for v in lane_row]
        assert len(b) == LANE_MISMATCH_LANE_COLS and 0 <= max_d <= LANE_MISMATCH_MAX_D
        tiles = {}
        for name, row in zip(tile_names, tile_rows):
            assert len(row) == LANE_MISMATCH_TILE_COLS
            if name is not None:
                tiles[name] = [int(v) for v in row]
        sub = [[[int(v) for v in row] for row in cell] for cell in sub]
        assert all(len(cell) == 5 and all(len(row) == 5 for row in cell) for cell in sub)
        cycles = list(range(len(sub))) if cycles is None else [int(c) for c in cycles]
        assert len(cycles) == len(sub)
        return cls(int(k), int(max_d), b[0], b[1], b[2], b[3], b[4:], tiles, sub, cycles)

    def per_cycle(self):
        """-> [(mismatches, of which with N)] per scanned cycle"""
        return [(sum(map(sum, cell)), sum(cell[4]) + sum(row[4] for row in cell[:4])) for cell in self.sub]

    def symmetric(self, a: int, b: int) -> int:
        """The profiled pairs with codes a and b, either way round, summed over the cycles."""
        return sum(cell[a][b] + cell[b][a] for cell in self.sub)

    def per_pair(self) -> float:
        """Mismatches per profiled pair (0 without one)."""
        return self.mismatches / self.profiled if self.profiled else 0.0

    def error_rate(self) -> float:
        """Mismatches / (2 x Profiled x cycles): what a base's error rate would be if both copies of a pair carried
        errors alike.  Truncated from above: pairs further apart than the clusters link are never seen."""
        den = 2 * self.profiled * len(self.sub)
        return self.mismatches / den if den else 0.0


def write_lane_mismatches(lane, counts: LaneMismatchCounts, verbose: bool = False, out=None) -> None:
    """The block that follows every other block of a lane under --lane-dups-mismatches: per-tile and per-cycle lines
    (verbose; tiles in sorted order as write_report, cycles numbered as --cycles), then the summary: the distances of
    the redundant wells from their roots, the mismatches per profiled pair and the per-base rate they imply, the
    substitutions with either direction summed, and the share of the last distance the clusters still link."""
    out = out or sys.stdout
    c = counts
    share = lambda v, of: v / of if of else 0.0
    print(file=out)
    if verbose:
        for tile in sorted(c.tiles):
            t = c.tiles[tile]
            print("LaneMismatches: %s\tTile: %s\tPairs: %i\tProfiled: %i\tMismatches: %i\tWithN: %i" % (
                lane, tile, t[0], t[1], t[2], t[3]), file=out)
        for cycle, (n, with_n) in zip(c.cycles, c.per_cycle()):
            print("LaneMismatches: %s\tCycle: %i\tMismatches: %i (%.6f per profiled pair)\tWithN: %i" % (
                lane, cycle, n, share(n, c.profiled), with_n), file=out)
    print("LaneMismatchesSummary: %s\tTiles: %i\tHamming: %i\tMaxD: %i\tPairs: %i\tProfiled: %i (%.5f)\tMismatches: %i\t"
          "WithN: %i" % (lane, len(c.tiles), c.k, c.max_d, c.pairs, c.profiled, share(c.profiled, c.pairs), c.mismatches,
                         c.with_n), file=out)
    print("Dist: %s" % "\t".join("%s: %i (%.5f)" % (name, n, share(n, c.pairs))
                                 for name, n in zip(LANE_MISMATCH_DIST_NAMES, c.dist)), file=out)
    print("Mismatches per profiled pair: %.5f" % c.per_pair(), file=out)
    print("Implied error rate per base (Mismatches / (2 x Profiled x %i cycles)): %.3e" % (len(c.sub), c.error_rate()),
          file=out)
    for a in range(4):
        for b in range(a + 1, 4):
            n = c.symmetric(a, b)
            print("Substitution: %s<>%s\t%i (%.5f of Mismatches)" % (CODE_NAMES[a], CODE_NAMES[b], n, share(n, c.mismatches)),
                  file=out)
    for a in range(4):
        n = c.symmetric(a, 4)
        print("Substitution: %s<>N\t%i (%.5f of Mismatches)" % (CODE_NAMES[a], n, share(n, c.mismatches)), file=out)
    last = min(c.k, len(c.dist) - 1)
    near = sum(c.dist[1:last + 1])
    print("Pairs at distance %i, the last the clusters link: %i (%.5f of the pairs at 1..%i, %.5f of Pairs)" % (
        last, c.dist[last] if last else 0, share(c.dist[last] if last else 0, near), last, share(c.dist[last] if last else 0, c.pairs)),
          file=out)


LANE_DISTANCE_EDGES = [32 << b for b in range(10)]                     # 32, 64, .., 16384: where a Dist bin ends
LANE_DISTANCE_DIST_NAMES = (["<32"] + ["%i-%i" % (e, 2 * e) for e in LANE_DISTANCE_EDGES[:-1]] +
                            [">=%i" % LANE_DISTANCE_EDGES[-1]])
LANE_DISTANCE_LANE_COLS = 3 + len(LANE_DISTANCE_DIST_NAMES)
LANE_DISTANCE_TILE_COLS = 3
LANE_DISTANCE_MAX_RADIUS = 1 << 25
LANE_DISTANCE_CROSS_NAMES = ["adjacent tile of the swath", "same surface otherwise", "other surface"]


def cross_tile_category(a: str, b: str) -> int:
    """Where tile b lies seen from tile a, by their names S W TT (surface, swath, tile; workload.tiles_for_stype):
    0 = same surface and swath and the next tile number, 1 = same surface otherwise, 2 = the other surface (or a
    name that is not of that form)."""
    a, b = str(a), str(b)
    if len(a) < 3 or len(b) < 3 or not (a.isdigit() and b.isdigit()) or a[0] != b[0]:
        return 2
    return 0 if a[1] == b[1] and abs(int(a[2:]) - int(b[2:])) == 1 else 1


@dataclass
class LaneDistanceCounts:
    """How far apart a lane's duplicate copies lie (include/welldup_lanedistance.h, LaneDups.distances): every
    redundant well against its root.  The lane row's columns, per tile (by the tile's name) [Pairs, SameTile, Local],
    the cross-tile pairs by where the root's tile lies (cross_tile_category; None without TilePairs) beside the share
    each category would have if copies fell on tiles in proportion to their PF wells, the area of the coordinates'
    bounding box, and from the lane row the labels belong to: PF wells, Redundant and InClasses - TileSpans."""
    radius: int = 0
    pairs: int = 0
    same_tile: int = 0
    local: int = 0
    dist: List[int] = field(default_factory=lambda: [0] * len(LANE_DISTANCE_DIST_NAMES))
    tiles: Dict[str, List[int]] = field(default_factory=dict)
    cross: Optional[List[int]] = None
    cross_by_pf: Optional[List[float]] = None
    area: float = 0.0
    pf: int = 0
    redundant: int = 0
    within_tiles: int = 0

    @classmethod
    def from_rows(cls, lane_row: Sequence[int], tile_rows: Sequence[Sequence[int]], tile_pairs, tile_names: Sequence,
                  radius: int, final: "LaneDupCounts", area: float) -> "LaneDistanceCounts":
        """The three results of LaneDups.distances(x, y, radius) (tile_pairs may be None); tile_names as
        LaneDupCounts.from_rows takes them; final: the LaneDupCounts (LaneNearCounts under --lane-dups-hamming) of
        the labels the lane was left with; area: (max x - min x) * (max y - min y) of the coordinates."""
        b = [int(v) for v in lane_row]
        assert len(b) == LANE_DISTANCE_LANE_COLS and 0 <= radius <= LANE_DISTANCE_MAX_RADIUS
        tiles = {}
        for name, row in zip(tile_names, tile_rows):
            assert len(row) == LANE_DISTANCE_TILE_COLS
            if name is not None:
                tiles[name] = [int(v) for v in row]
        cross = by_pf = None
        if tile_pairs is not None:
            named = [(i, name) for i, name in enumerate(tile_names) if name is not None and i < len(tile_pairs)]
            cross, weight = [0, 0, 0], [0.0, 0.0, 0.0]
            for i, a in named:
                for j, c in named:
                    if i < j:
                        cat = cross_tile_category(a, c)
                        cross[cat] += int(tile_pairs[i][j]) + int(tile_pairs[j][i])
                        weight[cat] += float(final.tiles[a][0] if a in final.tiles else 0) * \
                            float(final.tiles[c][0] if c in final.tiles else 0)
            total = sum(weight)
            by_pf = [w / total if total else 0.0 for w in weight]
        return cls(int(radius), b[0], b[1], b[2], b[3:], tiles, cross, by_pf, float(area), final.pf, final.redundant,
                   final.within_tiles)

    @property
    def cross_tile(self) -> int:
        return self.pairs - self.same_tile

    def coverage(self) -> float:
        """SameTile / (InClasses - TileSpans): the share of the redundant wells with an earlier classmate on their own
        tile that the pairing with the root sees as same-tile pairs (the rest: their root lies on another tile)."""
        return self.same_tile / self.within_tiles if self.within_tiles else 0.0

    def uniform_shares(self) -> List[float]:
        """Per Dist bin the share a copy placed uniformly over the tile would have: pi (hi^2 - lo^2) / area, without
        an edge correction, capped so that the bins sum to at most 1 (the open bin takes what is left); zeros
        without an area."""
        edges = [0.0] + [float(e) for e in LANE_DISTANCE_EDGES] + [math.inf]
        if self.area <= 0:                               # (no wells, or all on a line: nothing to hold against)
            return [0.0] * len(LANE_DISTANCE_DIST_NAMES)
        out, left = [], 1.0
        for lo, hi in zip(edges, edges[1:]):
            raw = math.pi * (hi * hi - lo * lo) / self.area if hi < math.inf else math.inf
            out.append(min(raw, left))
            left -= out[-1]
        return out

    def library_size_without_local(self) -> Optional[float]:
        """library_size with the local copies taken out of the reads, as other duplicate markers take out their
        optical duplicates: (PF - Local) reads, PF - Redundant of them distinct."""
        return library_size(self.pf - self.local, self.pf - self.redundant)


def write_lane_distances(lane, counts: LaneDistanceCounts, verbose: bool = False, out=None) -> None:
    """The block that closes a lane's output under --lane-dups-distance: per-tile lines (verbose, in sorted tile
    order as write_report), then the summary: the redundant wells by where their root lies, the distances of the
    same-tile pairs beside what uniformly placed copies would give, the cross-tile pairs by where the root's tile
    lies beside what the tiles' PF wells would give, and the library size without the local copies."""
    out = out or sys.stdout
    c = counts
    share = lambda v, of: v / of if of else 0.0
    print(file=out)
    if verbose:
        for tile in sorted(c.tiles):
            t = c.tiles[tile]
            print("LaneDistances: %s\tTile: %s\tPairs: %i\tSameTile: %i\tLocal: %i" % (lane, tile, t[0], t[1], t[2]), file=out)
    print("LaneDistancesSummary: %s\tTiles: %i\tR: %i\tPairs: %i\tSameTile: %i (%.5f)\tLocal: %i (%.5f)\t"
          "SameTile of the wells with an earlier classmate on their tile: %.5f" % (
              lane, len(c.tiles), c.radius, c.pairs, c.same_tile, share(c.same_tile, c.pairs), c.local,
              share(c.local, c.pairs), c.coverage()), file=out)
    print("Dist (share of SameTile; uniform~: a copy placed uniformly over the tile, an approximation without edges): %s" %
          "\t".join("%s: %i (%.5f, uniform~ %.5f)" % (name, n, share(n, c.same_tile), u)
                    for name, n, u in zip(LANE_DISTANCE_DIST_NAMES, c.dist, c.uniform_shares())), file=out)
    if c.cross is not None:
        print("Cross-tile pairs: %i\t%s" % (c.cross_tile, "\t".join(
            "%s: %i (%.5f, by PF wells %.5f)" % (name, n, share(n, c.cross_tile), p)
            for name, n, p in zip(LANE_DISTANCE_CROSS_NAMES, c.cross, c.cross_by_pf))), file=out)
    size = c.library_size_without_local()
    print("Estimated library size without local copies (R = %i; distinct/X = 1 - exp(-(PF - Local)/X)): %s" % (
        c.radius, "n/a" if size is None else "%.0f" % size), file=out)


LANE_QUALITY_MAX_D = 7
LANE_QUALITY_MAX_BINS = 8
LANE_QUALITY_VALUES = 64
LANE_QUALITY_COLS = 4


@dataclass
class LaneQualityCounts:
    """A lane's reported base quality against its duplicate copies (include/welldup_lanequality.h,
    LaneDups.qualities): the bins' lower edges, the lane row's columns, per tile (by the tile's name) [Pairs,
    Profiled, Observations, Mismatches], QHist by raw quality, and Obs and Mis by [root's bin][member's bin] over the
    pairs with d <= max_d.  k = 0: the labels are classes, every copy is identical."""
    k: int = 0
    max_d: int = 0
    edges: List[int] = field(default_factory=lambda: [0])
    pairs: int = 0
    profiled: int = 0
    observations: int = 0
    mismatches: int = 0
    tiles: Dict[str, List[int]] = field(default_factory=dict)
    qhist: List[int] = field(default_factory=lambda: [0] * LANE_QUALITY_VALUES)
    obs: List[List[int]] = field(default_factory=lambda: [[0] * LANE_QUALITY_MAX_BINS for _ in range(LANE_QUALITY_MAX_BINS)])
    mis: List[List[int]] = field(default_factory=lambda: [[0] * LANE_QUALITY_MAX_BINS for _ in range(LANE_QUALITY_MAX_BINS)])

    @classmethod
    def from_rows(cls, lane_row: Sequence[int], tile_rows: Sequence[Sequence[int]], qhist, obs, mis, tile_names: Sequence,
                  k: int, max_d: int, edges: Sequence[int]) -> "LaneQualityCounts":
        """The five results of LaneDups.qualities(max_d); tile_names as LaneDupCounts.from_rows takes them; edges: what
        LaneDups.qual_begin got."""
        b = [int(v) for v in lane_row]
        edges = [int(e) for e in edges]
        assert len(b) == LANE_QUALITY_COLS and 0 <= max_d <= LANE_QUALITY_MAX_D
        assert 1 <= len(edges) <= LANE_QUALITY_MAX_BINS and edges[0] == 0 and edges == sorted(edges) and edges[-1] < LANE_QUALITY_VALUES
        tiles = {}
        for name, row in zip(tile_names, tile_rows):
            assert len(row) == LANE_QUALITY_COLS
            if name is not None:
                tiles[name] = [int(v) for v in row]
        qhist = [int(v) for v in qhist]
        obs, mis = ([[int(v) for v in row] for row in m] for m in (obs, mis))
        assert len(qhist) == LANE_QUALITY_VALUES
        assert all(len(m) == LANE_QUALITY_MAX_BINS and all(len(row) == LANE_QUALITY_MAX_BINS for row in m) for m in (obs, mis))
        return cls(int(k), int(max_d), edges, b[0], b[1], b[2], b[3], tiles, qhist, obs, mis)

    def bin_range(self, b: int):
        """-> (lowest, highest quality of bin b); highest < lowest for a bin that an equal edge leaves empty"""
        return self.edges[b], (self.edges[b + 1] if b + 1 < len(self.edges) else LANE_QUALITY_VALUES) - 1

    def values(self, b: int) -> List[int]:
        """the raw qualities seen in bin b"""
        lo, hi = self.bin_range(b)
        return [q for q in range(lo, hi + 1) if self.qhist[q]]

    def seen(self, b: int) -> int:
        """the PF observations of the lane in bin b"""
        lo, hi = self.bin_range(b)
        return sum(self.qhist[lo:hi + 1])

    def roots(self, b: int) -> int:
        return sum(self.obs[b])

    def members(self, b: int) -> int:
        return sum(row[b] for row in self.obs)

    def occupied(self) -> List[int]:
        return [b for b in range(len(self.edges)) if self.seen(b) or self.roots(b) or self.members(b)]

    def mean_quality(self, b: int) -> Optional[float]:
        lo, hi = self.bin_range(b)
        n = self.seen(b)
        return sum(q * self.qhist[q] for q in range(lo, hi + 1)) / n if n else None

    def error_rate(self, b: int) -> Optional[float]:
        """Mis[b][b] / (2 x Obs[b][b]): the two bases of such an observation were reported alike, so either is as
        likely to be the wrong one.  None without an observation."""
        return self.mis[b][b] / (2 * self.obs[b][b]) if self.obs[b][b] else None

    def error_rate_against_top(self, b: int) -> Optional[float]:
        """(Mis[b][t] + Mis[t][b]) / (Obs[b][t] + Obs[t][b]) - error_rate(t), not below 0, t the highest occupied bin:
        what is left for the base of bin b once the other's share is taken off.  None for t itself and without an
        observation on either side."""
        occ = self.occupied()
        t = occ[-1] if occ else None
        if t is None or b == t or self.error_rate(t) is None:
            return None
        den = self.obs[b][t] + self.obs[t][b]
        return max(0.0, (self.mis[b][t] + self.mis[t][b]) / den - self.error_rate(t)) if den else None


def phred(rate: Optional[float]) -> str:
    """-10 log10 of an error rate as text: "-" for None, "inf" for 0"""
    if rate is None:
        return "-"
    return "inf" if rate <= 0 else "%.1f" % (-10.0 * math.log10(rate) + 0.0)      # (+ 0.0: a rate of 1 is Q 0.0, not -0.0)


def write_lane_qualities(lane, counts: LaneQualityCounts, verbose: bool = False, out=None) -> None:
    """The block that closes a lane's output under --lane-dups-quality: per-tile lines (verbose, in sorted tile order
    as write_report), the summary line with the caveats, a line per occupied quality bin - its range, the raw values
    seen in it, its share of the lane's PF observations, of the roots' and of the members' observations, the mean
    reported quality, the error rate and empirical quality among pairs of that bin, and the error rate against the
    highest occupied bin - and (verbose) Obs and Mis row by row."""
    out = out or sys.stdout
    c = counts
    share = lambda v, of: v / of if of else 0.0
    rate = lambda r: "-" if r is None else "%.3e" % r
    print(file=out)
    if verbose:
        for tile in sorted(c.tiles):
            t = c.tiles[tile]
            print("LaneQualities: %s\tTile: %s\tPairs: %i\tProfiled: %i\tObservations: %i\tMismatches: %i" % (
                lane, tile, t[0], t[1], t[2], t[3]), file=out)
    caveat = ("rates are truncated from above: clusters only link within %i; distinct molecules within %i inflate them"
              % (c.k, c.k)) if c.k else \
        "under equality every copy is identical: only the reported qualities of copies against the lane's are shown"
    print("LaneQualitiesSummary: %s\tTiles: %i\tHamming: %i\tMaxD: %i\tPairs: %i\tProfiled: %i (%.5f)\tObservations: %i\t"
          "Mismatches: %i\t(%s)" % (lane, len(c.tiles), c.k, c.max_d, c.pairs, c.profiled, share(c.profiled, c.pairs),
                                    c.observations, c.mismatches, caveat), file=out)
    total = sum(c.qhist)
    for b in c.occupied():
        lo, hi = c.bin_range(b)
        mean = c.mean_quality(b)
        e, top = c.error_rate(b), c.error_rate_against_top(b)
        print("LaneQualities: %s\tBin: %i-%i\tValues: %s\tPF share: %.5f\tRoots: %.5f\tMembers: %.5f\tMean Q: %s\t"
              "Error rate: %s (Q %s)\tAgainst top bin: %s (Q %s)" % (
                  lane, lo, hi, ",".join(str(q) for q in c.values(b)) or "-", share(c.seen(b), total),
                  share(c.roots(b), c.observations), share(c.members(b), c.observations),
                  "-" if mean is None else "%.2f" % mean, rate(e), phred(e), rate(top), phred(top)), file=out)
    if verbose:
        for name, m in (("Obs", c.obs), ("Mis", c.mis)):
            for a in range(len(c.edges)):
                print("LaneQualities: %s\t%s root bin %i-%i:\t%s" % ((lane, name) + c.bin_range(a) + (
                    "\t".join(str(v) for v in m[a][:len(c.edges)]),)), file=out)


LANE_SATURATION_MAX_STEPS = 64
LANE_SATURATION_MAX_RADIUS = LANE_DISTANCE_MAX_RADIUS


@dataclass
class LaneSaturationCounts:
    """A lane's distinct reads against its depth (include/welldup_lanesaturation.h, LaneDups.saturation): PF wells,
    the wells dropped as local copies (closer than `radius` to their root on its tile; 0 without a radius), Redundant
    of the lane row the labels belong to, and per step the counted wells and the distinct reads the step brought.
    k = 0: the labels are classes; K > 0: clusters at Hamming distance <= K."""
    pf: int = 0
    dropped: int = 0
    redundant: int = 0
    new_reads: List[int] = field(default_factory=lambda: [0])
    new_distinct: List[int] = field(default_factory=lambda: [0])
    steps: int = 1
    seed: int = 0
    radius: int = 0
    k: int = 0

    @classmethod
    def from_rows(cls, head: Sequence[int], new_reads: Sequence[int], new_distinct: Sequence[int], seed: int, radius: int,
                  final: "LaneDupCounts", k: int = 0) -> "LaneSaturationCounts":
        """The three results of LaneDups.saturation(steps, seed, x, y, radius); final: the LaneDupCounts
        (LaneNearCounts under --lane-dups-hamming K = k) of the labels the lane was left with."""
        h = [int(v) for v in head]
        r, d = [int(v) for v in new_reads], [int(v) for v in new_distinct]
        assert len(h) == 2 and 1 <= len(r) == len(d) <= LANE_SATURATION_MAX_STEPS
        assert 0 <= radius <= LANE_SATURATION_MAX_RADIUS and 0 <= seed < 1 << 32
        assert sum(r) == h[0] - h[1] and sum(d) == h[0] - final.redundant and h[0] == final.pf
        return cls(h[0], h[1], final.redundant, r, d, len(r), int(seed), int(radius), int(k))

    def cumulative(self):
        """-> (reads, distinct) of the subsample at each step"""
        reads, distinct, a, b = [], [], 0, 0
        for r, d in zip(self.new_reads, self.new_distinct):
            a, b = a + r, b + d
            reads.append(a)
            distinct.append(b)
        return reads, distinct

    def half_step(self) -> int:
        """the step whose nominal share (j + 1) / S is nearest a half (the earlier of two)"""
        return min(range(self.steps), key=lambda j: (abs(2 * (j + 1) - self.steps), j))

    def size_ratio(self) -> Optional[float]:
        """library_size at full depth over library_size at half_step(); None where either has no solution"""
        reads, distinct = self.cumulative()
        j = self.half_step()
        full, half = library_size(reads[-1], distinct[-1]), library_size(reads[j], distinct[j])
        return full / half if full is not None and half is not None else None

    def projection(self, factor: float):
        """-> (distinct reads, duplication) Lander-Waterman gives at factor x the counted reads with the full-depth
        library size; None without one"""
        reads, distinct = self.cumulative()
        size = library_size(reads[-1], distinct[-1])
        if size is None:
            return None
        n = factor * reads[-1]
        c = -size * math.expm1(-n / size)
        return c, 1.0 - c / n


def write_lane_saturation(lane, counts: LaneSaturationCounts, verbose: bool = False, out=None) -> None:
    """The block that closes a lane's output under --lane-dups-saturation: a line per step (verbose) - its nominal
    share of the reads, the reads and distinct reads up to it, their duplication, the library size they give and
    the step's own yield of new molecules -, then the summary: what the last reads still brought (measured), whether
    the library size holds at half the depth (the model's test), what the model projects for more reads, and the
    local copies that were left out."""
    out = out or sys.stdout
    c = counts
    share = lambda v, of: v / of if of else 0.0
    size_text = lambda s: "n/a" if s is None else "%.0f" % s
    reads, distinct = c.cumulative()
    print(file=out)
    if verbose:
        for j in range(c.steps):
            print("LaneSaturation: %s\tStep: %i/%i\tShare: %.5f\tReads: %i\tDistinct: %i\tDuplication: %.5f\t"
                  "Library size: %s\tNewReads: %i\tNewDistinct: %i\tYield: %.5f" % (
                      lane, j + 1, c.steps, (j + 1) / c.steps, reads[j], distinct[j], 1.0 - share(distinct[j], reads[j])
                      if reads[j] else 0.0, size_text(library_size(reads[j], distinct[j])), c.new_reads[j],
                      c.new_distinct[j], share(c.new_distinct[j], c.new_reads[j])), file=out)
    print("LaneSaturationSummary: %s\tSteps: %i\tSeed: %i\tHamming: %i\tPF wells: %i\tDropped: %i\tReads: %i\t"
          "Distinct: %i\tDuplication: %.5f\tLibrary size: %s" % (
              lane, c.steps, c.seed, c.k, c.pf, c.dropped, reads[-1], distinct[-1],
              1.0 - share(distinct[-1], reads[-1]) if reads[-1] else 0.0, size_text(library_size(reads[-1], distinct[-1]))),
          file=out)
    print("New molecules per 1000 further reads (measured, no model: the last step's %i reads brought %i): %s" % (
        c.new_reads[-1], c.new_distinct[-1],
        "%.1f" % (1000.0 * c.new_distinct[-1] / c.new_reads[-1]) if c.new_reads[-1] else "n/a"), file=out)
    j = c.half_step()
    ratio = c.size_ratio()
    print("Library size at full depth / at step %i/%i: %s (near 1: equally likely molecules, as Lander-Waterman assumes, "
          "fit; well above 1: the library is more uneven and the size a lower bound)" % (
              j + 1, c.steps, "n/a" if ratio is None else "%.3f" % ratio), file=out)
    proj = [(f, c.projection(f)) for f in (2, 4)]
    print("Projection (Lander-Waterman with the full-depth size, not a measurement): %s" % "\t".join(
        "%ix reads: n/a" % f if p is None else "%ix reads: %.0f distinct, duplication %.5f" % (f, p[0], p[1])
        for f, p in proj), file=out)
    if c.radius > 0:
        print("Local copies dropped: %i closer than R = %i to the first well of their class on its tile (%.5f of PF wells)" % (
            c.dropped, c.radius, share(c.dropped, c.pf)), file=out)
    else:
        print("Local copies dropped: none (no radius)", file=out)


LANE_TOP_MAX = 1024
LANE_TOP_EDGES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50, 100, 500, 1000, 5000, 10000)


def lane_top_note(read: str, size: int, tiles_touched: int) -> str:
    """What a listed read looks like, from the read alone: 'all N'; 'poly-A/C/G/T' when at least 90 % of the called
    bases are one base; 'N-rich' at 20 % N or more; 'one tile' when the whole group lies on one tile and has at least
    ten wells; else empty.  The first that applies."""
    called = [b for b in read if b != "N"]
    if read and not called:
        return "all N"
    for base in "ACGT":
        if called and 10 * called.count(base) >= 9 * len(called):
            return "poly-" + base
    if read and 5 * (len(read) - len(called)) >= len(read):
        return "N-rich"
    if tiles_touched == 1 and size >= 10:
        return "one tile"
    return ""


@dataclass
class LaneTopCounts:
    """A lane's most frequent reads and their spread (include/welldup_lanetop.h, LaneDups.top): PF wells, the groups
    of at least two wells, per duplication level the groups and their wells, and the listed groups - root, size, the
    wells whose read equals the root's, the wells per tile, the root's read.  redundant: Redundant of the lane row
    the labels belong to.  k = 0: the groups are classes; K > 0: clusters at Hamming distance <= K."""
    pf: int = 0
    groups2: int = 0
    covered: int = 0
    redundant: int = 0
    groups: List[int] = field(default_factory=lambda: [0] * len(LANE_TOP_EDGES))
    wells: List[int] = field(default_factory=lambda: [0] * len(LANE_TOP_EDGES))
    root: List[int] = field(default_factory=list)
    size: List[int] = field(default_factory=list)
    exact: List[int] = field(default_factory=list)
    tile_count: List[List[int]] = field(default_factory=list)
    reads: List[str] = field(default_factory=list)
    tiles: List[str] = field(default_factory=list)
    n_wells: int = 1
    n_top: int = 1
    k: int = 0

    @classmethod
    def from_rows(cls, head: Sequence[int], levels, root, size, exact, tile_count, reads: Sequence[str], n_top: int,
                  n_wells: int, tiles: Sequence[str], final: "LaneDupCounts", k: int = 0) -> "LaneTopCounts":
        """The seven results of LaneDups.top(n_top); n_wells: the wells of a tile; tiles: the tiles' names by tile
        index; final: the LaneDupCounts (LaneNearCounts under --lane-dups-hamming K = k) of the labels the lane was
        left with."""
        h = [int(v) for v in head]
        g, w = ([int(v) for v in row] for row in levels)
        counts = [[int(v) for v in row] for row in tile_count]
        assert len(h) == 4 and len(g) == len(w) == len(LANE_TOP_EDGES) and 1 <= n_top <= LANE_TOP_MAX
        assert h[2] == min(n_top, h[1]) == len(root) == len(size) == len(exact) == len(counts) == len(reads)
        assert sum(w) == h[0] == final.pf and sum(g[1:]) == h[1] and sum(w[1:]) - h[1] == final.redundant
        assert all(len(row) == len(tiles) and sum(row) == s for row, s in zip(counts, size))
        return cls(h[0], h[1], h[3], final.redundant, g, w, [int(v) for v in root], [int(v) for v in size],
                   [int(v) for v in exact], counts, list(reads), [str(t) for t in tiles], int(n_wells), int(n_top), int(k))

    def listed_redundancy(self) -> int:
        """the redundant wells that lie in the listed groups: sum(size - 1)"""
        return sum(s - 1 for s in self.size)


def write_lane_top(lane, counts: LaneTopCounts, verbose: bool = False, out=None) -> None:
    """The block that closes a lane's output under --lane-dups-top: (a) a line per non-empty duplication level - its
    groups, its wells, their share of the distinct reads and of the PF reads -, (b) the listed groups - rank, size,
    share of PF, the root's tile and well, the tiles touched, the largest share of the group on one tile, the wells
    that equal the root's read (clusters only), the read and a note (lane_top_note) -, (c) the share of the lane's
    redundancy that lies in the listed groups.  Not verbose: (c), the top level line and the first five entries."""
    out = out or sys.stdout
    c = counts
    share = lambda v, of: v / of if of else 0.0
    distinct = sum(c.groups)
    print(file=out)
    occupied = [i for i in range(len(LANE_TOP_EDGES)) if c.groups[i]]
    for i in occupied if verbose else occupied[-1:]:
        last = i + 1 == len(LANE_TOP_EDGES)
        hi = None if last else LANE_TOP_EDGES[i + 1] - 1
        name = ">=%i" % LANE_TOP_EDGES[i] if last else str(hi) if hi == LANE_TOP_EDGES[i] else "%i-%i" % (LANE_TOP_EDGES[i], hi)
        print("LaneTopLevel: %s\tSize: %s\tGroups: %i\tWells: %i\tOf distinct: %.5f\tOf PF: %.5f" % (
            lane, name, c.groups[i], c.wells[i], share(c.groups[i], distinct), share(c.wells[i], c.pf)), file=out)
    if c.k and c.root:
        print("LaneTop: %s\tthe read shown is that of the cluster's first well (Hamming <= %i), not a consensus" % (lane, c.k),
              file=out)
    for r in range(len(c.root) if verbose else min(5, len(c.root))):
        row = c.tile_count[r]
        touched = sum(1 for v in row if v)
        t, w = divmod(c.root[r], c.n_wells)
        exact = "\tExact: %i/%i" % (c.exact[r], c.size[r]) if c.k else ""
        print("LaneTop: %s\tRank: %i\tSize: %i\tOf PF: %.5f\tRoot: %s:%i\tTiles: %i\tLargest tile share: %.5f%s\tRead: %s\t"
              "Note: %s" % (lane, r + 1, c.size[r], share(c.size[r], c.pf), c.tiles[t], w, touched,
                            share(max(row), c.size[r]), exact, c.reads[r], lane_top_note(c.reads[r], c.size[r], touched) or "-"),
              file=out)
    print("LaneTopSummary: %s\tAsked: %i\tListed: %i\tHamming: %i\tPF wells: %i\tGroups: %i\tCovered: %i (%.5f of PF)\t"
          "Redundant in listed: %i of %i (%.5f)" % (
              lane, c.n_top, len(c.root), c.k, c.pf, c.groups2, c.covered, share(c.covered, c.pf), c.listed_redundancy(),
              c.redundant, share(c.listed_redundancy(), c.redundant)), file=out)


def write_lane_top_tsv(lane, counts: LaneTopCounts, out, header: bool = True) -> None:
    """--lane-dups-top-out: a line per listed group - lane, rank, size, exact, tiles, root_tile, root_well, read - and
    then a tile=count column per tile the group touches."""
    c = counts
    if header:
        print("lane\trank\tsize\texact\ttiles\troot_tile\troot_well\tread", file=out)
    for r in range(len(c.root)):
        t, w = divmod(c.root[r], c.n_wells)
        cols = ["%s=%i" % (c.tiles[i], v) for i, v in enumerate(c.tile_count[r]) if v]
        print("\t".join([str(lane), str(r + 1), str(c.size[r]), str(c.exact[r]), str(len(cols)), c.tiles[t], str(w),
                         c.reads[r]] + cols), file=out)


LANE_HOPS_MAX_E = 3
LANE_HOPS_MAX_LISTED = 1024
LANE_HOPS_STATE_NAMES = ("Same", "Near", "Far")
LANE_HOPS_TILE_COLS = 4
LANE_HOPS_LANE_COLS = LANE_HOPS_TILE_COLS + 9


@dataclass
class LaneHopCounts:
    """Which libraries a lane's duplicate copies join (include/welldup_lanehops.h, LaneDups.hops): the index read of
    every redundant well against its root's.  The lane row's columns - state[3 s1 + s2] with s = 0 Same, 1 Near (at
    most max_e cycles of the index read differ), 2 Far -, per tile (by the tile's name) [Pairs, SameTile, Hop1, Hop2],
    the listed libraries' keys, names (bases; the last is Other) and PF wells (the last: every PF well of the lane
    whose key is not listed), and matrix[root's library][copy's library]."""
    k: int = 0
    split: int = 1
    single: bool = True
    max_e: int = 0
    n_pairs: int = 10
    pairs: int = 0
    same_tile: int = 0
    hop1: int = 0
    hop2: int = 0
    state: List[int] = field(default_factory=lambda: [0] * 9)
    tiles: Dict[str, List[int]] = field(default_factory=dict)
    keys: List[int] = field(default_factory=list)
    names: List[str] = field(default_factory=lambda: ["Other"])
    pf: List[int] = field(default_factory=lambda: [0])
    matrix: List[List[int]] = field(default_factory=lambda: [[0]])

    @classmethod
    def from_rows(cls, lane_row: Sequence[int], tile_rows: Sequence[Sequence[int]], matrix, keys: Sequence[int],
                  pf: Sequence[int], lengths: Sequence[int], tile_names: Sequence, max_e: int, k: int = 0,
                  n_pairs: int = 10) -> "LaneHopCounts":
        """The three results of LaneDups.hops(lengths[0], max_e, keys); keys: the listed keys in the order given to
        it; pf: the PF wells of each listed library and, last, of all the others; lengths: the cycles of every index
        range (the first is the split; one range is a single index); tile_names as LaneDupCounts.from_rows takes
        them; k: the K of --lane-dups-hamming; n_pairs: the library pairs write_lane_hops lists."""
        b = [int(v) for v in lane_row]
        m = len(keys)
        assert len(b) == LANE_HOPS_LANE_COLS and 0 <= max_e <= LANE_HOPS_MAX_E and m <= LANE_HOPS_MAX_LISTED
        assert len(pf) == m + 1 and len(matrix) == m + 1 and all(len(row) == m + 1 for row in matrix)
        tiles = {}
        for name, row in zip(tile_names, tile_rows):
            assert len(row) == LANE_HOPS_TILE_COLS
            if name is not None:
                tiles[name] = [int(v) for v in row]
        names = [index_bases(key, lengths) for key in keys] + ["Other"]
        return cls(int(k), int(lengths[0]), len(lengths) == 1 or lengths[0] == sum(lengths), int(max_e), int(n_pairs),
                   b[0], b[1], b[2], b[3], b[4:], tiles, [int(key) for key in keys], names, [int(v) for v in pf],
                   [[int(v) for v in row] for row in matrix])

    @property
    def errors_only(self) -> int:
        """The pairs with an index-read error and no other index: no part Far, not both Same."""
        return sum(self.state[s] for s in (1, 3, 4))

    @property
    def off_diagonal(self) -> int:
        """H: the pairs whose root and copy lie in different libraries (Other being one)."""
        return sum(map(sum, self.matrix)) - sum(self.matrix[i][i] for i in range(len(self.matrix)))

    def within(self, a: int) -> int:
        return self.matrix[a][a]

    def exchanged(self, a: int) -> int:
        """The pairs with exactly one end in library a: its row and its column without the diagonal."""
        return sum(self.matrix[a]) + sum(row[a] for row in self.matrix) - 2 * self.matrix[a][a]

    def into_listed(self) -> int:
        """The off-diagonal pairs whose copy carries a listed key - a matrix count, not a state count (see
        write_lane_hops)."""
        m = len(self.keys)
        return sum(self.matrix[a][b] for a in range(m + 1) for b in range(m) if a != b)

    def into_unlisted(self) -> int:
        """The pairs of a listed root whose copy carries no listed key: column Other without its diagonal."""
        m = len(self.keys)
        return sum(self.matrix[a][m] for a in range(m))

    def expected(self, a: int, b: int) -> Optional[Fraction]:
        """What random exchange between libraries a and b would give: H x 2 p_a p_b / (1 - sum p_i^2), p the PF
        shares over the listed libraries and Other - an exact fraction; None where the denominator is 0 (no PF well,
        or one library holds them all)."""
        total = sum(self.pf)
        den = total * total - sum(v * v for v in self.pf)
        return Fraction(self.off_diagonal * 2 * self.pf[a] * self.pf[b], den) if den else None

    def top_pairs(self):
        """-> [(a, b, count)], a < b: the unordered library pairs with a pair between them, [a][b] + [b][a], by
        count (largest first), then by the two keys (Other last)."""
        m = len(self.keys)
        key = lambda i: self.keys[i] if i < m else 1 << 64
        got = [(a, b, self.matrix[a][b] + self.matrix[b][a]) for a in range(m + 1) for b in range(a + 1, m + 1)
               if self.matrix[a][b] + self.matrix[b][a]]
        return sorted(got, key=lambda t: (-t[2], ) + tuple(sorted((key(t[0]), key(t[1])))))


def write_lane_hops(lane, counts: LaneHopCounts, verbose: bool = False, out=None) -> None:
    """The block that follows every other block of a lane under --lane-dups-hops: (a) a line per state that can
    occur - nine, or three for a single index -: the states of the two index reads, the pairs and their share;
    (b) verbose: a line per tile; (c) a line per listed library and one for Other: the index read, its PF wells, the
    pairs inside it, the pairs with one end in it and their share of its PF wells; (d) the n_pairs largest unordered
    library pairs: count, share of all pairs between libraries, what random exchange would give and the ratio to it
    (n/a where that is 0 or undefined); (e) the summary.
    Its last two counts before SameTile are matrix counts, not state counts: "into a listed library" is every pair
    whose copy carries a listed key other than its root's, "into an unlisted combination" every pair of a listed
    root whose copy's key is not listed.  With max_e = 0 every pair off the diagonal has a Far part and they split
    Hop1 + Hop2 (less the pairs between two unlisted keys, which lie in the one cell Other x Other).  With max_e >= 1
    a Near pair is off the diagonal too - its key differs from its root's, and is rarely listed -, so "into an
    unlisted combination" then holds the index-read errors as well and the two can exceed Hop1 + Hop2."""
    out = out or sys.stdout
    c = counts
    ham = "\tHamming: %i" % c.k if c.k else ""
    share = lambda v, of: v / of if of else 0.0
    print(file=out)
    for s in range(9):
        if c.single and s % 3:
            continue
        print("LaneHops: %s%s\tIndex1: %s\tIndex2: %s\tPairs: %i (%.5f)" % (
            lane, ham, LANE_HOPS_STATE_NAMES[s // 3], "-" if c.single else LANE_HOPS_STATE_NAMES[s % 3], c.state[s],
            share(c.state[s], c.pairs)), file=out)
    if verbose:
        for tile in sorted(c.tiles):
            t = c.tiles[tile]
            print("LaneHopsTile: %s\tTile: %s\tPairs: %i\tSameTile: %i\tHop1: %i\tHop2: %i" % (
                lane, tile, t[0], t[1], t[2], t[3]), file=out)
    for a, name in enumerate(c.names):
        print("LaneHopLibrary: %s%s\tIndex: %s\tPF wells: %i\tWithin: %i\tExchanged: %i (%.6f of PF)" % (
            lane, ham, name, c.pf[a], c.within(a), c.exchanged(a), share(c.exchanged(a), c.pf[a])), file=out)
    h = c.off_diagonal
    for a, b, n in c.top_pairs()[:max(0, c.n_pairs)]:
        e = c.expected(a, b)
        print("LaneHopPair: %s%s\tIndex: %s\tIndex: %s\tPairs: %i (%.5f)\tExpected: %s\tRatio: %s" % (
            lane, ham, c.names[a], c.names[b], n, share(n, h), "n/a" if e is None else "%.2f" % float(e),
            "%.3f" % float(n / e) if e else "n/a"), file=out)
    print("LaneHopsSummary: %s%s\tSplit: %s\tMaxE: %i\tListed: %i\tPairs: %i\tSame index: %i (%.5f)\t"
          "Index-read errors only: %i (%.5f)\tOne index read swapped: %i (%.6f per pair)\tBoth: %i\t"
          "Into a listed library: %i\tInto an unlisted combination: %i\tSameTile: %i" % (
              lane, ham, "single" if c.single else str(c.split), c.max_e, len(c.keys), c.pairs, c.state[0],
              share(c.state[0], c.pairs), c.errors_only, share(c.errors_only, c.pairs), c.hop1, share(c.hop1, c.pairs),
              c.hop2, c.into_listed(), c.into_unlisted(), c.same_tile), file=out)


def write_lane_hops_tsv(lane, counts: LaneHopCounts, out, header: bool = True) -> None:
    """--lane-dups-hops-out: a line per cell of the matrix that is not zero - lane, the root's index read, the
    copy's, the pairs -, row by row."""
    c = counts
    if header:
        print("lane\tindex_a\tindex_b\tpairs", file=out)
    for a, row in enumerate(c.matrix):
        for b, n in enumerate(row):
            if n:
                print("%s\t%s\t%s\t%i" % (lane, c.names[a], c.names[b], n), file=out)


# ---- --lane-dups-gc: a lane's duplication against its reads' GC content (include/welldup_lanegc.h) ----
LANE_GC_HIST_COLS = 4
LANE_GC_LANE_COLS = 8
LANE_GC_TILE_COLS = 5
LANE_GC_MIN_BINS, LANE_GC_MAX_BINS = 2, 100


def gc_quartiles(distinct: Sequence[int]):
    """distinct[g]: the distinct molecules with GC g -> (q1, q3), the quartiles of g over them cut at whole g: q1 is
    the smallest g with 4 x (molecules at or below g) >= the molecules, q3 the smallest with 4 x (molecules at or
    below g) >= 3 x the molecules.  Every molecule of one g lies on the same side of a cut: "at or below the first
    quartile" is g <= q1 (it holds at least a quarter of the molecules, more when q1 is a tie), "above the third"
    g > q3 (at most a quarter), and the rest, q1 < g <= q3, lies between.  (0, 0) without a molecule."""
    total, below, q1, q3 = sum(distinct), 0, None, None
    if total == 0:
        return 0, 0
    for g, n in enumerate(distinct):
        below += n
        if q1 is None and 4 * below >= total:
            q1 = g
        if q3 is None and 4 * below >= 3 * total:
            q3 = g
    return q1, q3


def hist_over(hist, keys) -> List[int]:
    """hist[key] = [Single, Roots, Copies, FamilyWells] (the GC pass's by g, the adapter pass's by a) -> [distinct
    molecules, reads by the molecule's key, redundant wells, Roots, FamilyWells, Copies by their own read] summed over
    the keys."""
    rows = [hist[key] for key in keys]
    s, r, c, f = (sum(row[i] for row in rows) for i in range(4))
    return [s + r, s + f, f - r, r, f, c]


def _share(v, of):
    return v / of if of else 0.0


def _num(v, fmt="%.5f"):
    return "n/a" if v is None else fmt % v


def hist_bin_columns(part, every) -> str:
    """The columns a line of the GC block and of the adapter block share, from hist_over of the line's keys and of
    every key: the distinct molecules and their share, the reads by the molecule's key, the redundant wells among
    them, the duplication in the bin and against the lane's, the mean family size, the copies by their own read and
    library_size of the bin."""
    distinct, reads, redundant, roots, family, copies = part
    dup, lane_dup = _share(redundant, reads), _share(every[2], every[1])
    return ("Distinct: %i (%.5f)\tReads: %i\tRedundant: %i\tDuplication: %.5f\tRelative: %s\tMeanFamily: %s\t"
            "Copies: %i\tLibrarySize: %s" % (
                distinct, _share(distinct, every[0]), reads, redundant, dup,
                _num(dup / lane_dup if lane_dup else None, "%.3f"), _num(family / roots if roots else None, "%.3f"),
                copies, _num(library_size(reads, distinct), "%.0f")))


@dataclass
class LaneGCCounts:
    """A lane's duplication against its reads' GC content (include/welldup_lanegc.h, LaneDups.gc): the lane row's
    columns, per tile (by the tile's name) [PF, Counted, GC, CopiesCounted, CopiesGC], and hist[g] = [Single, Roots,
    Copies, FamilyWells] for g = 0 .. L over the wells with at most max_n no-calls."""
    k: int = 0
    max_n: int = 0
    bins: int = 20
    pf: int = 0
    single: int = 0
    roots: int = 0
    copies: int = 0
    skip_single: int = 0
    skip_roots: int = 0
    skip_copies: int = 0
    skip_family_wells: int = 0
    tiles: Dict[str, List[int]] = field(default_factory=dict)
    hist: List[List[int]] = field(default_factory=lambda: [[0] * LANE_GC_HIST_COLS])

    @classmethod
    def from_rows(cls, lane_row: Sequence[int], tile_rows: Sequence[Sequence[int]], hist, tile_names: Sequence,
                  max_n: int, bins: int = 20, k: int = 0) -> "LaneGCCounts":
        """The three results of LaneDups.gc(max_n); tile_names as LaneDupCounts.from_rows takes them; bins: the lines
        write_lane_gc prints; k: the K of --lane-dups-hamming."""
        b = [int(v) for v in lane_row]
        h = [[int(v) for v in row] for row in hist]
        assert len(b) == LANE_GC_LANE_COLS and len(h) >= 1 and all(len(row) == LANE_GC_HIST_COLS for row in h)
        assert LANE_GC_MIN_BINS <= bins <= LANE_GC_MAX_BINS and 0 <= max_n <= len(h) - 1
        tiles = {}
        for name, row in zip(tile_names, tile_rows):
            assert len(row) == LANE_GC_TILE_COLS
            if name is not None:
                tiles[name] = [int(v) for v in row]
        return cls(int(k), int(max_n), int(bins), *b, tiles, h)

    @property
    def cycles(self) -> int:
        return len(self.hist) - 1

    @property
    def skipped(self) -> int:
        return self.skip_single + self.skip_roots + self.skip_copies

    @property
    def counted(self) -> int:
        return self.pf - self.skipped

    def bin_of(self, g: int) -> int:
        """min(B - 1, g * B // L), in integers: g = L alone would open a bin of its own."""
        return min(self.bins - 1, g * self.bins // self.cycles) if self.cycles else 0

    def over(self, gs) -> List[int]:
        """[distinct molecules, reads by the molecule's GC, redundant wells, Roots, FamilyWells, Copies by their own
        read] summed over the g of gs."""
        return hist_over(self.hist, gs)

    def mean_gc(self, col) -> Optional[float]:
        """The mean of g / L over the wells of col(row) per g; None without a well."""
        n = sum(col(row) for row in self.hist)
        return sum(g * col(row) for g, row in enumerate(self.hist)) / (n * self.cycles) if n and self.cycles else None

    def tile_means(self):
        """tile -> (mean GC of its counted reads, of its counted copies), None for none."""
        per = lambda gc, n: gc / (n * self.cycles) if n and self.cycles else None
        return {t: (per(r[2], r[1]), per(r[4], r[3])) for t, r in self.tiles.items()}


def write_lane_gc(lane, counts: LaneGCCounts, verbose: bool = False, out=None) -> None:
    """The block that follows every other block of a lane under --lane-dups-gc: a line per GC bin - the range of g
    it takes, the distinct molecules (Single + Roots) and their share, the reads by the molecule's GC (Single +
    FamilyWells), the redundant wells among them (FamilyWells - Roots), the duplication in the bin and against the
    lane's, the mean family size (FamilyWells / Roots), the copies by their own read, library_size of the bin -, with
    verbose a line per tile and the tile whose mean lies furthest from the lane's (the first in sorted order on a tie),
    then the summary: mean GC of the distinct
    molecules and of the redundant wells (the copies, each by its own read) and the shift between them, the
    duplication among the molecules at or below the first quartile of GC, between the quartiles and above the third
    (gc_quartiles), and the bin with the highest duplication among those that hold at least 1 % of the distinct
    molecules (the lowest such bin on a tie)."""
    out = out or sys.stdout
    c = counts
    ham = "\tHamming: %i" % c.k if c.k else ""
    share = lambda v, of: v / of if of else 0.0
    num = lambda v, fmt="%.5f": "n/a" if v is None else fmt % v
    L = c.cycles
    every = c.over(range(L + 1))
    lane_dup = share(every[2], every[1])
    print(file=out)
    best = None
    for b in range(c.bins):
        gs = [g for g in range(L + 1) if c.bin_of(g) == b]
        distinct, reads, redundant, roots, family, copies = c.over(gs)
        dup = share(redundant, reads)
        if distinct and 100 * distinct >= every[0] and (best is None or dup > best[1]):
            best = (b, dup, gs)
        print("LaneGC: %s%s\tBin: %i\tGC: %s\t%s" % (
            lane, ham, b, "%i-%i" % (gs[0], gs[-1]) if gs else "-", hist_bin_columns(c.over(gs), every)), file=out)
    lane_mean = share(sum(t[2] for t in c.tiles.values()), sum(t[1] for t in c.tiles.values()) * L)
    if verbose:
        means = c.tile_means()
        for tile in sorted(c.tiles):
            t = c.tiles[tile]
            print("LaneGCTile: %s\tTile: %s\tPF: %i\tCounted: %i\tMeanGC: %s\tCopies: %i\tCopiesMeanGC: %s" % (
                lane, tile, t[0], t[1], num(means[tile][0]), t[3], num(means[tile][1])), file=out)
        gc, n = sum(t[2] for t in c.tiles.values()), sum(t[1] for t in c.tiles.values())
        far = [(abs(Fraction(c.tiles[t][2], c.tiles[t][1]) - Fraction(gc, n)), t) for t in sorted(c.tiles) if c.tiles[t][1]]
        if far:                                          # (in exact arithmetic: the first of the sorted tiles on a tie)
            d, t = max(far, key=lambda e: e[0])
            print("LaneGCTiles: %s\tLaneMeanGC: %.5f\tFurthest: %s (%.5f, %+.5f)" % (
                lane, lane_mean, t, means[t][0], means[t][0] - lane_mean), file=out)
    m_distinct = c.mean_gc(lambda row: row[0] + row[1])
    m_copies = c.mean_gc(lambda row: row[2])
    q1, q3 = gc_quartiles([row[0] + row[1] for row in c.hist])
    parts = [c.over(range(0, q1 + 1)), c.over(range(q1 + 1, q3 + 1)), c.over(range(q3 + 1, L + 1))]
    print("LaneGCSummary: %s%s\tMaxN: %i\tCycles: %i\tBins: %i\tCounted: %i\tSkipped: %i\tDistinct: %i\t"
          "Duplication: %.5f\tMeanGC distinct: %s\tMeanGC redundant: %s\tShift: %s\tQ1: %i\tQ3: %i\t"
          "Duplication at or below Q1: %.5f\tbetween: %.5f\tabove Q3: %.5f\tHighest: %s" % (
              lane, ham, c.max_n, L, c.bins, c.counted, c.skipped, every[0], lane_dup, num(m_distinct), num(m_copies),
              num(m_copies - m_distinct if m_distinct is not None and m_copies is not None else None, "%+.5f"), q1, q3,
              share(parts[0][2], parts[0][1]), share(parts[1][2], parts[1][1]), share(parts[2][2], parts[2][1]),
              "n/a" if best is None else "bin %i (GC %i-%i, %.5f)" % (best[0], best[2][0], best[2][-1], best[1])), file=out)


def write_lane_gc_tsv(lane, counts: LaneGCCounts, out, header: bool = True) -> None:
    """--lane-dups-gc-out: a line per g = 0 .. L - lane, gc, single, roots, copies, family_wells."""
    if header:
        print("lane\tgc\tsingle\troots\tcopies\tfamily_wells", file=out)
    for g, row in enumerate(counts.hist):
        print("%s\t%i\t%i\t%i\t%i\t%i" % (lane, g, row[0], row[1], row[2], row[3]), file=out)


# ---- --lane-dups-adapter: a lane's duplication by insert length (include/welldup_laneadapter.h) ----
LANE_ADAPTER_HIST_COLS = 4
LANE_ADAPTER_LANE_COLS = 10
LANE_ADAPTER_TILE_COLS = 5
LANE_ADAPTER_MIN_BINS, LANE_ADAPTER_MAX_BINS = 2, 100


@dataclass
class LaneAdapterCounts:
    """A lane's duplication by insert length (include/welldup_laneadapter.h, LaneDups.adapter): the lane row's
    columns, per tile (by the tile's name) [PF, Adapter, Copies, CopiesAdapter, SumA], and hist[a] = [Single, Roots,
    Copies, FamilyWells] for a = 0 .. L, row L the reads without adapter."""
    k: int = 0
    name: str = ""
    m: int = 0
    max_e: int = 1
    min_overlap: int = 8
    bins: int = 10
    dimer: int = 10
    first_cycle: int = 0
    pf: int = 0
    single: int = 0
    roots: int = 0
    copies: int = 0
    ad_single: int = 0
    ad_roots: int = 0
    ad_copies: int = 0
    ad_family_wells: int = 0
    inexact: int = 0
    partial: int = 0
    tiles: Dict[str, List[int]] = field(default_factory=dict)
    hist: List[List[int]] = field(default_factory=lambda: [[0] * LANE_ADAPTER_HIST_COLS])

    @classmethod
    def from_rows(cls, lane_row: Sequence[int], tile_rows: Sequence[Sequence[int]], hist, tile_names: Sequence,
                  name: str, m: int, max_e: int, min_overlap: int, bins: int = 10, dimer: int = 10, k: int = 0,
                  first_cycle: int = 0) -> "LaneAdapterCounts":
        """The three results of LaneDups.adapter(codes, max_e, min_overlap); tile_names as LaneDupCounts.from_rows
        takes them; name: what --lane-dups-adapter was given; m: the adapter's length; bins: the lines
        write_lane_adapter prints; dimer: the largest a of an adapter dimer; k: the K of --lane-dups-hamming;
        first_cycle: the number of the first scanned cycle, as --cycles counts them."""
        b = [int(v) for v in lane_row]
        h = [[int(v) for v in row] for row in hist]
        assert len(b) == LANE_ADAPTER_LANE_COLS and len(h) >= 1 and all(len(row) == LANE_ADAPTER_HIST_COLS for row in h)
        assert LANE_ADAPTER_MIN_BINS <= bins <= LANE_ADAPTER_MAX_BINS and dimer >= 0
        tiles = {}
        for tname, row in zip(tile_names, tile_rows):
            assert len(row) == LANE_ADAPTER_TILE_COLS
            if tname is not None:
                tiles[tname] = [int(v) for v in row]
        return cls(int(k), str(name), int(m), int(max_e), int(min_overlap), int(bins), int(dimer), int(first_cycle), *b,
                   tiles, h)

    @property
    def cycles(self) -> int:
        return len(self.hist) - 1

    @property
    def with_adapter(self) -> int:
        return self.ad_single + self.ad_roots + self.ad_copies

    def bin_of(self, a: int) -> int:
        """of a < L: min(B - 1, a * B // L): bins of equal width over 0 .. L - 1"""
        return min(self.bins - 1, a * self.bins // self.cycles)

    def over(self, positions) -> List[int]:
        """hist_over of these rows: the columns the GC block counts per bin, here by the molecule's a."""
        return hist_over(self.hist, positions)

    def mean_a(self, col) -> Optional[float]:
        """The mean of a over the wells with adapter of col(row) per a; None without a well."""
        n = sum(col(row) for row in self.hist[:-1])
        return sum(a * col(row) for a, row in enumerate(self.hist[:-1])) / n if n else None


def write_lane_adapter(lane, counts: LaneAdapterCounts, verbose: bool = False, out=None) -> None:
    """The block that follows the GC block of a lane under --lane-dups-adapter: a line per bin of a - the range of
    positions it takes, numbered from the first scanned cycle, and the columns of a GC bin (hist_bin_columns), by the
    molecule's a - and a line "none" for the reads without adapter; with verbose a line per tile; then the summary:
    the share of PF reads with adapter, the share that are dimers (a <= the dimer length), the duplication of the
    dimers, of the other reads with adapter and of the reads without, the first matches that are inexact and partial
    as shares of the matches, and the mean a of the distinct molecules and of the redundant wells (the copies, each by
    its own read).  Offset: the first scanned cycle where that is not 0 - the inserts are longer by it."""
    out = out or sys.stdout
    c = counts
    ham = "\tHamming: %i" % c.k if c.k else ""
    L = c.cycles
    every = c.over(range(L + 1))
    print(file=out)
    for b in range(c.bins):
        ps = [a for a in range(L) if c.bin_of(a) == b]
        print("LaneAdapter: %s%s\tBin: %i\tInsert: %s\t%s" % (
            lane, ham, b, "%i-%i" % (c.first_cycle + ps[0], c.first_cycle + ps[-1]) if ps else "-",
            hist_bin_columns(c.over(ps), every)), file=out)
    print("LaneAdapter: %s%s\tBin: none\tInsert: -\t%s" % (lane, ham, hist_bin_columns(c.over([L]), every)), file=out)
    if verbose:
        for tile in sorted(c.tiles):
            t = c.tiles[tile]
            print("LaneAdapterTile: %s\tTile: %s\tPF: %i\tAdapter: %i (%.5f)\tMeanInsert: %s\tCopies: %i\t"
                  "CopiesAdapter: %i (%.5f)" % (lane, tile, t[0], t[1], _share(t[1], t[0]),
                                                _num(c.first_cycle + t[4] / t[1] if t[1] else None, "%.2f"), t[2], t[3],
                                                _share(t[3], t[2])), file=out)
    cut = min(c.dimer + 1, L)
    parts = [c.over(range(cut)), c.over(range(cut, L)), c.over([L])]
    dimers = sum(sum(row[:3]) for row in c.hist[:cut])
    m_distinct, m_copies = c.mean_a(lambda row: row[0] + row[1]), c.mean_a(lambda row: row[2])
    mean = lambda v: _num(None if v is None else c.first_cycle + v, "%.2f")
    print("LaneAdapterSummary: %s%s\tAdapter: %s\tLength: %i\tMismatches: %i\tMinOverlap: %i\tCycles: %i\t%sBins: %i\t"
          "PF: %i\tWithAdapter: %i (%.5f)\tDimers (a <= %i): %i (%.5f)\tDuplication: %.5f\tDuplication of dimers: %.5f\t"
          "of other reads with adapter: %.5f\tof reads without: %.5f\tInexact: %i (%.5f)\tPartial: %i (%.5f)\t"
          "MeanInsert distinct: %s\tMeanInsert redundant: %s" % (
              lane, ham, c.name, c.m, c.max_e, c.min_overlap, L,
              "Offset: %i\t" % c.first_cycle if c.first_cycle else "", c.bins, c.pf, c.with_adapter,
              _share(c.with_adapter, c.pf), c.dimer, dimers, _share(dimers, c.pf), _share(every[2], every[1]),
              _share(parts[0][2], parts[0][1]), _share(parts[1][2], parts[1][1]), _share(parts[2][2], parts[2][1]),
              c.inexact, _share(c.inexact, c.with_adapter), c.partial, _share(c.partial, c.with_adapter),
              mean(m_distinct), mean(m_copies)), file=out)


def write_lane_adapter_tsv(lane, counts: LaneAdapterCounts, out, header: bool = True) -> None:
    """--lane-dups-adapter-out: a line per a = 0 .. L - 1 and a line "none" - lane, insert (a numbered from the first
    scanned cycle), single, roots, copies, family_wells, cumulative: the share of PF reads with a at or before the
    line's - the adapter content curve, exact; "-" on the last line."""
    if header:
        print("lane\tinsert\tsingle\troots\tcopies\tfamily_wells\tcumulative", file=out)
    seen = 0
    for a, row in enumerate(counts.hist):
        seen += sum(row[:3])
        last = a == counts.cycles
        print("%s\t%s\t%i\t%i\t%i\t%i\t%s" % (lane, "none" if last else "%i" % (counts.first_cycle + a), row[0], row[1],
                                              row[2], row[3], "-" if last else "%.5f" % _share(seen, counts.pf)), file=out)


# ---- --lane-dups-consensus: a lane's errors against its families' vote (include/welldup_laneconsensus.h) ----
LANE_CONSENSUS_MAX_D = 7
LANE_CONSENSUS_MIN_FAMILY, LANE_CONSENSUS_MAX_FAMILY = 3, 4096
LANE_CONSENSUS_DIST_NAMES = LANE_MISMATCH_DIST_NAMES
LANE_CONSENSUS_LANE_COLS = 11 + len(LANE_CONSENSUS_DIST_NAMES)
LANE_CONSENSUS_TILE_COLS = 4


@dataclass
class LaneConsensusCounts:
    """A lane's errors against its families' vote (include/welldup_laneconsensus.h, LaneDups.consensus): the lane
    row's columns, per tile (by the tile's name) [Wells, Profiled, Mismatches, WithN], calls[c][a][b] - consensus a,
    own code b - over the wells with d <= max_d of the families of 3 .. max_family wells, the number of every scanned
    cycle as --cycles counts them, and the lane's PF wells."""
    k: int = 0
    max_d: int = 0
    max_family: int = 256
    pf: int = 0
    families: int = 0
    wells: int = 0
    profiled: int = 0
    mismatches: int = 0
    with_n: int = 0
    undecided: int = 0
    undecided_calls: int = 0
    first_off: int = 0
    pairs: int = 0
    large: int = 0
    large_wells: int = 0
    dist: List[int] = field(default_factory=lambda: [0] * len(LANE_CONSENSUS_DIST_NAMES))
    tiles: Dict[str, List[int]] = field(default_factory=dict)
    calls: List = field(default_factory=list)
    cycles: List[int] = field(default_factory=list)

    @classmethod
    def from_rows(cls, lane_row: Sequence[int], tile_rows: Sequence[Sequence[int]], calls, tile_names: Sequence, k: int,
                  max_d: int, max_family: int, pf: int, cycles: Optional[Sequence[int]] = None) -> "LaneConsensusCounts":
        """The three results of LaneDups.consensus(max_d, max_family); tile_names as LaneDupCounts.from_rows takes
        them; pf: the lane's PF wells (the finish's lane row); cycles: the scanned cycles' numbers (default 0, 1, ..)."""
        b = [int(v) for v in lane_row]
        assert len(b) == LANE_CONSENSUS_LANE_COLS and 0 <= max_d <= LANE_CONSENSUS_MAX_D
        assert LANE_CONSENSUS_MIN_FAMILY <= max_family <= LANE_CONSENSUS_MAX_FAMILY
        tiles = {}
        for name, row in zip(tile_names, tile_rows):
            assert len(row) == LANE_CONSENSUS_TILE_COLS
            if name is not None:
                tiles[name] = [int(v) for v in row]
        calls = [[[int(v) for v in row] for row in cell] for cell in calls]
        assert all(len(cell) == 5 and all(len(row) == 5 for row in cell) for cell in calls)
        cycles = list(range(len(calls))) if cycles is None else [int(c) for c in cycles]
        assert len(cycles) == len(calls)
        return cls(int(k), int(max_d), int(max_family), int(pf), *b[:11], b[11:], tiles, calls, cycles)

    def called(self) -> int:
        """Every call that was compared: the sum of calls."""
        return sum(sum(map(sum, cell)) for cell in self.calls)

    def error_rate(self) -> Optional[float]:
        """Mismatches per called base; None without a call."""
        n = self.called()
        return self.mismatches / n if n else None

    def count(self, a: int, b: int) -> int:
        """The calls of b where the consensus is a, over the cycles."""
        return sum(cell[a][b] for cell in self.calls)

    def rate(self, a: int, b: int) -> Optional[float]:
        """P(call b | molecule a) over the cycles; None where no consensus is a."""
        n = sum(sum(cell[a]) for cell in self.calls)
        return self.count(a, b) / n if n else None

    def per_cycle(self):
        """-> [(calls, errors, the most frequent substitution as (count, a, b) or None)] per scanned cycle; of equally
        frequent substitutions the first in the order of the codes"""
        rows = []
        for cell in self.calls:
            off = [(cell[a][b], -a, -b) for a in range(5) for b in range(5) if a != b and cell[a][b]]
            top = max(off) if off else None
            rows.append((sum(map(sum, cell)), sum(e[0] for e in off), None if top is None else (top[0], -top[1], -top[2])))
        return rows


def write_lane_consensus(lane, counts: LaneConsensusCounts, verbose: bool = False, out=None) -> None:
    """The block that follows every other block of a lane under --lane-dups-consensus: per-tile and per-cycle lines
    (verbose; tiles in sorted order as write_report, cycles numbered as --cycles: the calls compared, the errors
    among them, their rate and the most frequent substitution), then the summary: the families that voted and their
    wells, the errors per called base and the quality that amounts to, the (family, cycle) pairs without a majority,
    the families whose first well disagrees with the vote - what wd_lane_mismatches counts once per copy and in the
    wrong direction -, the distances of the wells from their family's consensus, and the twelve substitutions
    molecule>call with each direction's rate and its ratio to the reverse direction."""
    out = out or sys.stdout
    c = counts
    share = lambda v, of: v / of if of else 0.0
    sci = lambda v: "n/a" if v is None else "%.3e" % v
    name = lambda a, b: "%s>%s" % (CODE_NAMES[a], CODE_NAMES[b])
    print(file=out)
    if verbose:
        for tile in sorted(c.tiles):
            t = c.tiles[tile]
            print("LaneConsensus: %s\tTile: %s\tWells: %i\tProfiled: %i\tMismatches: %i\tWithN: %i" % (
                lane, tile, t[0], t[1], t[2], t[3]), file=out)
        for cycle, (n, errors, top) in zip(c.cycles, c.per_cycle()):
            print("LaneConsensus: %s\tCycle: %i\tCalls: %i\tErrors: %i\tRate: %s\tMost frequent: %s" % (
                lane, cycle, n, errors, sci(errors / n if n else None),
                "-" if top is None else "%s (%i)" % (name(top[1], top[2]), top[0])), file=out)
    rate = c.error_rate()
    print("LaneConsensusSummary: %s\tTiles: %i\tHamming: %i\tMaxD: %i\tMaxFamily: %i\tFamilies: %i\tWells: %i (%.5f of PF)\t"
          "Profiled: %i (%.5f)\tMismatches: %i\tWithN: %i\tErrors per called base: %s (Q %s)\tUndecided: %i\t"
          "FirstWellOff: %i (%.5f of Families)\tPairs left out: %i\tLarge left out: %i (%i wells)" % (
              lane, len(c.tiles), c.k, c.max_d, c.max_family, c.families, c.wells, share(c.wells, c.pf), c.profiled,
              share(c.profiled, c.wells), c.mismatches, c.with_n, sci(rate), phred(rate), c.undecided, c.first_off,
              share(c.first_off, c.families), c.pairs, c.large, c.large_wells), file=out)
    print("ConsensusDist: %s" % "\t".join("%s: %i (%.5f)" % (n, v, share(v, c.wells))
                                          for n, v in zip(LANE_CONSENSUS_DIST_NAMES, c.dist)), file=out)
    for a in range(4):
        for b in range(4):
            if a == b:
                continue
            fwd, rev = c.rate(a, b), c.rate(b, a)
            ratio = "n/a" if fwd is None or rev is None or (fwd == 0 and rev == 0) else "inf" if rev == 0 else "%.3f" % (fwd / rev)
            print("Consensus: %s\t%i (%.5f of Mismatches)\tRate: %s\tReverse %s: %i\tRatio: %s" % (
                name(a, b), c.count(a, b), share(c.count(a, b), c.mismatches), sci(fwd), name(b, a), c.count(b, a), ratio),
                  file=out)
    to_n, from_n = sum(c.count(a, 4) for a in range(4)), sum(c.count(4, b) for b in range(4))
    print("Consensus: N\tmolecule>N: %i\tN>call: %i\t(%.5f of Mismatches)" % (to_n, from_n, share(to_n + from_n, c.mismatches)),
          file=out)


def write_lane_consensus_tsv(lane, counts: LaneConsensusCounts, out, header: bool = True) -> None:
    """--lane-dups-consensus-out: a line per cell of calls that is not zero - lane, cycle, consensus, call, count."""
    if header:
        print("lane\tcycle\tconsensus\tcall\tcount", file=out)
    for cycle, cell in zip(counts.cycles, counts.calls):
        for a in range(5):
            for b in range(5):
                if cell[a][b]:
                    print("%s\t%i\t%s\t%s\t%i" % (lane, cycle, CODE_NAMES[a], CODE_NAMES[b], cell[a][b]), file=out)


# ---- --lane-dups-umi: a lane's duplicates split by molecular identifier (include/welldup_laneumi.h) ----
LANE_UMI_MAX_E = 3
LANE_UMI_MIN_FAMILY, LANE_UMI_MAX_FAMILY = 2, 1024
LANE_UMI_MAX_CYCLES = 20
LANE_UMI_BIN_NAMES = ("1", "2", "3", "4", "5-8", "9-16", "17-64", "65+")
LANE_UMI_TILE_COLS = 3
LANE_UMI_LANE_COLS = LANE_UMI_TILE_COLS + 8 + 2 * len(LANE_UMI_BIN_NAMES)


@dataclass
class LaneUmiCounts:
    """A lane's duplicates split by molecular identifier (include/welldup_laneumi.h, LaneDups.umi): the lane row's
    columns, per tile (by the tile's name) [Wells, UmiRedundant, Lone], and of the finish whose labels were split the
    lane's PF wells and its redundant wells."""
    k: int = 0
    max_e: int = 0
    max_family: int = 256
    umi_cycles: int = 0
    pf: int = 0
    redundant: int = 0
    wells: int = 0
    umi_redundant: int = 0
    lone: int = 0
    families: int = 0
    molecules: int = 0
    distinct_umis: int = 0
    split_families: int = 0
    split_wells: int = 0
    with_n: int = 0
    large: int = 0
    large_wells: int = 0
    per_family: List[int] = field(default_factory=lambda: [0] * len(LANE_UMI_BIN_NAMES))
    sizes: List[int] = field(default_factory=lambda: [0] * len(LANE_UMI_BIN_NAMES))
    tiles: Dict[str, List[int]] = field(default_factory=dict)

    @classmethod
    def from_rows(cls, lane_row: Sequence[int], tile_rows: Sequence[Sequence[int]], tile_names: Sequence, k: int, max_e: int,
                  max_family: int, umi_cycles: int, pf: int, redundant: int) -> "LaneUmiCounts":
        """The two results of LaneDups.umi(max_e, max_family); tile_names as LaneDupCounts.from_rows takes them; k: the
        K of --lane-dups-hamming; umi_cycles: U; pf, redundant: PF and Redundant of the finish's lane row."""
        b = [int(v) for v in lane_row]
        n = len(LANE_UMI_BIN_NAMES)
        assert len(b) == LANE_UMI_LANE_COLS and 0 <= max_e <= LANE_UMI_MAX_E
        assert LANE_UMI_MIN_FAMILY <= max_family <= LANE_UMI_MAX_FAMILY and 1 <= umi_cycles <= LANE_UMI_MAX_CYCLES
        tiles = {}
        for name, row in zip(tile_names, tile_rows):
            assert len(row) == LANE_UMI_TILE_COLS
            if name is not None:
                tiles[name] = [int(v) for v in row]
        return cls(int(k), int(max_e), int(max_family), int(umi_cycles), int(pf), int(redundant), *b[:11], b[11:11 + n],
                   b[11 + n:], tiles)

    def to_rows(self):
        """-> (lane row, tile rows in sorted order of the tiles' names)"""
        return ([self.wells, self.umi_redundant, self.lone, self.families, self.molecules, self.distinct_umis,
                 self.split_families, self.split_wells, self.with_n, self.large, self.large_wells] + list(self.per_family) +
                list(self.sizes), [list(self.tiles[t]) for t in sorted(self.tiles)])

    @property
    def redundant_with_umi(self) -> int:
        """The redundant wells once the UMI is looked at: UmiRedundant, and the copies of the large families, which
        are counted as before."""
        return self.umi_redundant + self.large_wells - self.large

    @property
    def own_molecules(self) -> int:
        """The former "copies" that are molecules of their own: Molecules - Families."""
        return self.molecules - self.families

    def merged_rate(self) -> Optional[float]:
        """The UMI reads merged as read errors - DistinctUmis - Molecules - per UMI base of the gathered wells; None
        without one."""
        bases = self.wells * self.umi_cycles
        return (self.distinct_umis - self.molecules) / bases if bases else None


def write_lane_umi(lane, counts: LaneUmiCounts, verbose: bool = False, out=None) -> None:
    """The block that follows every other block of a lane under --lane-dups-umi: per-tile lines (verbose; tiles in
    sorted order as write_report), then the summary: the gathered and the large families, the lane's duplication as it
    was and with the UMI - its redundant wells UmiRedundant plus the copies of the large families, which are counted
    as before -, the library size from each (library_size), the share of the former copies that are molecules of
    their own, the UMI reads merged as read errors as a rate per UMI base, and the two histograms."""
    out = out or sys.stdout
    c = counts
    share = lambda v, of: v / of if of else 0.0
    size_text = lambda s: "n/a" if s is None else "%.0f" % s
    print(file=out)
    if verbose:
        for tile in sorted(c.tiles):
            t = c.tiles[tile]
            print("LaneUmi: %s\tTile: %s\tWells: %i\tUmiRedundant: %i\tLone: %i" % (lane, tile, t[0], t[1], t[2]), file=out)
    print("LaneUmiSummary: %s\tTiles: %i\tHamming: %i\tUmiCycles: %i\tMismatches: %i\tMaxFamily: %i\tFamilies: %i\tWells: %i "
          "(%.5f of PF)\tMolecules: %i\tDistinctUmis: %i\tUmiRedundant: %i\tLone: %i\tSplitFamilies: %i (%.5f of Families)\t"
          "SplitWells: %i\tWithN: %i\tLarge left out: %i (%i wells)" % (
              lane, len(c.tiles), c.k, c.umi_cycles, c.max_e, c.max_family, c.families, c.wells, share(c.wells, c.pf),
              c.molecules, c.distinct_umis, c.umi_redundant, c.lone, c.split_families, share(c.split_families, c.families),
              c.split_wells, c.with_n, c.large, c.large_wells), file=out)
    with_umi = c.redundant_with_umi
    print("Lane duplication (Redundant/PF wells): {:.2%}\twith the UMI: {:.2%} ({:d} redundant wells, {:d} before)".format(
        share(c.redundant, c.pf), share(with_umi, c.pf), with_umi, c.redundant), file=out)
    print("Estimated library size (distinct/X = 1 - exp(-PF/X)): %s\twith the UMI: %s" % (
        size_text(library_size(c.pf, c.pf - c.redundant)), size_text(library_size(c.pf, c.pf - with_umi))), file=out)
    copies = c.wells - c.families
    print("Copies that are molecules of their own: %i of %i (%.5f)" % (c.own_molecules, copies, share(c.own_molecules, copies)),
          file=out)
    rate = c.merged_rate()
    print("UMI reads merged as read errors: %i (%s per UMI base)" % (c.distinct_umis - c.molecules,
                                                                     "n/a" if rate is None else "%.3e" % rate), file=out)
    print("MoleculesPerFamily: %s" % "\t".join("%s: %i" % (n, v) for n, v in zip(LANE_UMI_BIN_NAMES, c.per_family)), file=out)
    print("MoleculeSizes: %s" % "\t".join("%s: %i" % (n, v) for n, v in zip(LANE_UMI_BIN_NAMES, c.sizes)), file=out)


def write_lane_umi_tsv(lane, counts: LaneUmiCounts, out, header: bool = True) -> None:
    """--lane-dups-umi-out: the two histograms and the tile rows - lane, table (per_family, size or tile), the bin or
    the tile's name, and three counts (a histogram's line holds its count and two zeros; a tile's Wells, UmiRedundant
    and Lone)."""
    if header:
        print("lane\ttable\tkey\twells\tumi_redundant\tlone", file=out)
    for table, values in (("per_family", counts.per_family), ("size", counts.sizes)):
        for name, v in zip(LANE_UMI_BIN_NAMES, values):
            print("%s\t%s\t%s\t%i\t0\t0" % (lane, table, name, v), file=out)
    for tile in sorted(counts.tiles):
        t = counts.tiles[tile]
        print("%s\ttile\t%s\t%i\t%i\t%i" % (lane, tile, t[0], t[1], t[2]), file=out)


LANE_KEEP_GAIN_NAMES = ("0", "1-9", "10-19", "20-49", "50-99", "100-199", "200-499", "500+")
LANE_KEEP_TILE_COLS = 6
LANE_KEEP_LANE_COLS = LANE_KEEP_TILE_COLS + 3 + len(LANE_KEEP_GAIN_NAMES)


@dataclass
class LaneKeepCounts:
    """The best well of each of a lane's families (include/welldup_lanekeep.h, LaneDups.keep): the lane row's columns,
    and per tile (by the tile's name) [PF, Kept, Dropped, MovedIn, SumKept, SumDropped]."""
    k: int = 0
    min_q: int = 15
    cycles: int = 0
    edges: List[int] = field(default_factory=lambda: [0])
    pf: int = 0
    kept: int = 0
    dropped: int = 0
    moved_in: int = 0
    sum_kept: int = 0
    sum_dropped: int = 0
    families: int = 0
    moved: int = 0
    sum_roots: int = 0
    gains: List[int] = field(default_factory=lambda: [0] * len(LANE_KEEP_GAIN_NAMES))
    tiles: Dict[str, List[int]] = field(default_factory=dict)
    by: Optional[str] = None                       # "molecule" under --lane-dups-keep-umi, "family" if said; None: not said

    @classmethod
    def from_rows(cls, lane_row: Sequence[int], tile_rows: Sequence[Sequence[int]], tile_names: Sequence, k: int,
                  min_q: int, edges: Sequence[int], cycles: int, by: Optional[str] = None) -> "LaneKeepCounts":
        """The two rows of LaneDups.keep(min_q); tile_names as LaneDupCounts.from_rows takes them; k: the K of
        --lane-dups-hamming; edges: the quality bins' lower edges; cycles: the scanned cycles; by: "molecule" for the
        rows of keep(by_molecule=True) (include/welldup_lanemolecules.h), whose "families" are UMI molecules of two or
        more wells."""
        b = [int(v) for v in lane_row]
        assert len(b) == LANE_KEEP_LANE_COLS and 0 <= min_q <= 63 and by in (None, "family", "molecule")
        tiles = {}
        for name, row in zip(tile_names, tile_rows):
            assert len(row) == LANE_KEEP_TILE_COLS
            if name is not None:
                tiles[name] = [int(v) for v in row]
        return cls(int(k), int(min_q), int(cycles), [int(e) for e in edges], *b[:9], b[9:], tiles, by)

    @property
    def weights(self) -> List[int]:
        """the weight of every bin: its lower edge from min_q on"""
        return [e if e >= self.min_q else 0 for e in self.edges]

    def per_base(self, total: int, wells: int) -> Optional[float]:
        """a summed score as a mean per base of `wells` wells; None without a base"""
        return total / (wells * self.cycles) if wells and self.cycles else None


def write_lane_keep(lane, counts: LaneKeepCounts, verbose: bool = False, out=None) -> None:
    """The block that follows every other block of a lane under --lane-dups-keep: per-tile lines (verbose; tiles in
    sorted order as write_report), then the summary - the kept and the dropped wells and their shares of PF, the
    families and those whose kept well is not their first well -, the mean score per base of the kept wells (the
    families' representatives and the single reads), of the first wells of the families and of the dropped wells, and
    the families by gain.  With counts.by the summary line ends in "By: family" or "By: molecule", and by molecule
    (--lane-dups-keep-umi) the block says molecules where it says families."""
    out = out or sys.stdout
    c = counts
    share = lambda v, of: v / of if of else 0.0
    num = lambda v: "n/a" if v is None else "%.3f" % v
    groups, of_groups = ("Molecules", "molecules") if c.by == "molecule" else ("Families", "families")
    print(file=out)
    if verbose:
        for tile in sorted(c.tiles):
            t = c.tiles[tile]
            print("LaneKeep: %s\tTile: %s\tPF: %i\tKept: %i\tDropped: %i (%.5f)\tMovedIn: %i\tMeanScore kept: %s\tdropped: %s" % (
                lane, tile, t[0], t[1], t[2], share(t[2], t[0]), t[3], num(c.per_base(t[4], t[1])),
                num(c.per_base(t[5], t[2]))), file=out)
    print("LaneKeepSummary: %s\tTiles: %i\tHamming: %i\tMinQ: %i\tCycles: %i\tWeights: %s\tPF: %i\tKept: %i (%.5f)\t"
          "Dropped: %i (%.5f)\t%s: %i\tMoved: %i (%.5f of %s)%s" % (
              lane, len(c.tiles), c.k, c.min_q, c.cycles, ",".join(str(w) for w in c.weights), c.pf, c.kept,
              share(c.kept, c.pf), c.dropped, share(c.dropped, c.pf), groups, c.families, c.moved, share(c.moved, c.families),
              groups, "\tBy: %s" % c.by if c.by else ""), file=out)
    print("Mean score per base\tkept wells: %s\tfirst wells of %s: %s\tdropped wells: %s" % (
        num(c.per_base(c.sum_kept, c.kept)), of_groups, num(c.per_base(c.sum_roots, c.families)),
        num(c.per_base(c.sum_dropped, c.dropped))), file=out)
    print("%sByGain: %s" % (groups, "\t".join("%s: %i" % (n, v) for n, v in zip(LANE_KEEP_GAIN_NAMES, c.gains))), file=out)
