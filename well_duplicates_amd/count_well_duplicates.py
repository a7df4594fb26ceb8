#!/usr/bin/env python3
"""count_well_duplicates on an MI355X: same CLI, targets-file format and report as the
reference's count_well_duplicates.py, with the per-tile gather + compare + tally
(count_well_duplicates.py:212-265, :63-106) running in libwelldup.so.

Flow per lane (the reference's unit of output, :207-269):
  read the scanned cycles' planes + filter of every tile (threads: gunzip releases the GIL)
  -> upload into an HBM-resident TileBatch -> one wd_count_tiles call for the whole batch
  -> per-tile integer blocks -> report.write_report (text identical to output_writer).
Unless -q is given the stderr log is reproduced too, including the three lines the
reference prints per duplicate (:258-262), from the device's hit list.

Multi-GPU: started under torchrun (one process per GPU) the flat list of (lane, tile) items is
block-partitioned over the ranks, each rank scans its share on its own GPU, ONE int64
all-reduce per run merges the per-tile counter rows (well_duplicates_amd/dist.py) and rank 0
prints the lanes in order - identical to the single-GPU output.

Differences from the reference, all deliberate:
  * a lane with valid targets but no duplicate prints 0.00 % instead of dying with
    ZeroDivisionError (F5); --strict restores the exception;
  * `-t` with a pattern that matches nothing raises the AssertionError the reference
    intends (its own message formatting raises NameError first);
  * extra flags: --device, --dist-backend, --tile-batch, --threads, --strict, -o/--output,
    --all-wells, --slocs, --layout, --serial-ingest, --dup-sets, --dup-sets-out, --tile-dups, --tile-dups-out,
    --tile-dups-hamming, --tile-dups-pair-budget, --lane-dups, --lane-dups-out,
    --lane-dups-hamming, --lane-dups-index, --lane-dups-mismatches, --lane-dups-distance, --lane-dups-quality,
    --lane-dups-saturation, --lane-dups-top, --lane-dups-top-out, --lane-dups-hops, --lane-dups-hops-mismatches,
    --lane-dups-hops-out, --lane-dups-gc, --lane-dups-gc-bins, --lane-dups-gc-max-n, --lane-dups-gc-out,
    --lane-dups-adapter, --lane-dups-adapter-mismatches, --lane-dups-adapter-min-overlap, --lane-dups-adapter-bins,
    --lane-dups-adapter-dimer, --lane-dups-adapter-out,
    --lane-dups-consensus, --lane-dups-consensus-max-d, --lane-dups-consensus-max-family, --lane-dups-consensus-out,
    --lane-dups-umi, --lane-dups-umi-mismatches, --lane-dups-umi-max-family, --lane-dups-umi-out,
    --lane-dups-keep, --lane-dups-keep-min-q, --lane-dups-keep-out, --lane-dups-keep-umi;
  * --all-wells --dup-sets groups every tile's wells into duplicate sets and follows each lane's report
    with their counts and the exact duplication (report.write_dup_sets);
  * --all-wells --tile-dups groups every tile's PF wells into classes of equal reads, wherever on the tile they
    lie, and follows each lane's report with the duplication of the tiles as a whole and the share of it
    that lies inside the rings (report.write_tile_dups); --tile-dups-hamming K adds the same for the clusters of
    reads within Hamming distance K of each other (report.write_tile_near_dups);
  * --all-wells --lane-dups groups the PF wells of a whole lane into classes of equal reads, on whatever tiles they
    lie (a LaneDups accumulator is fed every batch before its buffers are reused), and closes each lane's output
    with the duplication of the lane, split into the part within tiles and the part across tiles, and the
    library size it lets one estimate (report.write_lane_dups); --lane-dups-index RANGES groups the lane's PF wells
    by the bases of the index cycles as well - the libraries of a pooled lane - and adds the duplication and the
    library size of each, and the classes that span more than one index read (report.write_lane_index_dups);
    --lane-dups-mismatches (with --lane-dups-hamming) compares every redundant well with the first of its cluster
    and says how far apart the copies lie and at which cycles they differ (report.write_lane_mismatches);
    --lane-dups-distance holds every redundant well against the first of its class or cluster by where the two sit:
    on the same tile or not, how far apart, and how many closer than --lane-dups-distance-radius, the local copies
    that the library size should not count (report.write_lane_distances); --lane-dups-quality keeps the reported
    quality of every base beside the reads and counts the (copy, cycle) observations by the quality bins of the two
    wells, all of them and those where the bases differ: the error rate among copies per reported quality
    (report.write_lane_qualities); --lane-dups-saturation gives every PF well of the lane a pseudo-random step and
    counts, step by step, the reads and the distinct reads among them - the lane's saturation curve, exact, with the
    local copies of --lane-dups-saturation-radius left out: what the last reads still brought, whether the library
    size holds at half the depth, and what it projects for more reads (report.write_lane_saturation);
    --lane-dups-top N names the duplicates: the lane's duplication levels and its N largest classes (clusters under
    --lane-dups-hamming) with their spread over the tiles and the read itself (report.write_lane_top);
    --lane-dups-hops (with --lane-dups-index) holds the index read of every redundant well against that of the first
    of its class or cluster: read error or another index, in which index read, between which libraries, and into a
    listed library or an index combination nobody used (report.write_lane_hops);
    --lane-dups-gc holds the duplication against the molecule: every PF read by its GC content and by what it is in
    its class or cluster - the distinct molecules, the duplication, the mean family size and the library size per GC
    bin, over every PF read and without an alignment (report.write_lane_gc);
    --lane-dups-adapter NAME|SEQ holds the duplication against the insert length: every PF read by the position at
    which it runs into the adapter, with mismatches and with partial overlaps at its end - the share of adapter dimers,
    of reads that read through into the adapter, and the duplication of the short inserts against the rest
    (report.write_lane_adapter);
    --lane-dups-consensus lets every family of three or more wells vote: the base most of its members call at a cycle
    is the molecule's, a member that disagrees made the error - the lane's error profile by cycle and by direction,
    G>T apart from T>G, which the comparison with a first well cannot give (report.write_lane_consensus);
    --lane-dups-umi RANGES reads a unique molecular identifier at those cycles and splits every class or cluster by it:
    two wells with the same read and different UMIs are two molecules - the lane's duplication and library size with
    the UMI beside those without, the copies that are molecules of their own, and the UMI reads merged as read errors
    (report.write_lane_umi);
    --lane-dups-keep acts on all of it: of every class or cluster the well with the highest summed base quality is
    kept and the others are dropped (report.write_lane_keep), and --lane-dups-keep-out DIR writes the lane's .filter
    files with the PF bit cleared on the dropped wells - a deduplicated lane for every downstream converter; with
    --lane-dups-keep-umi (and --lane-dups-umi) one well is kept per UMI molecule, not per class or cluster;
  * the resident layout is chosen per run (--layout auto): sampled scans the interleaved-by-four layout
    serves (the reference's default -e 2 among them) keep their cycles interleaved, everything else planes.
"""
from __future__ import annotations

import math
import os
import sys
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

from . import bcl as bcl_direct_reader
from . import _lib, report, workload
from .lane_passes import (ALL_PASSES, DEFAULT_QUALITY_BINS, LANE_PASSES, check_cycle_ranges, check_options, dest,  # noqa: F401
                          parse_quality_bins, resolve_passes, write_keep_filter, write_lane_keep_filters)
from .report import LENGTH, TALLY, output_writer  # noqa: F401  (reference module surface)
from .scanner import INVALID_TARGET, LaneDups, Scanner, TileBatch, compare_mode
from .targets import load_targets, load_targets_csr

__VERSION__ = 0.3        # report format version of the reference this mirrors (:4)

HISEQ_4000 = workload.HISEQ_4000
HISEQ_X = workload.HISEQ_X
SEQUENCE = bcl_direct_reader.SEQUENCE
QUAL_FLAG = bcl_direct_reader.QUAL_FLAG


def parse_args(argv=None):
    """Same options as the reference (count_well_duplicates.py:272-317) plus device knobs."""
    description = """Assess well duplicates in a run without mapping. Reads within level l of
    selected reads from the coordinate file are compared with the centre read (edit distance,
    or Hamming distance with --hamming) on an AMD MI355X."""
    p = ArgumentParser(description=description, formatter_class=ArgumentDefaultsHelpFormatter)
    p.add_argument("-f", "--coord_file", dest="coord_file", required=False,
                   help="The file containing the random sample per tile (required unless --all-wells).")
    p.add_argument("-e", "--edit_distance", dest="edit_distance", type=int, default=2,
                   help="max edit distance between two reads to count as duplicate")
    p.add_argument("-n", "--sample_size", dest="sample_size", type=int, default=2500,
                   help="number of reads to be tested for well duplicates")
    p.add_argument("-l", "--level", dest="level", type=int, default=3,
                   help="levels around central spot to test")
    p.add_argument("-s", "--stype", dest="stype", required=True,
                   help="Sequencer model. Can be {} or {} or else the highest tile number in which "
                        "case the tile/swath configuration will be inferred.".format(HISEQ_4000, HISEQ_X))
    p.add_argument("-r", "--run", dest="run", required=True,
                   help="path to base of run, i.e /ifs/seqdata/150715_K00169_0016_BH3FGFBBXX")
    p.add_argument("-t", "--tile", dest="tile_id", type=str,
                   help="comma-separated list of specific tiles on a lane to analyse; each item "
                        "is a regex, so 1... is the top surface only.")
    p.add_argument("-i", "--lane", dest="lane", type=str,
                   help="comma-separated list of specific lanes to analyse, 1-8")
    p.add_argument("-x", "--start", dest="start", type=int, default=50,
                   help="Starting cycle/base position for the slice of read to be examined")
    p.add_argument("-y", "--end", dest="end", type=int, default=100,
                   help="Final cycle/base position for the slice of read to be examined")
    p.add_argument("--cycles",
                   help="Cycles/bases to scan as a list of ranges, eg. 10-50,100-120. Overrides -x/-y.")
    p.add_argument("--hamming", action="store_true",
                   help="Compare sequences using the Hamming distance rather than the "
                        "Levenshtein edit distance.")
    p.add_argument("-S", "--summary-only", action="store_true",
                   help="Only print the summary per lane, not for every tile")
    p.add_argument("-q", "--quiet", action="store_true", help="No log output")
    p.add_argument("--version", action="version", version=str(__VERSION__))
    p.add_argument("--device", type=int, default=None,
                   help="GPU to run on (default: LOCAL_RANK under torchrun, else 0)")
    p.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo", "wd"],
                   help="the one collective under torchrun: nccl = RCCL through torch.distributed; "
                        "wd = RCCL through libwelldup's own binding (wd_allreduce_counts; torch only carries "
                        "the unique id); gloo = CPU, for rehearsals")
    p.add_argument("--tile-batch", type=int, default=0,
                   help="tiles loaded, kept resident in HBM and scanned together (default 0: as many as make "
                        "about 512 files, what one launch of the GPU decoder holds at once)")
    p.add_argument("--threads", type=int, default=default_threads(),
                   help="reader threads (gunzip with --host-inflate)")
    p.add_argument("-o", "--output", default=None,
                   help="write the report to this file instead of stdout")
    p.add_argument("--all-wells", action="store_true",
                   help="every well of a tile is a centre (no sampling, no targets file): the rings of "
                        "-l levels are generated on the GPU from the run's s.locs with the rules of "
                        "prepare_cluster_indexes.py; the per-duplicate log is not written in this mode")
    p.add_argument("--slocs", default=None,
                   help="s.locs file for --all-wells (default: <run>/Data/Intensities/s.locs)")
    p.add_argument("--layout", default="auto", choices=["auto", "planes", "interleaved"],
                   help="how the scanned cycles sit in GPU memory: planes = one plane per cycle, as in the "
                        ".bcl.gz files; interleaved = the four cycles of a group side by side per well (the "
                        "loaders write it at no extra cost; the scan of sampled targets then touches half the "
                        "cache lines).  interleaved: -e <= 3 (any -e with --hamming up to 254), not "
                        "with --all-wells.  auto (default) = interleaved wherever that holds, else planes")
    p.add_argument("--host-inflate", action="store_true",
                   help="gunzip the .bcl.gz files on the host threads (the default inflates them on the GPU: "
                        "the threads only read the compressed files, one wave per file decodes it; files the "
                        "GPU decoder declines are gunzipped on the host either way)")
    p.add_argument("--serial-ingest", action="store_true",
                   help="load a batch of tiles only after the previous one has been scanned (for measuring "
                        "what the double-buffered ingest gains)")
    p.add_argument("--strict", action="store_true",
                   help="reproduce the reference's ZeroDivisionError on a lane without duplicates")
    p.add_argument("--dup-sets", action="store_true",
                   help="with --all-wells: group every tile's PF wells into duplicate sets (single linkage over "
                        "the duplicate pairs of levels <= l) and print, after each lane's report, the sets, the "
                        "wells in them, the redundant wells and the exact duplication (redundant / PF wells)")
    p.add_argument("--dup-sets-out", default=None, metavar="PATH",
                   help="with --dup-sets: write lane, tile, well and set (the smallest well index of its set) of "
                        "every well in a set of two or more to this TSV file (single process only)")
    p.add_argument("--tile-dups", action="store_true",
                   help="with --all-wells: group every tile's PF wells into classes of equal reads over the scanned "
                        "cycles, wherever on the tile they lie, and print, after each lane's report, the classes, the "
                        "wells in them, how many of those have a classmate within each level of rings, and the "
                        "duplication of the tile as a whole (redundant / PF wells).  The classes are always by "
                        "equality, whatever -e / --hamming the scan runs with: near-duplicate classes over a whole "
                        "tile are what --tile-dups-hamming adds")
    p.add_argument("--tile-dups-out", default=None, metavar="PATH",
                   help="with --tile-dups: write lane, tile, well and class (the smallest well index of its class) of "
                        "every well in a class of two or more to this TSV file (single process only)")
    p.add_argument("--tile-dups-hamming", type=int, default=None, metavar="K",
                   help="with --tile-dups: also group every tile's PF wells into clusters of reads linked by Hamming "
                        "distance <= K (1..%d; single linkage, exact, wherever on the tile the wells lie) and print a "
                        "second block of the same shape for them, with the pairs of distinct reads within K and the "
                        "tile-wide duplication at Hamming <= K beside the one by equality.  Hamming only: clusters "
                        "by edit distance over a whole tile are not offered (an insertion or deletion shifts "
                        "every later segment of the read)" % _lib.TILENEAR_MAX_K)
    p.add_argument("--tile-dups-pair-budget", type=int, default=0, metavar="N",
                   help="with --tile-dups-hamming: the most candidate pairs one segment of one tile may have before "
                        "the run is refused (reads of low diversity: amplicons, a shared adaptor); 0 = the "
                        "library's default, max(16 x wells, 2^24)")
    p.add_argument("--lane-dups", action="store_true",
                   help="with --all-wells: group the PF wells of every tile of a lane into classes of equal reads over "
                        "the scanned cycles, on whatever tiles they lie, and print, after each lane's report and its "
                        "other blocks, the classes, the redundant wells within tiles and across tiles, the duplication "
                        "of the lane (redundant / PF wells) and the library size estimated from it.  A packed copy of "
                        "every PF read of the lane stays in GPU memory until the lane is done: a lane that does not "
                        "fit is refused before anything is loaded (single process only)")
    p.add_argument("--lane-dups-out", default=None, metavar="PATH",
                   help="with --lane-dups: write lane, tile, well, class_tile and class_well (tile and well of the "
                        "first well of its class) of every well in a lane class to this TSV file")
    p.add_argument("--lane-dups-hamming", type=int, default=None, metavar="K",
                   help="with --lane-dups: also group the PF wells of every tile of a lane into clusters of reads "
                        "linked by Hamming distance <= K (1..%d; single linkage, exact, on whatever tiles the wells lie) "
                        "and print a second block of the same shape for them, with the pairs of distinct reads of the "
                        "lane within K, the duplication of the lane at Hamming <= K beside the one by equality and the "
                        "library size estimated from the clusters; --lane-dups-out then lists the wells in a lane "
                        "cluster, with cluster_tile and cluster_well columns.  Hamming only" % _lib.LANENEAR_MAX_K)
    p.add_argument("--lane-dups-pair-budget", type=int, default=0, metavar="N",
                   help="with --lane-dups-hamming: the most candidate pairs one segment of a lane may have before the "
                        "run is refused (reads of low diversity); 0 = the library's default, max(16 x the lane's "
                        "wells, 2^24)")
    p.add_argument("--lane-dups-index", default=None, metavar="RANGES",
                   help="with --lane-dups: the index cycles of the run, as --cycles takes them (eg. 151-159,159-167; "
                        "%d cycles at most).  The PF wells of a lane are grouped by the bases of these cycles - its "
                        "libraries, found without a sample sheet - and a third block gives, per library, its share "
                        "of the lane, the redundant wells inside it, the library size estimated from them and the wells "
                        "whose class reaches into another library; then the redundancy within and across libraries "
                        "and the classes that span more than one (index hopping, cross-contamination).  With "
                        "--lane-dups-hamming the block is computed on the clusters; --lane-dups-out gains an index "
                        "column" % _lib.LANEINDEX_MAX_CYCLES)
    p.add_argument("--lane-dups-index-min-share", type=float, default=0.001, metavar="F",
                   help="with --lane-dups-index: an index read is listed as a library when it holds at least this "
                        "share of the lane's PF wells, in (0, 1]; all others (reads with a sequencing error in the "
                        "index, mostly) are summed into one Other line")
    p.add_argument("--lane-dups-mismatches", action="store_true",
                   help="with --lane-dups-hamming K: compare every redundant well of a lane's clusters with the first "
                        "well of its cluster and print, after every other block of the lane, how many cycles apart the "
                        "copies lie (0..7, >= 8: mass in the last distance within K says K is too small, pairs far "
                        "beyond K that unrelated reads are being chained), the mismatches per pair, per scanned cycle "
                        "and per tile, and the substitutions with either direction summed.  Copies of one molecule "
                        "should be identical, so the cycles at which they differ are sequencing errors (no-calls where "
                        "a read has N): an error profile of the lane without a spike-in or an alignment.  The implied "
                        "rate per base, Mismatches / (2 x Profiled x cycles), assumes both copies carry errors alike "
                        "and is truncated from above: the clusters only link within K, so copies with more errors "
                        "are never compared")
    p.add_argument("--lane-dups-mismatches-max-d", type=int, default=None, metavar="D",
                   help="with --lane-dups-mismatches: only pairs at most D cycles apart (0..%d, default K) enter the "
                        "mismatch and substitution counts - a chain member far from the first well of its cluster is "
                        "probably another molecule; the distances themselves are counted for every pair"
                        % _lib.LANEMISMATCH_MAX_D)
    p.add_argument("--lane-dups-distance", action="store_true",
                   help="with --lane-dups: hold every redundant well of a lane against the first well of its class (of its "
                        "cluster with --lane-dups-hamming) by where the two sit, and print, after every other block of the "
                        "lane: the pairs on one tile and across tiles, the distances of the former in bins that double "
                        "from 32 units to 16 384 beside what uniformly placed copies would give (do the copies fall off "
                        "like a local process or lie flat like PCR copies?), the cross-tile pairs by where the other "
                        "tile lies, and the library size estimated without the local copies.  A well is paired with "
                        "the first well of its class, not with its nearest classmate: the block says which share of the "
                        "within-tile redundancy that covers")
    p.add_argument("--lane-dups-distance-radius", type=int, default=2500, metavar="R",
                   help="with --lane-dups-distance: a copy closer than R to the first well of its class on the same tile "
                        "is a local copy (0..%d).  R is in the units of the FASTQ header's coordinates, "
                        "int(10 x the s.locs position + 1000.5), the units of Picard's OPTICAL_DUPLICATE_PIXEL_DISTANCE, "
                        "whose documentation gives 2500 for patterned flowcells" % _lib.LANEDISTANCE_MAX_RADIUS)
    p.add_argument("--lane-dups-quality", action="store_true",
                   help="with --lane-dups: keep the reported quality (byte >> 2) of every base of a lane beside its "
                        "reads, hold every redundant well against the first well of its class (of its cluster with "
                        "--lane-dups-hamming K) cycle by cycle, and print, after every other block of the lane, a line per "
                        "quality bin: the raw values seen in it, its share of the lane's bases, of the first wells' and "
                        "of the copies', and the error rate observed among copies reported in that bin beside the "
                        "quality it amounts to - an empirical quality table of the run without an alignment.  The rates "
                        "are truncated from above (the clusters only link within K) and distinct molecules within K "
                        "inflate them; without --lane-dups-hamming every copy is identical and only the reported "
                        "qualities of the copies against the lane's are shown.  Doubles the device memory of a lane's "
                        "packed reads")
    p.add_argument("--lane-dups-quality-bins", default=None, metavar="E0,E1,..",
                   help="with --lane-dups-quality: the lower edges of 1..%d quality bins, ascending from 0, at most 63 "
                        "(default %s: no-call, then the ranges of the instruments' 8-level quality binning).  For an "
                        "instrument that reports a few quality levels give its levels: the bins are then exact - the "
                        "block prints the raw values seen in every bin, so a wrong choice shows"
                        % (_lib.LANEQUALITY_MAX_BINS, ",".join(str(e) for e in DEFAULT_QUALITY_BINS)))
    p.add_argument("--lane-dups-quality-max-d", type=int, default=None, metavar="D",
                   help="with --lane-dups-quality: only pairs at most D cycles apart enter the table (0..%d; default "
                        "--lane-dups-mismatches-max-d where --lane-dups-mismatches is given, else K)"
                        % _lib.LANEQUALITY_MAX_D)
    p.add_argument("--lane-dups-saturation", action="store_true",
                   help="with --lane-dups: give every PF well of a lane a pseudo-random step (a hash of the well's "
                        "number in the lane) and print, after every other block of the lane, a line per step: the reads "
                        "and the distinct reads (classes, or clusters with --lane-dups-hamming) among the wells up to "
                        "that step, their duplication, the library size they give and the new molecules per read of "
                        "the step - the lane's saturation curve, exact and without an alignment.  The closing lines "
                        "say what the last reads still brought (measured), how the library size at full depth compares "
                        "with the one at half depth (near 1: the estimate can be trusted; well above 1: the library is "
                        "uneven and the estimate a lower bound), and what the estimate projects for 2x and 4x the "
                        "reads.  Needs 4 bytes of device memory per well of the lane")
    p.add_argument("--lane-dups-saturation-steps", type=int, default=None, metavar="S",
                   help="with --lane-dups-saturation: the steps of the curve (1..%d, default 20)"
                        % _lib.LANESATURATION_MAX_STEPS)
    p.add_argument("--lane-dups-saturation-seed", type=int, default=None, metavar="SEED",
                   help="with --lane-dups-saturation: another seed (0..2^32 - 1, default 0) draws other subsamples; the "
                        "totals do not depend on it")
    p.add_argument("--lane-dups-saturation-radius", type=int, default=None, metavar="R",
                   help="with --lane-dups-saturation: leave out the copies closer than R to the first well of their class "
                        "on the same tile (0..%d, in the units of --lane-dups-distance-radius; 0: leave out none) - they "
                        "are made on the flowcell and say nothing about the library.  Default: "
                        "--lane-dups-distance-radius where --lane-dups-distance is given, else 0"
                        % _lib.LANESATURATION_MAX_RADIUS)
    p.add_argument("--lane-dups-top", type=int, default=None, metavar="N",
                   help="with --lane-dups: print, after every other block of the lane, the lane's duplication levels (the "
                        "groups and wells per class size: FastQC's two curves, exact and over every PF read) and its N "
                        "(1..%d) largest classes (clusters with --lane-dups-hamming): size, share of the PF reads, "
                        "where the first well lies, the tiles touched, the read itself and a note - poly-A/C/G/T, all "
                        "N, N-rich, one tile - that tells a contaminant from a large PCR family"
                        % _lib.LANETOP_MAX)
    p.add_argument("--lane-dups-top-out", default=None, metavar="FILE",
                   help="with --lane-dups-top: also write the listed groups to FILE, tab-separated: lane, rank, size, "
                        "exact, tiles, root_tile, root_well, read, then a tile=count column per tile touched")
    p.add_argument("--lane-dups-hops", type=int, nargs="?", const=10, default=None, metavar="N",
                   help="with --lane-dups-index: hold the index read of every redundant well of a lane against that of "
                        "the first well of its class (of its cluster with --lane-dups-hamming) and print, after every "
                        "other block of the lane: the pairs by what became of each of the two index reads - the same, "
                        "a read error (at most --lane-dups-hops-mismatches cycles differ: what a demultiplexer forgives) "
                        "or another index -, per listed library the pairs inside it and those it exchanged with "
                        "another, the N (default 10) library pairs that exchanged most beside what random index hopping "
                        "would give them, and how many swapped copies land in a listed library and how many in an "
                        "index combination nobody used.  The first range of --lane-dups-index is the first index read "
                        "(i7), the rest the second; one range is a single index.  The libraries are the first %d that "
                        "--lane-dups-index lists" % _lib.LANEHOPS_MAX_LISTED)
    p.add_argument("--lane-dups-hops-mismatches", type=int, default=None, metavar="E",
                   help="with --lane-dups-hops: an index read that differs from the first well's in at most E cycles "
                        "(0..%d, default 1) is a read error, one that differs in more another index"
                        % _lib.LANEHOPS_MAX_E)
    p.add_argument("--lane-dups-hops-out", default=None, metavar="FILE",
                   help="with --lane-dups-hops: also write every cell of the library matrix that is not zero to FILE, "
                        "tab-separated: lane, index_a (the first well's), index_b (the copy's), pairs")
    p.add_argument("--lane-dups-gc", action="store_true",
                   help="with --lane-dups: count every PF read of a lane by its GC content - the cycles that read C or "
                        "G - and by what it is in its class (its cluster with --lane-dups-hamming): a lone read, the "
                        "first well or a copy, and print, after every other block of the lane, per GC bin the distinct "
                        "molecules, the reads and the redundant wells by the molecule's GC, the duplication in the bin "
                        "and against the lane's, the mean family size, the copies by their own read and the library "
                        "size; then the mean GC of the distinct molecules and of the redundant wells and the "
                        "duplication below, between and above the quartiles of GC: whether GC-poor or GC-rich "
                        "fragments were over-amplified")
    p.add_argument("--lane-dups-gc-bins", type=int, default=None, metavar="B",
                   help="with --lane-dups-gc: the GC bins printed, %d..%d (default 20); the bin of a read with g cycles "
                        "of C or G among L is min(B - 1, g * B // L)" % (report.LANE_GC_MIN_BINS, report.LANE_GC_MAX_BINS))
    p.add_argument("--lane-dups-gc-max-n", type=int, default=None, metavar="M",
                   help="with --lane-dups-gc: a read with more than M no-calls (0..the scanned cycles, default 0, so "
                        "that a read's GC fraction is exactly g / L) is counted by what it is but kept out of the bins")
    p.add_argument("--lane-dups-gc-out", default=None, metavar="FILE",
                   help="with --lane-dups-gc: also write a line per g to FILE, tab-separated: lane, gc, single, roots, "
                        "copies, family_wells")
    p.add_argument("--lane-dups-adapter", default=None, metavar="NAME|SEQ",
                   help="with --lane-dups: search every PF read of a lane for the adapter - truseq (AGATCGGAAGAGC), "
                        "nextera (CTGTCTCTTATACACATCT), smallrna (TGGAATTCTCGG), or 8..32 letters of ACGT - at every "
                        "position, and count the read by the first position that matches (its insert length when "
                        "--cycles starts at the read's first cycle) and by what it is in its class (its cluster with "
                        "--lane-dups-hamming); print, after the GC block, per bin of insert length and for the reads "
                        "without adapter the distinct molecules, the reads, the duplication in the bin and against the "
                        "lane's, the mean family size and the library size; then the share of reads with adapter and "
                        "of adapter dimers and the duplication of dimers, of the other reads with adapter and of the "
                        "reads without.  The scanned cycles must be one run of consecutive cycles")
    p.add_argument("--lane-dups-adapter-mismatches", type=int, default=None, metavar="E",
                   help="with --lane-dups-adapter: the mismatches allowed where the whole adapter fits, 0..3 (default "
                        "1); where only o of its m bases fit before the read's end, floor(E * o / m)")
    p.add_argument("--lane-dups-adapter-min-overlap", type=int, default=None, metavar="O",
                   help="with --lane-dups-adapter: the fewest bases of the adapter that count as a match at the read's "
                        "end, 3..the adapter's length (default 8, or the adapter's length if that is less)")
    p.add_argument("--lane-dups-adapter-bins", type=int, default=None, metavar="B",
                   help="with --lane-dups-adapter: the bins of insert length printed, %d..%d (default 10), of equal "
                        "width over the scanned cycles: the bin of position a among L is min(B - 1, a * B // L)"
                        % (report.LANE_ADAPTER_MIN_BINS, report.LANE_ADAPTER_MAX_BINS))
    p.add_argument("--lane-dups-adapter-dimer", type=int, default=None, metavar="D",
                   help="with --lane-dups-adapter: a read whose adapter begins at position D or before it is an adapter "
                        "dimer (default 10)")
    p.add_argument("--lane-dups-adapter-out", default=None, metavar="FILE",
                   help="with --lane-dups-adapter: also write a line per position to FILE, tab-separated: lane, insert, "
                        "single, roots, copies, family_wells, cumulative (the share of PF reads whose adapter begins at "
                        "or before the position: the adapter content curve, exact)")
    p.add_argument("--lane-dups-consensus", action="store_true",
                   help="with --lane-dups: gather the wells of every class (every cluster with --lane-dups-hamming K) of "
                        "three or more wells, take the base that more than half of them call at a cycle for the "
                        "molecule's, and print, after every other block of the lane: the families that voted, the "
                        "errors per called base and the quality that amounts to, the families whose first well "
                        "disagrees with the vote, the distances of the wells from their family's consensus and the "
                        "twelve substitutions molecule>call with each direction's rate and its ratio to the reverse "
                        "direction - which --lane-dups-mismatches, comparing with a first well, cannot tell apart.  "
                        "Without --lane-dups-hamming every copy is identical: no well disagrees, and only the families "
                        "and the calls per consensus base are shown.  Takes 8 bytes of device memory per well of the lane")
    p.add_argument("--lane-dups-consensus-max-d", type=int, default=None, metavar="D",
                   help="with --lane-dups-consensus: a well further than D (0..%d) from its family's consensus is "
                        "counted by its distance but kept out of the substitutions (default: the D of "
                        "--lane-dups-mismatches, else K)" % _lib.LANECONSENSUS_MAX_D)
    p.add_argument("--lane-dups-consensus-max-family", type=int, default=None, metavar="M",
                   help="with --lane-dups-consensus: a family of more than M wells (3..%d, default 256) is a contaminant "
                        "- poly-G, an adapter dimer: what --lane-dups-top names -, not a molecule: it is counted and "
                        "left out of the vote" % _lib.LANECONSENSUS_MAX_FAMILY)
    p.add_argument("--lane-dups-consensus-out", default=None, metavar="FILE",
                   help="with --lane-dups-consensus: also write every cell of the call matrix that is not zero to FILE, "
                        "tab-separated: lane, cycle, consensus, call, count")
    p.add_argument("--lane-dups-umi", default=None, metavar="RANGES",
                   help="with --lane-dups: the cycles of a unique molecular identifier (UMI), given as --lane-dups-index "
                        "takes its cycles, 1..%d in all, among the scanned cycles or not.  The wells of every class "
                        "(every cluster with --lane-dups-hamming K) are grouped by their UMI read: two wells with the "
                        "same read and different UMIs are two molecules, not copies.  Printed after every other block of "
                        "the lane: the families looked into and those left out, the lane's duplication and library size "
                        "as they were and with the UMI, the share of the copies that are molecules of their own, the UMI "
                        "reads merged as read errors, and the families by their molecules and the molecules by their "
                        "wells.  Takes 16 bytes of device memory per well of the lane: 8 for the UMI reads, 8 for the "
                        "pass" % _lib.LANEUMI_MAX_CYCLES)
    p.add_argument("--lane-dups-umi-mismatches", type=int, default=None, metavar="E",
                   help="with --lane-dups-umi: two UMI reads of a family that differ at up to E cycles (0..%d, default 1) "
                        "are one molecule read with an error; molecules are the connected components under that rule "
                        "(single linkage).  0: only equal UMI reads are one molecule" % _lib.LANEUMI_MAX_E)
    p.add_argument("--lane-dups-umi-max-family", type=int, default=None, metavar="M",
                   help="with --lane-dups-umi: a family of more than M wells (2..%d, default 256) is counted and not "
                        "looked into: its copies stay copies" % _lib.LANEUMI_MAX_FAMILY)
    p.add_argument("--lane-dups-umi-out", default=None, metavar="FILE",
                   help="with --lane-dups-umi: also write the two histograms and the tile rows to FILE, tab-separated: "
                        "lane, table, key, wells, umi_redundant, lone")
    p.add_argument("--lane-dups-keep", action="store_true",
                   help="with --lane-dups: of every class (every cluster with --lane-dups-hamming K) keep the well with "
                        "the highest sum of reported base qualities at or above --lane-dups-keep-min-q - the choice of "
                        "Picard's MarkDuplicates; the first well among equals - and drop the others, and print, after "
                        "every other block of the lane, the kept and the dropped wells, the families whose kept well is "
                        "not their first well, the mean score per base of the kept, the first and the dropped wells, and "
                        "the families by what the choice gained.  A quality counts as the lower edge of its bin "
                        "(--lane-dups-quality-bins): exact where the edges are the instrument's levels, a lower bound "
                        "otherwise.  Keeps the reported qualities beside the reads as --lane-dups-quality does (given or "
                        "not) and takes 10 bytes of device memory per well of the lane besides.  One well per UMI "
                        "molecule instead of per family: --lane-dups-keep-umi")
    p.add_argument("--lane-dups-keep-umi", action="store_true",
                   help="with --lane-dups-keep and --lane-dups-umi: keep one well per UMI molecule, not per family - the "
                        "best well of every molecule the --lane-dups-umi block counts (at its --lane-dups-umi-mismatches "
                        "and --lane-dups-umi-max-family; a family above max-family stays one molecule), so that a well the "
                        "UMI shows to be a molecule of its own is not dropped.  The keep block and the "
                        "--lane-dups-keep-out files are then per molecule, and the summary line ends in By: molecule.  "
                        "Takes 8 bytes of device memory per well of the lane besides")
    p.add_argument("--lane-dups-keep-min-q", type=int, default=None, metavar="Q",
                   help="with --lane-dups-keep: a base counts from quality Q on (0..%d, default %d)"
                        % (_lib.LANEKEEP_MAX_Q, _lib.LANEKEEP_DEFAULT_MIN_Q))
    p.add_argument("--lane-dups-keep-out", default=None, metavar="DIR",
                   help="with --lane-dups-keep: for every scanned tile write DIR/L00<lane>/<the name of the tile's .filter "
                        "file>, the tile's filter file with the PF bit cleared on every dropped well.  Put in place of "
                        "the run directory's own files they make bcl2fastq or BCL Convert emit the deduplicated lane")
    args = p.parse_args(argv)
    check_options(args, p.error)                # the passes after a lane's finish: lane_passes.ALL_PASSES
    if not args.coord_file and not args.all_wells:
        p.error("the following arguments are required: -f/--coord_file (or --all-wells)")
    if args.layout == "interleaved" and (args.all_wells or (args.edit_distance > 3 and not args.hamming)):
        p.error("--layout interleaved needs sampled targets (-f) and, for the edit distance, -e <= 3")
    if args.dup_sets and not args.all_wells:
        p.error("--dup-sets needs --all-wells (with sampled targets the pairs only leave the centres)")
    if args.dup_sets_out and not args.dup_sets:
        p.error("--dup-sets-out needs --dup-sets")
    if args.dup_sets_out and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        p.error("--dup-sets-out is written by a single process only")
    if args.tile_dups and not args.all_wells:
        p.error("--tile-dups needs --all-wells (the rings of every well say which classmates are local)")
    if args.tile_dups_out and not args.tile_dups:
        p.error("--tile-dups-out needs --tile-dups")
    if args.tile_dups_out and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        p.error("--tile-dups-out is written by a single process only")
    if args.tile_dups_hamming is not None and not args.tile_dups:
        p.error("--tile-dups-hamming needs --tile-dups")
    if args.tile_dups_hamming is not None and not 1 <= args.tile_dups_hamming <= _lib.TILENEAR_MAX_K:
        p.error("--tile-dups-hamming takes 1..%d" % _lib.TILENEAR_MAX_K)
    if args.tile_dups_pair_budget < 0:
        p.error("--tile-dups-pair-budget must not be negative")
    if args.tile_dups_pair_budget and args.tile_dups_hamming is None:
        p.error("--tile-dups-pair-budget needs --tile-dups-hamming")
    if args.lane_dups and not args.all_wells:
        p.error("--lane-dups needs --all-wells (the resident layout of every well, a plane per cycle)")
    if args.lane_dups_out and not args.lane_dups:
        p.error("--lane-dups-out needs --lane-dups")
    if args.lane_dups_hamming is not None and not args.lane_dups:
        p.error("--lane-dups-hamming needs --lane-dups")
    if args.lane_dups_hamming is not None and not 1 <= args.lane_dups_hamming <= _lib.LANENEAR_MAX_K:
        p.error("--lane-dups-hamming takes 1..%d" % _lib.LANENEAR_MAX_K)
    if args.lane_dups_pair_budget < 0:
        p.error("--lane-dups-pair-budget must not be negative")
    if args.lane_dups_pair_budget and args.lane_dups_hamming is None:
        p.error("--lane-dups-pair-budget needs --lane-dups-hamming")
    if args.lane_dups_index is not None and not args.lane_dups:
        p.error("--lane-dups-index needs --lane-dups")
    if args.lane_dups_index is not None:
        check_cycle_ranges(p.error, "--lane-dups-index", args.lane_dups_index, "151-159,159-167",
                           _lib.LANEINDEX_MAX_CYCLES)
    if not 0.0 < args.lane_dups_index_min_share <= 1.0:
        p.error("--lane-dups-index-min-share takes a share in (0, 1], not %g" % args.lane_dups_index_min_share)
    if args.lane_dups and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        p.error("--lane-dups runs in a single process only: under WORLD_SIZE > 1 a lane's tiles are spread over the "
                "ranks, and the classes of a lane need all of them in one GPU's table")
    return args


_T0 = [0.0]


def default_threads() -> int:
    """Reader threads (they read files into pinned memory; with --host-inflate they also gunzip):
    at most 32, and under torchrun this rank's share of the host's CPUs - eight ranks of one node
    read through one page cache and must not start 8 x 32 threads."""
    cpus = os.cpu_count() or 1
    try:
        cpus = len(os.sched_getaffinity(0)) or cpus
    except (AttributeError, OSError):
        pass
    local_world = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1") or 1))
    return max(1, min(32, cpus // local_world))


def resident_layout(args, mode, k, csr, reader, lanes, tiles, cycle_list) -> int:
    """--layout -> the well stride of the batches (1 = a plane per cycle, 4 = interleaved by four).  `auto`
    takes the interleaved layout wherever the kernels that read it serve the run: sampled targets of at most
    508 neighbour slots, equality / Hamming <= 254 / Levenshtein <= 3 (the reference's default is 2:
    count_well_duplicates.py:282-283); .bcl.gz files and the .cbcl blocks of a NovaSeq run are both written
    straight into it by the loaders."""
    from .scanner import MODE_EQ, MODE_HAMMING
    if args.layout != "auto":
        return 4 if args.layout == "interleaved" else 1
    if args.all_wells or csr is None:
        return 1
    served = mode == MODE_EQ or (mode == MODE_HAMMING and k <= 254) or (mode not in (MODE_EQ, MODE_HAMMING) and k <= 3)
    lvl_off = csr[1]
    slots = int((lvl_off[:, -1] - lvl_off[:, 0]).max()) if lvl_off.shape[0] else 0
    if not served or slots > 508 or not cycle_list or lvl_off.shape[0] >= 65536:      # (65536 targets: the dense path, on planes)
        return 1
    return 4


def _lap(what: str):
    """WD_CLI_TIMING=1: where the wall clock of a run goes (stderr)."""
    if os.environ.get("WD_CLI_TIMING"):
        import time
        now = time.perf_counter()
        print("[wd timing] %-28s %7.1f ms" % (what, (now - _T0[0]) * 1e3), file=sys.stderr)
        _T0[0] = now


def _decode(seq_bytes: np.ndarray) -> str:
    """BCL bytes of one well over the scanned cycles -> the reference's string."""
    lut = np.frombuffer(b"NACGT", dtype="S1")
    return lut[np.where(seq_bytes == 0, 0, (seq_bytes & 3) + 1)].tobytes().decode()


def _decode_rows(rows: np.ndarray):
    """[n, L] BCL bytes -> n strings."""
    lut = np.frombuffer(b"NACGT", dtype="S1")
    codes = lut[np.where(rows == 0, 0, (rows & 3) + 1)]
    return [r.tobytes().decode() for r in codes]


class _Loading:
    """One batch of tiles on its way into HBM: the TileBatch and the loader pool's futures."""

    def __init__(self, chunk, handles, tb, futures, error=None):
        self.chunk, self.handles, self.tb, self.futures = chunk, handles, tb, futures
        self.error = error                  # what submitting the batch raised (a missing lane directory, ...)

    def wait(self):
        if self.error is not None:
            raise self.error
        for f in self.futures:
            f.result()                      # re-raises the loader's exception (FileNotFoundError, ...)


def set_members(labels: np.ndarray):
    """One tile's labels (wd_dup_sets) -> (wells, set labels) of the wells in sets of two or more, by well."""
    valid = labels != INVALID_TARGET
    size = np.bincount(labels[valid].astype(np.int64), minlength=labels.shape[0])
    member = np.zeros(labels.shape[0], dtype=bool)
    member[valid] = size[labels[valid].astype(np.int64)] >= 2
    wells = np.flatnonzero(member)
    return wells, labels[wells]


def lane_members(labels: np.ndarray):
    """A lane's labels [tiles, N] (LaneDups.finish) -> (tile index, well, class tile index, class well) of the
    wells in a lane class, by tile index and well."""
    n = labels.shape[1]
    flat = labels.reshape(-1)
    ids = np.flatnonzero(flat != INVALID_TARGET)
    lab = flat[ids].astype(np.int64)
    size = np.bincount(lab, minlength=flat.shape[0])
    keep = size[lab] >= 2
    ids, lab = ids[keep], lab[keep]
    return ids // n, ids % n, lab // n, lab % n


def lane_cluster_members(class_labels: np.ndarray, cluster_labels: np.ndarray):
    """A lane's class and cluster labels [tiles, N] (LaneDups.finish(hamming=K)) -> (tile index, well, class tile
    index, class well, cluster tile index, cluster well) of the wells in a lane cluster, by tile index and well."""
    ti, w, cti, cw = lane_members(cluster_labels)
    lab = class_labels.reshape(-1)[ti * class_labels.shape[1] + w].astype(np.int64)
    return ti, w, lab // class_labels.shape[1], lab % class_labels.shape[1], cti, cw


# check_lane_dups_fits' keywords and the flag each is reported under, in the order of the message's clauses: the
# label stage's two, then every pass's own (keywords of one flag make one clause)
_FIT_CLAUSES = (("scratch", "--lane-dups-hamming"), ("index", "--lane-dups-index")) + \
    tuple(clause for p in ALL_PASSES for clause in p.fit)


def check_lane_dups_fits(need: int, free: int, tiles: int, wells: int, cycles: int, **parts):
    """--lane-dups: the accumulator's workspace plus `parts`, the device bytes by _FIT_CLAUSES' keywords - scratch: the
    near finish; index: the index workspace; a pass's own: its scratch and the part of the accumulator it asks for
    (LanePass.bytes) - against the free device memory, before anything is loaded."""
    unknown = set(parts) - {keyword for keyword, _ in _FIT_CLAUSES}
    if unknown:
        raise TypeError("check_lane_dups_fits() got an unexpected keyword argument %r" % sorted(unknown)[0])
    by_flag = {}
    for keyword, flag in _FIT_CLAUSES:
        by_flag[flag] = by_flag.get(flag, 0) + parts.get(keyword, 0)
    need += sum(by_flag.values())
    if need > free:
        raise MemoryError("--lane-dups needs %.2f GB of device memory for a lane of %d tiles x %d wells x %d cycles "
                          "(%d bytes%s), and %.2f GB (%d bytes) are free" % (
                              need / 1e9, tiles, wells, cycles, need,
                              "".join(", %d of them for %s" % (b, flag) for flag, b in by_flag.items() if b),
                              free / 1e9, free))


def index_listing(min_share: float, pf: int):
    """--lane-dups-index-min-share F and a lane's PF wells -> (min_pf, cap) of LaneDups.index_finish: a group is
    listed from ceil(F x PF) wells on, and no more than floor(1 / F) groups can each hold a share F of the reads."""
    return max(1, int(math.ceil(min_share * pf))), int(math.floor(1.0 / min_share)) + 1


def scan_lanes(sc: Scanner, reader, lane_tiles, cycle_list, mode, k, csr, wells, tile_batch,
               threads, want_log, overlap=True, interleave=1, gpu_inflate=True, lane_done=None, into=None,
               dup_sets=0, tile_dups=0, tile_near=0, pair_budget=0, lane_dups=0, lane_near=0, lane_pair_budget=0,
               lane_index=None, lane_passes=()):
    """lane_tiles: [(lane, [tiles])] in the order they are reported -> ({(lane, tile): TileCounts},
    {(lane, tile): [log lines]}); `lane_done(lane)` is called when a lane's last tile has been scanned.
    dup_sets (needs `into`): 1 = the duplicate sets of every tile too (into["sets"][(lane, tile)] = DupSetCounts),
    2 = and their members (into["members"][(lane, tile)] = (wells, labels), set_members).
    tile_dups (needs `into`): the same for the read classes of every tile (TileBatch.tile_dups), run on the resident
    batch after the scan: into["tdups"][(lane, tile)] = TileDupCounts, into["tmembers"][(lane, tile)].
    tile_near = K > 0 (with tile_dups): and the clusters at Hamming distance <= K (TileBatch.tile_near_dups):
    into["tnear"][(lane, tile)] = TileNearCounts, into["tnmembers"][(lane, tile)] = (wells, classes, clusters).
    lane_dups (needs `into`, batches a plane per cycle): the read classes of every lane as a whole - a LaneDups
    accumulator is begun at a lane's first batch, fed every batch after its scan and before its buffers are
    released, and finished at the lane's last batch: into["ldups"][lane] = LaneDupCounts; 2 = and the members,
    into["lmembers"][lane] = (tile names by index,) + lane_members(labels).  A tile index is the tile's place
    in the lane's list.
    lane_near = K > 0 (with lane_dups): and the lane's clusters at Hamming distance <= K (LaneDups.finish(hamming=K)):
    into["lnear"][lane] = LaneNearCounts, and into["lmembers"][lane] = (names,) + lane_cluster_members(...).
    lane_index = (index cycles, cycles per index range, min share) (with lane_dups): every batch gets a second
    TileBatch of the index cycles, whose files are appended to the batch's job list - one call loads both, through
    the GPU decoder and the .cbcl path alike - and which is fed to LaneDups.index_add, reused and released with the
    scan batch; after the lane's finish into["lindex"][lane] = LaneIndexCounts (on the clusters under lane_near), and
    with the members into["lmindex"][lane] = the index read of every row of into["lmembers"][lane].
    lane_passes = [(LanePass, params)] (lane_passes.resolve_passes; with lane_dups): after the lane's finish, and after
    its index finish, every pass runs in the list's order on the labels the lane was left with:
    into[pass.key][lane] = pass.run(the accumulator, the lane's context, params).  The parts of the accumulator that
    are fed batch by batch - the qualities beside the reads, a further TileBatch of UMI cycles - are there when a
    pass of the list asks for them (LanePass.parts).  What each pass takes and does stands with its entry.

    Pipelined: while the GPU scans batch n (and its report rows and log lines are put together),
    batch n + 1 is being inflated and batch n + 2 read and copied, each into a TileBatch of its own
    (the ctypes calls release the GIL).  A batch holds tiles of one lane, but the pipeline runs on from
    one lane into the next: the first batches of lane n + 1 are on their way while the last ones of lane
    n are decoded and scanned (a lane at a time, every lane paid for the fill and the drain of its own
    pipeline: a tenth of a second of a 0.43 s lane).  Whatever goes wrong, every loader thread has
    finished before a TileBatch is freed or the exception leaves this function: the threads
    write through the scanner's copy streams into the batches' planes.
    """
    centre, lvl_off, nbr = csr
    levels = lvl_off.shape[1] - 1
    index_cycles, index_lengths, index_share = lane_index if lane_index else ([], [], 1.0)
    assert not index_cycles or (lane_dups and interleave == 1)
    # the side cycle sets: each gets a further TileBatch per scan batch, loaded by the batch's job list, fed to
    # LaneDups.<name>_add, reused and released with the scan batch (tb: id(scan batch) -> its side batch; spare: finished
    # ones).  The index cycles belong to the label stage; the others, and the quality part, are asked for by passes
    side = lambda name, cycles: SimpleNamespace(name=name, cycles=cycles, tb={}, spare=[])      # noqa: E731
    sides = [side("index", index_cycles)] if index_cycles else []
    qual_edges = None
    for p, params in lane_passes:
        parts = p.parts(params)
        qual_edges = parts.get("quality") if qual_edges is None else qual_edges
        sides += [side(name, cycles) for name, cycles in parts.get("sides", {}).items()]
    assert not sides or (lane_dups and interleave == 1)
    begins = [(s.name, len(s.cycles)) for s in sides]       # LaneDups.<name>_begin(argument), in this order:
    if qual_edges is not None:
        begins.insert(bool(index_cycles), ("qual", qual_edges))     # the index, the qualities, the passes' sides
    counts, logs = (into["counts"], into["logs"]) if into else ({}, {})
    batches = []                            # (lane, [tiles]), never across a lane's end: an error stays its lane's (start_ahead)
    for lane, tiles in lane_tiles:
        if not tiles:
            continue
        tb_n = tile_batch
        if tb_n <= 0:
            # as many files per batch as one launch of the GPU decoder holds at once - 512, or 768 of files
            # that expand less than 1.75-fold (its small-window form; base calls with binned qualities do:
            # the first file's size tells) - in batches of equal size (a short last batch would cost a full
            # round of the decoder all the same)
            room = 512
            try:
                first = reader.get_tile(lane, tiles[0])
                if os.path.getsize(first.plane_path(cycle_list[0])) * 7 >= (first.num_clusters + 4) * 4:
                    room = 700
            except (OSError, IndexError, RuntimeError, AssertionError):
                pass                            # (whatever is wrong with the first tile is reported when it is loaded)
            per = max(1, room // max(1, len(cycle_list) + sum(len(s.cycles) for s in sides) + 1))
            n_batches = max(1, -(-len(tiles) // per))
            tb_n = max(1, -(-len(tiles) // n_batches))
        batches += [(lane, tiles[b0:b0 + tb_n]) for b0 in range(0, len(tiles), tb_n)]
    last_batch_of = {lane: bi for bi, (lane, _) in enumerate(batches)}
    pool = ThreadPoolExecutor(max_workers=max(1, threads))
    live = []                               # TileBatches not yet freed
    lane_acc = {"ld": None, "lane": None}   # the LaneDups of the lane being scanned
    tiles_of_lane = {lane: list(tiles) for lane, tiles in lane_tiles}
    spare = []                              # finished ones whose buffers the next batch takes over

    def start(batch):
        """Submit every load of a batch; returns at once."""
        lane, chunk = batch
        handles = [reader.get_tile(lane, t) for t in chunk]
        n_clusters = handles[0].num_clusters
        for h in handles:
            # one targets file, hence one geometry, per flowcell (README.md:14)
            if h.num_clusters != n_clusters:
                raise RuntimeError("tiles of one batch differ in cluster count")
        if wells.size and (wells[-1] >= n_clusters or wells[0] < 0):
            raise IndexError("Requested cluster %i is out of range.  Highest on this "
                             "tile is %i." % (int(wells[-1]), n_clusters - 1))
        # (a finished batch's buffers are taken over: freeing device memory would wait for the
        # decoder's kernels of the batches behind)
        tb = TileBatch(sc, len(chunk), len(cycle_list), n_clusters, interleave=interleave,
                       reuse=spare.pop() if spare else None)
        live.append(tb)
        for s in sides:
            s.tb[id(tb)] = TileBatch(sc, len(chunk), len(s.cycles), n_clusters, reuse=s.spare.pop() if s.spare else None)
        _lap("  batch of %d tiles: buffers" % len(chunk))
        # ingest: every (tile, cycle) file is gunzipped into pinned memory and copied to the GPU
        # by libwelldup (wd_load_bcl_gz).  Runs without .bcl.gz files are NovaSeq runs: the
        # tile's block of the lane/surface .cbcl is gunzipped on the host and expanded on the
        # GPU (wd_load_cbcl_tile), which needs the tile's filter first.
        # a job: (slot, cycle, where its plane goes); the planes of the side cycles go to batches of their own
        jobs = [(i, cycle_list[c], tb.plane_ptr(i, c)) for i in range(len(handles)) for c in range(len(cycle_list))]
        for s in sides:
            stb = s.tb[id(tb)]
            jobs += [(i, cyc, stb.plane_ptr(i, c)) for i in range(len(handles)) for c, cyc in enumerate(s.cycles)]
        batch = None                        # which files the GPU decoder gets as one batch
        if gpu_inflate and jobs:
            if os.path.exists(handles[0].plane_path(cycle_list[0])):
                batch = "bcl.gz"
            elif os.path.exists(handles[0].cbcl_path(cycle_list[0])):
                batch = "cbcl"
        # (in a batch the filters travel with the planes, below)
        filt = [] if batch else [pool.submit(sc.load_filter, h.filter_file, tb.filter_ptr(i), n_clusters)
                                 for i, h in enumerate(handles)]

        def load(i, cyc, dst):
            try:
                sc.load_bcl_gz(handles[i].plane_path(cyc), dst, n_clusters, interleave)
            except FileNotFoundError:       # only a missing file: a corrupt one is reported as such
                if filt:
                    filt[i].result()
                sc.load_cbcl_tile(handles[i].cbcl_path(cyc), int(handles[i].tile),
                                  tb.filter_ptr(i), n_clusters, dst, interleave)
        if batch == "cbcl":
            # NovaSeq: the filters first (the expansion of a tile's blocks needs its filter in HBM),
            # then every (tile, cycle) block of the batch through one launch of the GPU decoder
            def load_all():
                sc.load_bcl_gz_batch([], [], n_clusters, threads=max(1, threads),
                                     filters=[(h.filter_file, tb.filter_ptr(i)) for i, h in enumerate(handles)])
                sc.load_cbcl_batch([(handles[i].cbcl_path(cyc), int(handles[i].tile), tb.filter_ptr(i), dst)
                                    for i, cyc, dst in jobs], n_clusters, threads=max(1, threads),
                                   well_stride=interleave)
            planes = [pool.submit(load_all)]
        elif batch:
            # the whole batch - planes and filters - goes through one call: the library's threads read
            # the files, the GPU inflates the .bcl.gz ones (wd_load_tile_files_batch)
            def load_all():
                missing = sc.load_bcl_gz_batch([handles[i].plane_path(cyc) for i, cyc, _ in jobs],
                                               [dst for _, _, dst in jobs], n_clusters,
                                               threads=max(1, threads), missing_ok=True, well_stride=interleave,
                                               filters=[(h.filter_file, tb.filter_ptr(i)) for i, h in enumerate(handles)],
                                               tile_of=[i for i, _, _ in jobs] + list(range(len(handles))))
                for j in missing:           # (a run is .bcl.gz or .cbcl, never both: this loop is for the odd file)
                    load(*jobs[j])
            planes = [pool.submit(load_all)]
        else:
            planes = [pool.submit(load, *job) for job in jobs]
        return _Loading((lane, chunk), handles, tb, filt + planes)

    def start_ahead(batch):
        """start(), for a batch that is not yet the current one: whatever submitting it raises (a lane
        directory that does not exist, no .filter file, a tile of another size, an index beyond the tile)
        is kept and raised when the batch's turn comes - the reference reports lane n before it touches
        lane n + 1 (count_well_duplicates.py:207-226, :269), so an error of a later lane must not cost
        an earlier lane its report."""
        try:
            return start(batch)
        except Exception as e:              # noqa: BLE001 - re-raised by _Loading.wait()
            return _Loading(batch, None, None, [], error=e)

    def release(tb, keep=False):
        live.remove(tb)
        for mine, its_spare in [(tb, spare)] + [(s.tb.pop(id(tb), None), s.spare) for s in sides]:
            if mine is not None and keep:
                its_spare.append(mine)
            elif mine is not None:
                mine.free()

    try:
        # three batches on their way at any time: one's files are read and copied while the one before
        # is still being inflated (the GPU decoder's time per batch does not shrink with the batch)
        # and the one before that is scanned and reported - the library serves the batch calls in
        # the order they were made
        depth = 3 if overlap else 1
        ahead = []
        for b in batches[:depth]:
            ahead.append(start_ahead(b))
        for bi in range(len(batches)):
            cur = ahead.pop(0)
            cur.wait()
            _lap("batch %d: planes in HBM" % bi)
            (lane, chunk), tb = cur.chunk, cur.tb
            n_clusters = tb.N
            if want_log:
                sc.hitlog_enable(max(1024, int(nbr.size) * len(chunk)))
            if dup_sets:
                blocks, set_rows, labels = tb.dup_sets(mode, k, labels=dup_sets > 1)
                for i, t in enumerate(chunk):
                    into["sets"][(lane, t)] = report.DupSetCounts.from_block(set_rows[i], levels)
                    if labels is not None:
                        into["members"][(lane, t)] = set_members(labels[i])
            else:
                blocks, _ = tb.count(mode, k)
            _lap("batch %d: scanned" % bi)
            if tile_dups:
                td_rows, td_labels = tb.tile_dups(labels=tile_dups > 1)
                for i, t in enumerate(chunk):
                    into["tdups"][(lane, t)] = report.TileDupCounts.from_block(td_rows[i], levels, wells=n_clusters)
                    if td_labels is not None:
                        into["tmembers"][(lane, t)] = set_members(td_labels[i])
                _lap("batch %d: read classes" % bi)
                if tile_near:
                    tn_rows, tn_labels = tb.tile_near_dups(tile_near, labels=tile_dups > 1, pair_budget=pair_budget)
                    for i, t in enumerate(chunk):
                        into["tnear"][(lane, t)] = report.TileNearCounts.from_block(tn_rows[i], levels, wells=n_clusters)
                        if tn_labels is not None:
                            ws, clusters = set_members(tn_labels[i])
                            into["tnmembers"][(lane, t)] = (ws, td_labels[i][ws], clusters)
                    _lap("batch %d: read clusters" % bi)
            if lane_dups:
                names = tiles_of_lane[lane]
                ld = lane_acc["ld"]
                if lane_acc["lane"] != lane:
                    if ld is not None and (ld.N, ld.max_tiles, ld.L) == (n_clusters, len(names), len(cycle_list)):
                        ld.restart()            # (the workspace of the lane before: freeing it would wait for the loaders)
                    else:
                        if ld is not None:
                            ld.close()
                        lane_acc["ld"] = None
                        ld = lane_acc["ld"] = LaneDups(sc, n_clusters, len(names), len(cycle_list))
                        for name, argument in begins:
                            getattr(ld, name + "_begin")(argument)
                    lane_acc["lane"] = lane
                slots = [names.index(t) for t in chunk]
                ld.add(tb, slots)
                if qual_edges is not None:
                    ld.qual_add(tb, slots)
                for s in sides:
                    getattr(ld, s.name + "_add")(s.tb[id(tb)], slots)
                if last_batch_of[lane] == bi:
                    got = ld.finish(labels=lane_dups > 1, hamming=lane_near, pair_budget=lane_pair_budget)
                    lane_row, tile_rows, lane_labels = got[:3]
                    into["ldups"][lane] = report.LaneDupCounts.from_rows(lane_row, tile_rows, names)
                    if lane_near:
                        into["lnear"][lane] = report.LaneNearCounts.from_rows(got[3], got[4], names)
                        if lane_labels is not None:
                            into["lmembers"][lane] = (names,) + lane_cluster_members(lane_labels, got[5])
                    elif lane_labels is not None:
                        into["lmembers"][lane] = (names,) + lane_members(lane_labels)
                    listing = final = None
                    if index_cycles:
                        final = got[3] if lane_near else lane_row      # the row of the labels the lane was left with
                        listing = ld.index_finish(*index_listing(index_share, int(final[0])))
                        into["lindex"][lane] = report.LaneIndexCounts.from_rows(*listing, index_lengths, final[0], final[1])
                        if lane_labels is not None:
                            m = into["lmembers"][lane]
                            into["lmindex"][lane] = ld.index_keys()[m[1] * n_clusters + m[2]]
                    del lane_labels, got        # (lane-sized; `final` is a row of counters)
                    context = SimpleNamespace(names=names, n_clusters=n_clusters, cycle_list=cycle_list, lane_near=lane_near,
                                              left=into["lnear"][lane] if lane_near else into["ldups"][lane],
                                              listing=listing, final=final, index_lengths=index_lengths,
                                              reader=reader, lane=lane)
                    for p, params in lane_passes:
                        into[p.key][lane] = p.run(ld, context, params)
                _lap("batch %d: lane classes" % bi)
            hits, seq_bytes, seq_wells = None, {}, {}
            if want_log:
                hits, total = sc.hitlog_fetch(max(1024, int(nbr.size) * len(chunk)))
                sc.hitlog_enable(0)
                order = np.lexsort((hits["slot"], hits["target"], hits["tile"]))
                hits = hits[order]
                # the bytes of the wells that figure in a duplicate come back, for the stderr log (:260-262):
                # a few hundred per tile, not the 200 000 some target touches
                for i in np.unique(hits["tile"]):
                    sel = hits[hits["tile"] == i]
                    ws = np.unique(np.concatenate([centre[sel["target"]], nbr[sel["slot"]]]).astype(np.int64))
                    seq_wells[int(i)] = ws
                    seq_bytes[int(i)] = sc.gather_wells_batch(tb, int(i), ws)
            release(tb, keep=bi + depth < len(batches))
            if overlap and bi + depth < len(batches):
                ahead.append(start_ahead(batches[bi + depth]))
            for i, t in enumerate(chunk):
                counts[(lane, t)] = report.TileCounts.from_block(blocks[i], levels)
                if want_log:
                    lines = ["Reading tile %s in lane %s" % (t, lane),
                             "Got %i sequences from %i contiguous cycle ranges." % (
                                 wells.size * want_log, want_log)]
                    sel = hits[hits["tile"] == i]
                    if sel.size:
                        # every well of the tile's duplicates decoded once, the three lines per duplicate
                        # (:260-262) put together from those strings
                        sb, sw = seq_bytes[i], seq_wells[i]
                        seqs = _decode_rows(sb)
                        cw, ww = centre[sel["target"]].astype(np.int64), nbr[sel["slot"]].astype(np.int64)
                        ci, wi = np.searchsorted(sw, cw), np.searchsorted(sw, ww)
                        for c, w, a, b, d in zip(cw.tolist(), ww.tolist(), ci.tolist(), wi.tolist(), sel["dist"].tolist()):
                            lines.append("center seq at {:>07}: {}".format(c, seqs[a]))
                            lines.append("well seq at   {:>07}: {}".format(w, seqs[b]))
                            lines.append("edit distance: {}".format(d))
                    logs[(lane, t)] = lines
            if lane_done is not None and last_batch_of[lane] == bi:
                lane_done(lane)
            if not overlap and bi + 1 < len(batches):
                ahead.append(start_ahead(batches[bi + 1]))
    finally:
        # queued loads are dropped, running ones finish - only then may their targets go
        pool.shutdown(wait=True, cancel_futures=True)
        if lane_acc["ld"] is not None:      # finished or half built
            lane_acc["ld"].close()
        for tb in list(live):
            release(tb)
        for tb in spare + [stb for s in sides for stb in s.spare]:
            tb.free()
    return counts, logs


def write_set_members(path, members, column="set"):
    """--dup-sets-out (--tile-dups-out: column "class"): lane, tile, well, set of every well in a set of two or
    more, by lane, tile, well."""
    with open(path, "w") as fh:
        fh.write("lane\ttile\twell\t%s\n" % column)
        for lane, tile in sorted(members, key=lambda lt: (str(lt[0]), str(lt[1]))):
            wells, labels = members[(lane, tile)]
            fh.writelines("%s\t%s\t%d\t%d\n" % (lane, tile, w, s) for w, s in zip(wells.tolist(), labels.tolist()))


def write_cluster_members(path, members):
    """--tile-dups-out under --tile-dups-hamming: lane, tile, well, class, cluster of every well in a cluster of
    two or more, by lane, tile, well (class: the well's own index when it is in no class)."""
    with open(path, "w") as fh:
        fh.write("lane\ttile\twell\tclass\tcluster\n")
        for lane, tile in sorted(members, key=lambda lt: (str(lt[0]), str(lt[1]))):
            wells, classes, clusters = members[(lane, tile)]
            fh.writelines("%s\t%s\t%d\t%d\t%d\n" % (lane, tile, w, c, s)
                          for w, c, s in zip(wells.tolist(), classes.tolist(), clusters.tolist()))


def write_lane_members(path, members, index=None):
    """--lane-dups-out: lane, tile, well, class_tile, class_well of every well in a lane class, by lane, then in
    the order of the lane's tiles, then by well.  members[lane] = (tile names by index, tile index, well, class
    tile index, class well) - or, under --lane-dups-hamming, those and (cluster tile index, cluster well) of every
    well in a lane cluster, which makes two more columns.  index (--lane-dups-index) = (cycles per index range,
    {lane: the index key of every row}): a last column `index`, the well's index read as bases."""
    with open(path, "w") as fh:
        near = any(len(m) == 7 for m in members.values())
        fh.write("lane\ttile\twell\tclass_tile\tclass_well%s%s\n" % ("\tcluster_tile\tcluster_well" if near else "",
                                                                   "\tindex" if index else ""))
        for lane in sorted(members, key=str):
            names, cols = members[lane][0], [c.tolist() for c in members[lane][1:]]
            if index:
                reads = {int(k): report.index_bases(k, index[0]) for k in np.unique(index[1][lane])}
                cols.append([reads[k] for k in index[1][lane].tolist()])
                fmt = "%s\t%s\t%d\t%s\t%d" + ("\t%s\t%d" if near else "") + "\t%s\n"
                fh.writelines(fmt % ((lane, names[r[0]], r[1], names[r[2]], r[3]) +
                                     ((names[r[4]], r[5]) if near else ()) + (r[-1],)) for r in zip(*cols))
                continue
            if near:        # (--lane-dups-hamming: the wells in a lane cluster, their class and their cluster)
                fh.writelines("%s\t%s\t%d\t%s\t%d\t%s\t%d\n" % (lane, names[a], b, names[c], d, names[e], f)
                              for a, b, c, d, e, f in zip(*cols))
            else:
                fh.writelines("%s\t%s\t%d\t%s\t%d\n" % (lane, names[a], b, names[c], d) for a, b, c, d in zip(*cols))


def main(argv=None, exiting=False):
    """exiting=True (what `python -m well_duplicates_amd.count_well_duplicates` passes): the process ends
    when this returns, so the GPU context is closed without freeing its buffers one by one."""
    if os.environ.get("WD_CLI_TIMING"):
        import time
        _T0[0] = time.perf_counter()
    args = parse_args(argv)
    args.exiting = bool(exiting)
    log = (lambda msg: None) if args.quiet else (lambda msg: print(str(msg), file=sys.stderr))

    # The GPU context first (this thread's current device is its device from here on), so that the batch
    # loaders' pinned ring - pinning 64 MB takes 25 ms - can be set up by a thread of its own while this one
    # parses the targets file and lists the run directory (the call releases the GIL).  Whatever goes wrong
    # here is raised where the scanner is needed: under torchrun that is inside the ranks' failure protocol.
    from . import dist as wdist
    rank, world, local_rank = wdist.env_rank()
    device = args.device if args.device is not None else (local_rank if world > 1 else 0)
    early = {"sc": None, "err": None}
    import threading
    opener = None
    try:
        early["sc"] = Scanner(device)
        if os.environ.get("WD_INFLATE_CHUNK_MB"):            # (measurements: the pinned ring's chunk size)
            early["sc"].set_option("inflate_chunk_mb", int(os.environ["WD_INFLATE_CHUNK_MB"]))
        if not args.host_inflate:
            def warm():
                try:
                    early["sc"].set_option("inflate_warm", 1)
                except Exception as e:          # noqa: BLE001
                    early["err"] = e
            opener = threading.Thread(target=warm, name="wd-ingest-warm-up")
            opener.start()
    except Exception as e:                      # noqa: BLE001
        early["err"] = e
    try:
        return _main(args, log, wdist, rank, world, device, opener, early)
    finally:
        if opener is not None:
            opener.join()
        if early["sc"] is not None:
            early["sc"].close(exiting=args.exiting)     # (a second close is a no-op)


def _main(args, log, wdist, rank, world, device, opener, early):

    # Under torchrun the process group comes FIRST: whatever a rank's setup raises after this point - a
    # run directory it cannot list, a targets file it cannot parse, a GPU it cannot use - goes through the
    # ranks' one failure flag below, and the others end with it instead of waiting in the rendezvous for a
    # rank that has already left (bcl_direct_reader.py:59-70 and target.py:6-40 raise on the first bad path).
    if world > 1:
        import torch
        import torch.distributed as tdist
        if args.dist_backend == "nccl":
            torch.cuda.set_device(device)
            tdist.init_process_group("nccl", device_id=torch.device("cuda", device))
        else:
            tdist.init_process_group("gloo")            # gloo; "wd": the bootstrap channel of the unique id
    levels = args.level
    out_fh = None
    try:
        # a rank whose setup fails (an unreadable run directory, no memory on its GPU, a bad device, targets
        # it cannot upload) must not leave the others waiting in the first collective: setup and scan feed
        # ONE failure flag
        sc, err = None, None
        lanes, tiles, cycles, cycle_list, mode, k = [], [], [], [], 0, 0
        reader = csr = xy = None
        wells = np.zeros(0, dtype=np.int64)
        n_targets = 0
        try:
            lanes = args.lane.split(",") if args.lane else range(1, 8 + 1)
            tiles = workload.tiles_for_stype(args.stype)
            if args.tile_id:
                tiles = workload.filter_tiles(tiles, args.tile_id, args.stype)
            cycles = workload.parse_cycles(args.start, args.end, args.cycles)
            cycle_list = [c for s, e in cycles for c in range(s, e)]
            mode, k = compare_mode(args.edit_distance, args.hamming)

            if args.all_wells:
                from . import cluster_indexes
                xy = cluster_indexes.read_slocs(args.slocs or os.path.join(args.run, "Data", "Intensities", "s.locs"))
            else:
                # a regular targets file is parsed in bulk; anything else goes through the reference's parser,
                # which raises what the reference raises
                fast = load_targets_csr(args.coord_file, args.level, args.sample_size)
                if fast is not None:
                    n_parsed, csr = fast[0], fast[1:]
                else:
                    targets = load_targets(filename=args.coord_file, levels=args.level + 1, limit=args.sample_size)
                    n_parsed, csr = len(targets), targets.to_csr(args.level)
                # every well some target touches = targets.get_all_indices(), sorted (the rings loaded are 1..-l)
                wells = np.unique(np.concatenate([csr[0], csr[2]]).astype(np.int64))
            run_path = args.run
            if os.environ.get("WD_TEST_RUN_SUFFIX"):        # (tests: "<rank>:<suffix>" breaks one rank's run path)
                r_, _, suffix = os.environ["WD_TEST_RUN_SUFFIX"].partition(":")
                if int(r_) == rank:
                    run_path = run_path + suffix
            reader = bcl_direct_reader.BCLReader(run_path)
            _lap("targets file, run directory")
            if args.output and rank == 0:
                out_fh = open(args.output, "w")
            if opener is not None:
                opener.join()
            if early["err"] is not None:
                raise early["err"]
            sc = early["sc"]
            if args.all_wells:
                n_targets, n_slots = sc.targets_from_coords(xy[0], xy[1], None, levels=levels)
                log("All %i wells are centres: %i neighbour slots in %i levels" % (n_targets, n_slots, levels))
                # the scan needs nothing of the rings on the host; the log of single duplicates is off
                csr = (np.zeros(0, np.int32), np.zeros((0, levels + 1), np.int32), np.zeros(0, np.int32))
            else:
                n_targets = n_parsed
                sc.set_targets(*csr)
        except Exception as e:              # noqa: BLE001 - re-raised below, on every rank
            err = e
        try:
            _lap("context, targets on the GPU")
            # (lane, tile) items are independent (count_well_duplicates.py:207-226): the flat list
            # is block-partitioned over the ranks, every rank scans its share lane by lane, and ONE
            # all-reduce of the [items, 1 + 5 levels] counter block (plus one gather of the log
            # lines) makes rank 0 hold what the single-process run holds
            lanes = list(lanes)
            items = [(lane, t) for lane in lanes for t in tiles]
            pos = {item: i for i, item in enumerate(items)}
            mine = wdist.shard(items, rank, world)
            ncnt = 1 + 5 * levels
            # --dup-sets: the duplicate sets' counters ride in the same row (one all-reduce either way)
            nsets = 1 + 3 * levels + len(report.SIZE_BIN_NAMES) if args.dup_sets else 0
            # --tile-dups: and the read classes' columns behind them
            ntd = 4 + 2 * levels + len(report.CLASS_BIN_NAMES) if args.tile_dups else 0
            # --tile-dups-hamming: and the clusters' behind those
            near_k = args.tile_dups_hamming or 0
            lane_near_k = args.lane_dups_hamming or 0
            index_ranges = workload.parse_cycles(0, 0, args.lane_dups_index) if args.lane_dups_index else []
            index_cycles = [c for s, e in index_ranges for c in range(s, e)]
            # the passes after a lane's finish that the command line asks for, with their parameters
            run = SimpleNamespace(xy=xy, cycle_list=cycle_list, n_wells=n_targets, n_tiles=len(tiles))
            lane_passes = resolve_passes(args, run) if err is None else []
            ntn = 5 + 2 * levels + len(report.CLASS_BIN_NAMES) if near_k else 0
            rows = np.zeros((len(mine), ncnt + nsets + ntd + ntn), dtype=np.int64)
            logs = {}

            def emit(lane, block):          # a finished lane: its log lines, then its report (:269)
                counts = {t: report.TileCounts.from_block(block[pos[(lane, t)]][:ncnt], levels) for t in tiles}
                for t in tiles:
                    lines = logs.get((lane, t))
                    if lines:
                        log("\n".join(lines))
                report.write_report(lane, n_targets, counts, verbose=not args.summary_only,
                                    strict=args.strict, out=out_fh)
                if args.dup_sets:
                    sets = {t: report.DupSetCounts.from_block(block[pos[(lane, t)]][ncnt:ncnt + nsets], levels)
                            for t in tiles}
                    report.write_dup_sets(lane, sets, verbose=not args.summary_only, out=out_fh, levels=levels)
                if args.tile_dups:          # (every well is a target: n_targets is the tile's size)
                    tds = {t: report.TileDupCounts.from_block(block[pos[(lane, t)]][ncnt + nsets:ncnt + nsets + ntd],
                                                              levels, wells=n_targets) for t in tiles}
                    report.write_tile_dups(lane, tds, verbose=not args.summary_only, out=out_fh, levels=levels)
                if near_k:
                    tns = {t: report.TileNearCounts.from_block(block[pos[(lane, t)]][ncnt + nsets + ntd:], levels,
                                                               wells=n_targets) for t in tiles}
                    equal = report.TileDupCounts.zeros(levels)
                    for t in tiles:
                        equal = equal + tds[t]
                    report.write_tile_near_dups(lane, near_k, tns, verbose=not args.summary_only, out=out_fh,
                                                levels=levels, equal=equal)
                if args.lane_dups:          # (single process: the lane's counts never travel through `block`)
                    report.write_lane_dups(lane, results["ldups"][lane], verbose=not args.summary_only, out=out_fh)
                if lane_near_k:
                    report.write_lane_near_dups(lane, lane_near_k, results["lnear"][lane], verbose=not args.summary_only,
                                                out=out_fh, equal=results["ldups"][lane])
                if index_cycles:
                    report.write_lane_index_dups(lane, results["lindex"][lane], hamming=lane_near_k, out=out_fh)
                for p, _ in lane_passes:
                    p.write(lane, results[p.key][lane], verbose=not args.summary_only, out=out_fh)

            try:
                lane_tiles = [(lane, [t for (ln, t) in mine if ln == lane]) for lane in lanes] if err is None else []
                where = {item: i for i, item in enumerate(mine)}
                # scan_lanes fills these, lane_done reads them
                results = {"counts": {}, "logs": {}, "sets": {}, "members": {}, "tdups": {}, "tmembers": {},
                           "tnear": {}, "tnmembers": {}, "ldups": {}, "lmembers": {}, "lnear": {}, "lindex": {},
                           "lmindex": {}, **{p.key: {} for p in ALL_PASSES}}
                def lane_done(lane):
                    for t in dict(lane_tiles)[lane]:
                        c = results["counts"][(lane, t)]
                        rows[where[(lane, t)]][:ncnt] = [c.targets] + c.wells + c.dups + c.hit + c.first + c.last
                        if args.dup_sets:
                            d = results["sets"][(lane, t)]
                            rows[where[(lane, t)]][ncnt:ncnt + nsets] = [d.pf] + d.sets + d.in_sets + d.redundant + d.sizes
                        if args.tile_dups:
                            rows[where[(lane, t)]][ncnt + nsets:ncnt + nsets + ntd] = results["tdups"][(lane, t)].to_block()
                        if near_k:
                            rows[where[(lane, t)]][ncnt + nsets + ntd:] = results["tnear"][(lane, t)].to_block()
                        if (lane, t) in results["logs"]:
                            logs[(lane, t)] = results["logs"][(lane, t)]
                    if world == 1:          # as the reference: a lane is reported when it is done
                        emit(lane, rows)

                if err is None and args.lane_dups:
                    # before anything is loaded: a lane's accumulator has to fit beside the batches
                    import torch
                    parts = {"scratch": sc.lane_near_scratch_bytes(n_targets, len(tiles), len(cycle_list), lane_near_k),
                             "index": sc.lane_index_workspace_bytes(n_targets, len(tiles), len(index_cycles))
                             if index_cycles else 0}
                    for p, params in lane_passes:       # (a region two passes share comes under one keyword, once)
                        parts.update(p.bytes(sc, run, params))
                    check_lane_dups_fits(sc.lane_dups_workspace_bytes(n_targets, len(tiles), len(cycle_list)),
                                         torch.cuda.mem_get_info(device)[0], len(tiles), n_targets, len(cycle_list), **parts)
                if err is None:             # (a rank whose setup failed has nothing to scan: it goes to the flag)
                    scan_lanes(sc, reader, lane_tiles, cycle_list, mode, k, csr, wells,
                               max(0, args.tile_batch), args.threads,
                               0 if (args.quiet or args.all_wells) else len(cycles),
                               overlap=not args.serial_ingest,
                               interleave=resident_layout(args, mode, k, csr, reader, lanes, tiles, cycle_list),
                               gpu_inflate=not args.host_inflate, lane_done=lane_done, into=results,
                               dup_sets=(2 if args.dup_sets_out else 1) if args.dup_sets else 0,
                               tile_dups=(2 if args.tile_dups_out else 1) if args.tile_dups else 0,
                               tile_near=near_k, pair_budget=args.tile_dups_pair_budget,
                               lane_dups=(2 if args.lane_dups_out else 1) if args.lane_dups else 0,
                               lane_near=lane_near_k, lane_pair_budget=args.lane_dups_pair_budget,
                               lane_index=(index_cycles, [e - s for s, e in index_ranges],
                                           args.lane_dups_index_min_share) if index_cycles else None,
                               lane_passes=lane_passes)
                    if args.dup_sets_out:
                        write_set_members(args.dup_sets_out, results["members"])
                    if args.tile_dups_out and near_k:
                        write_cluster_members(args.tile_dups_out, results["tnmembers"])
                    elif args.tile_dups_out:
                        write_set_members(args.tile_dups_out, results["tmembers"], column="class")
                    for p in ALL_PASSES:
                        path = getattr(args, dest(p.out[0])) if p.out else None
                        if path:
                            with open(path, "w") as fh:
                                for i, lane in enumerate(sorted(results[p.key], key=lanes.index)):
                                    p.out[1](lane, results[p.key][lane], fh, header=i == 0)
                    if args.lane_dups_out:
                        write_lane_members(args.lane_dups_out, results["lmembers"],
                                           index=([e - s for s, e in index_ranges], results["lmindex"])
                                           if index_cycles else None)
            except Exception as e:          # noqa: BLE001 - re-raised below, on every rank
                err = e
            if world > 1:
                # a rank that failed must not leave the others waiting in the collective
                failed = wdist.any_rank_failed(err is not None, world, backend=args.dist_backend, device=device)
                if failed:
                    raise err if err is not None else RuntimeError("another rank failed; see its message")
                full = wdist.merge_blocks(rows, len(items), rank, world, backend=args.dist_backend,
                                          device=device, scanner=sc)
                logs = wdist.gather_dicts(logs, world)
                if rank == 0:
                    for lane in lanes:
                        emit(lane, full)
            elif err is not None:
                raise err
        finally:
            _lap("reports")
            if sc is not None:
                sc.close(exiting=args.exiting)
    finally:
        _lap("context closed")
        if out_fh:
            out_fh.close()
        if world > 1:
            import torch.distributed as tdist
            tdist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main(exiting=True))
